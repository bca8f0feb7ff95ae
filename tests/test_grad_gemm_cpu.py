"""CPU tier of the GEMM gradient kernel (NF_CFG_GRAD_GEMM, csrc/nf_grad_gemm.hip; coupling widths 33 .. 512): what
``nf_grad_supported`` accepts and refuses under the flag, that the flag changes nothing at widths up to 32, the parameter image
(csrc/nf_gemm_layout.h, NFGG_*) un-permuted and held bit for bit to the folded model, the embedded test model of the full-patch GPU
cases, and the Python keyword.  No device is touched.

``embedded_variables(v32, W)``: the variables of a width-32 model placed into a width-W model whose other channels are dead (zero
``l_1/W`` columns, zero biases, BN mean 0 and variance 1, zero ``l_2/W`` rows and columns, zero ``l_last/W`` rows; the
edge-indicator row moves to index W).  The 32 live channels sit at scattered positions, one per slab of W / 32 channels, so that
every K slab and every accumulator tile of the wide kernel carries one.  The function is that of the width-32 model.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs
from nll_grad_ref import NllGradRef
from test_grad_wide_layout_cpu import NF_OP_COUPLING_FWD, NF_OP_MIX, NF_OP_SCALE, _fold, _generic, chan
from test_grad_wide_supported_cpu import paper_like_variables
from test_nll_grad_ref_cpu import WIDE_ARCH, _supported

ISO, CAM = 800.0, 2.0


def pad_width(w):
    return 64 if w <= 64 else 128 if w <= 128 else 256 if w <= 256 else 512


def embedded_positions(W):
    slab = W // 32
    return np.array([slab * i + (5 * i + 3) % slab for i in range(32)])


def embedded_variables(v32, W):
    pos = embedded_positions(W)
    out = {}
    for k, a in v32.items():
        a = np.asarray(a)
        if k.endswith("l_1/W"):
            b = np.zeros(a.shape[:3] + (W,), a.dtype)
            b[..., pos] = a
        elif k.endswith("l_1/b") or k.endswith("l_2/b"):
            b = np.zeros(a.shape[:3] + (W,), a.dtype)
            b[..., pos] = a
        elif k.endswith("l_2/W"):
            b = np.zeros((1, 1, W, W), a.dtype)
            b[0, 0][np.ix_(pos, pos)] = a[0, 0]
        elif k.endswith("l_last/W"):
            b = np.zeros((3, 3, W + 1, 4), a.dtype)
            b[:, :, pos] = a[:, :, :32]
            b[:, :, W] = a[:, :, 32]
        elif k.endswith("/mean") and "bn_nvp_conv" in k:
            b = np.zeros((W,), a.dtype)
            b[pos] = a
        elif k.endswith("/var") and "bn_nvp_conv" in k:
            b = np.ones((W,), a.dtype)
            b[pos] = a
        else:
            b = a.copy()
        out[k] = b
    return out


# ---- nf_grad_supported under the flag ----------------------------------------------------------------------------------------
_VARS = {}


def _vars(arch, width):
    if (arch, width) not in _VARS:
        _VARS[(arch, width)] = paper_like_variables(arch, width)
    return _VARS[(arch, width)]


@pytest.mark.parametrize("arch,width,hw", [(WIDE_ARCH, 33, (16, 16)), (WIDE_ARCH, 64, (32, 32)), (WIDE_ARCH, 200, (9, 13)),
                                           (WIDE_ARCH, 512, (32, 32)), (WIDE_ARCH, 512, (1, 1)), (FULL_ARCH, 512, (32, 32))])
def test_supported_with_the_flag(arch, width, hw):
    from noise_flow_amd import _lib
    rc, msg = _supported(arch, _vars(arch, width), width, hw, _lib.NF_CFG_GRAD_GEMM)
    assert rc == 0, msg
    rc, msg = _supported(arch, _vars(arch, width), width, hw, 0)   # and stays refused without it, in today's words
    assert rc == _lib.NF_EINVAL and "the GEMM families have no gradient kernel" in msg, msg


@pytest.mark.parametrize("hw,extra,word", [((33, 32), "", "32x32"), ((64, 64), "", "32x32"), ((96, 80), "TILED", "32x32"),
                                           ((96, 80), "TILED_WIDE", "32x32"), ((16, 16), "FP16_CNN", "fp32")])
def test_refusals_with_the_flag(hw, extra, word):
    from noise_flow_amd import _lib
    flags = _lib.NF_CFG_GRAD_GEMM | {"": 0, "TILED": _lib.NF_CFG_GRAD_TILED, "TILED_WIDE": _lib.NF_CFG_GRAD_TILED_WIDE,
                                     "FP16_CNN": _lib.NF_CFG_FP16_CNN}[extra]
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 64), 64, hw, flags)
    assert rc == _lib.NF_EINVAL
    assert msg and word in msg and "NF_CFG_GRAD_GEMM" in msg, msg
    if extra.startswith("TILED"):
        assert "no tile mode" in msg, msg


def test_coupling_limit_is_named():
    """At most 32 couplings (nf_gemm_layout.h, NFGG_MAX_COUPLINGS): the architecture grammar cannot exceed it (a coupling comes with
    its 1x1 matrix, 64 ops in all), a layer list through the C ABI can — 33 bare couplings sharing one parameter block."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    arch = "unc"
    layers, descs, flat = params.pack(arch, _vars(arch, 64), 64, "loss_first")
    cpl = [d for d in descs if d.width == 64][0]
    for n, want in ((32, 0), (33, _lib.NF_EINVAL)):
        many = (_lib.nf_layer_desc * n)(*[_lib.nf_layer_desc(cpl.type, cpl.width, cpl.param_offset) for _ in range(n)])
        cfg = _lib.nf_config(8, 8, 4, n, -1, _lib.NF_CFG_GRAD_GEMM)
        rc = lib.nf_grad_supported(C.byref(cfg), many, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
        msg = (lib.nf_last_error() or b"").decode()
        assert rc == want, (n, rc, msg)
        if want:
            assert "32 couplings" in msg, msg


@pytest.mark.parametrize("width,hw", [(4, (32, 32)), (4, (64, 64)), (32, (16, 16)), (32, (32, 32)), (16, (64, 64))])
def test_flag_without_effect_up_to_width_32(width, hw):
    """nf_grad_supported (code and message) and nf_grad_fold (path, program, block bytes) are those of flags = 0."""
    from noise_flow_amd import _lib
    a = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, 0)
    b = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, _lib.NF_CFG_GRAD_GEMM)
    assert a == b, (a, b)
    for extra in (0, _lib.NF_CFG_GRAD_MFMA):
        fa, fb = _fold(width, hw, extra), _fold(width, hw, extra | _lib.NF_CFG_GRAD_GEMM)
        if fa[1] is None:
            assert fb[1] is None and fa[0] == fb[0]
        else:
            assert fa[0][0] == fb[0][0] and fa[0][1] == fb[0][1] and fa[0][2].tobytes() == fb[0][2].tobytes()


# ---- the parameter image ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [96, 300])
def test_gemm_gradient_block_unpermutes_to_the_folded_model(width):
    """Every image of the block against the generic block of nf_fold_params, bit for bit; a padded channel is exactly zero."""
    from noise_flow_amd import _lib
    w, wp = width, pad_width(width)
    MT, KC = wp // 32, wp // 8
    (path, gops, blk), (fops, gen) = _fold(width, (16, 16), _lib.NF_CFG_GRAD_GEMM)
    assert path == _lib.NF_GRAD_PATH_GEMM
    assert [t for t, _ in gops] == [t for t, _ in fops]
    img_size = MT * 832 + wp * wp + MT * (1024 + 128)
    FWD, BWD = 68, 68 + img_size
    SIZE = BWD + MT * (1280 + 1024) + wp * wp
    A1, B1, B2, A2, A3, A3C = 0, MT * 768, MT * 800, MT * 832, MT * 832 + wp * wp, MT * 832 + wp * wp + MT * 1024
    A3T, A2T, A1T = 0, MT * 1280, MT * 1280 + wp * wp
    lanes = np.arange(64)
    g_of, i_of = lanes >> 5, lanes & 31

    def padded(a, axes):   # the generic array zero-padded from w to wp along `axes`
        pad = [(0, 0)] * a.ndim
        for ax in axes:
            pad[ax] = (0, wp - w)
        return np.pad(a, pad)

    n_cpl = 0
    for (t, off), (_, foff) in zip(gops, fops):
        if t == NF_OP_MIX:
            A, Ai = blk[off:off + 16].reshape(4, 4).astype(np.float64), blk[off + 16:off + 32].reshape(4, 4).astype(np.float64)
            assert np.array_equal(blk[off:off + 16], gen[foff:foff + 16]) and np.abs(A @ Ai - np.eye(4)).max() < 1e-5
        elif t == NF_OP_SCALE:
            assert blk[off] == gen[foff] and abs(float(blk[off]) * float(blk[off + 1]) - 1.0) < 1e-6
        elif t == NF_OP_COUPLING_FWD:
            n_cpl += 1
            img = blk[off:off + SIZE]
            E, W3, W1, b1, W2, b2, sc = _generic(gen[foff:], w)
            W3p, W1p, W2p, b1p, b2p = padded(W3, (1,)), padded(W1, (2,)), padded(W2, (0, 1)), padded(b1, (0,)), padded(b2, (0,))
            assert np.array_equal(img[:64], E) and img[64] == sc and not img[65:68].any()
            f, b = img[FWD:BWD], img[BWD:]
            for m in range(MT):
                ch = 32 * m + i_of   # the lane's channel of tile m
                for s in range(12):   # l_1: step = tap, K slice = input channel
                    got = f[A1 + ((m * 3 + (s >> 2)) * 64 + lanes) * 4 + (s & 3)]
                    assert np.array_equal(got, W1p[s, g_of, ch] if s < 9 else np.zeros(64, np.float32)), ("A1", m, s)
                for s in range(20):   # l_last^T: step = (tap, element pair), K slice = element of the pair
                    got = b[A3T + ((m * 5 + (s >> 2)) * 64 + lanes) * 4 + (s & 3)]
                    assert np.array_equal(got, W3p[s >> 1, ch, 2 * (s & 1) + g_of] if s < 18 else np.zeros(64, np.float32)), ("A3T", m, s)
                for kk in range(4 * KC):   # l_2 and l_2^T: K step kk consumes register kk % 16 of tile kk / 16
                    kch = 32 * (kk // 16) + chan(kk % 16, g_of)
                    at = ((m * KC + (kk >> 2)) * 64 + lanes) * 4 + (kk & 3)
                    assert np.array_equal(f[A2 + at], W2p[kch, ch]), ("A2", m, kk)
                    assert np.array_equal(b[A2T + at], W2p[ch, kch]), ("A2T", m, kk)
                for v in range(16):   # l_last as P (rows 4 tap + j, taps 0 .. 7) and l_1^T as D18 (rows 2 tap + ch): K = the channels of tile m
                    kch = 32 * m + chan(v, g_of)
                    at = ((m * 4 + (v >> 2)) * 64 + lanes) * 4 + (v & 3)
                    assert np.array_equal(f[A3 + at], W3p[i_of >> 2, kch, i_of & 3]), ("A3", m, v)
                    want = np.where(i_of < 18, W1p[np.minimum(i_of, 17) >> 1, np.minimum(i_of, 17) & 1, kch], np.float32(0))
                    assert np.array_equal(b[A1T + at], want), ("A1T", m, v)
                    for g in range(2):
                        for j in range(4):
                            assert f[A3C + ((m * 4 + (v >> 2)) * 8 + g * 4 + j) * 4 + (v & 3)] == W3p[8, 32 * m + chan(v, g), j]
                for g in range(2):
                    for v in range(16):
                        assert f[B1 + m * 32 + g * 16 + v] == b1p[32 * m + chan(v, g)] and f[B2 + m * 32 + g * 16 + v] == b2p[32 * m + chan(v, g)]
            # padded channels: every row, column and bias beyond w is exactly zero — which the comparisons above already say element
            # by element (the padded generic arrays are zero there); the count of non-zeros says it once more for the whole image
            assert np.count_nonzero(f) <= np.count_nonzero(W1) + np.count_nonzero(W2) + np.count_nonzero(W3) + np.count_nonzero(b1) + np.count_nonzero(b2)
            assert np.count_nonzero(b) <= np.count_nonzero(W1) + np.count_nonzero(W2) + np.count_nonzero(W3)
    assert n_cpl == 3
    assert blk.size >= 3 * SIZE


# ---- the embedded model -------------------------------------------------------------------------------------------------------
def test_embedded_model_is_the_width_32_model():
    v32 = paper_like_variables(FULL_ARCH, 32)
    v512 = embedded_variables(v32, 512)
    assert len(set(embedded_positions(512) // 16)) == 32 and len(set(embedded_positions(128) // 4)) == 32
    x, y = make_inputs(2, 9, 13, seed=0)
    a = NllGradRef(FULL_ARCH, v32).nll_and_grads(x, y, ISO, CAM)
    b = NllGradRef(FULL_ARCH, v512).nll_and_grads(x, y, ISO, CAM)
    for name, p, q in zip(("nll", "gx", "gy"), a, b):
        d = np.abs(p - q).max() / np.abs(p).max()
        print("%s: width-512 embedding to width-32 source, relative %.2e" % (name, d))
        assert d <= 1e-12, (name, d)
    from noise_flow_amd import _lib
    rc, msg = _supported(FULL_ARCH, v512, 512, (32, 32), _lib.NF_CFG_GRAD_GEMM)
    assert rc == 0, msg


# ---- Python -----------------------------------------------------------------------------------------------------------------
def test_grad_kernel_keyword(monkeypatch):
    """grad_kernel='gemm' sets NF_CFG_GRAD_GEMM in the nf_config handed to nf_create (recorded in front of it: no device is
    opened, the device plumbing is a stub), hps.grad_kernel does the same; with cnn_dtype='fp16' it raises, any other value still
    raises."""
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from noise_flow_amd import noise_flow_model as nfm
    v = _vars(WIDE_ARCH, 64)
    seen = []

    class Recorded(Exception):
        pass

    class StubDev:
        def __init__(self, device=None):
            self.device = type("D", (), {"index": 0})()

    def recording(*a):
        seen.append(int(a[-1]))
        raise Recorded()

    monkeypatch.setattr(nfm, "_Dev", StubDev)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "nf_config", recording)
        for kw, hps_kw in (({"grad_kernel": "gemm"}, {}), ({}, {"grad_kernel": "gemm"}), ({"grad_kernel": "scalar"}, {}), ({"grad_kernel": "mfma"}, {})):
            with pytest.raises(Recorded):
                NoiseFlow([16, 16, 4], False, default_hps(arch=WIDE_ARCH, width=64, **hps_kw), variables=v, **kw)
    assert seen == [_lib.NF_CFG_GRAD_GEMM, _lib.NF_CFG_GRAD_GEMM, 0, _lib.NF_CFG_GRAD_MFMA], seen
    with pytest.raises(ValueError):
        NoiseFlow([16, 16, 4], False, default_hps(arch=WIDE_ARCH, width=64), variables=v, grad_kernel="gemm", cnn_dtype="fp16")
    with pytest.raises(ValueError):
        NoiseFlow([16, 16, 4], False, default_hps(arch=WIDE_ARCH, width=64), variables=v, grad_kernel="tensor")
    assert _lib.NF_CFG_GRAD_GEMM == 64 and _lib.NF_GRAD_PATH_GEMM == 4
