"""The parameter image of the matrix-core gradient kernel (csrc/nf_device.h, NFGW_*; built by relayout_coupling_grad_wide in
csrc/nf_host.hip) against the folded model, without a GPU: ``nf_grad_fold`` returns the block ``nf_create`` uploads; every image is
un-permuted by the fetch-order formulas of the header comment and compared, bit for bit, with the generic block of
``nf_fold_params`` — forward chain (the NF4_IMG_* order without the 2 log2(e) factor) and the three transposed products.  The
1x1 matrices carry their inverse, the scales their reciprocal, as in the scalar gradient block.
"""
import ctypes as C

import numpy as np
import pytest

from test_fold_layout_digests_cpu import model

NF_OP_MIX, NF_OP_COUPLING_FWD, NF_OP_SCALE = 1, 2, 6
FWD, BWD, SIZE = 68, 68 + 3008, 68 + 3008 + 3456
A1, B1, A2, B2, A3, A3C = 0, 768, 800, 1824, 1856, 2880
A3T, A2T, A1T, A1TC = 0, 1280, 2304, 3328
TAP_OF = ((0, 6), (2, 8), (1, 7), (3, 5))   # taps of the P row groups by (a, g')


def chan(v, g):
    return 8 * (v >> 2) + 4 * g + (v & 3)


def _fold(width, hw, flags):
    """((path, ops, block) of nf_grad_fold, (ops, block) of nf_fold_params in the NLL direction)."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    descs, flat = model("sdn5|unc|gain4|unc|gain|unc", 1, "LU", width)
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(descs), -1, flags)
    fptr = flat.ctypes.data_as(C.POINTER(C.c_float))
    ops = (C.c_int32 * 256)()
    n_ops, nf, path, ld = C.c_int32(), C.c_size_t(), C.c_int32(), C.c_double()
    head = (C.byref(cfg), descs, fptr, flat.size, C.byref(path), ops, 128, C.byref(n_ops))
    rc = lib.nf_grad_fold(*head, None, 0, C.byref(nf))
    if rc != 0:
        return rc, None
    blk = np.empty(nf.value, np.float32)
    assert lib.nf_grad_fold(*head, blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(nf)) == 0
    grad = (path.value, [(ops[2 * i], ops[2 * i + 1]) for i in range(n_ops.value)], blk)
    head = (C.byref(cfg), descs, fptr, flat.size, 0, ops, 128, C.byref(n_ops))
    assert lib.nf_fold_params(*head, None, 0, C.byref(nf), C.byref(ld)) == 0
    gen = np.empty(nf.value, np.float32)
    assert lib.nf_fold_params(*head, gen.ctypes.data_as(C.POINTER(C.c_float)), gen.size, C.byref(nf), C.byref(ld)) == 0
    return grad, ([(ops[2 * i], ops[2 * i + 1]) for i in range(n_ops.value)], gen)


def _generic(v1, w=32):
    o = 64
    W3 = v1[o:o + 36 * w].reshape(9, w, 4); o += 36 * w
    W1 = v1[o:o + 18 * w].reshape(9, 2, w); o += 18 * w
    b1 = v1[o:o + w]; o += w
    W2 = v1[o:o + w * w].reshape(w, w); o += w * w
    b2 = v1[o:o + w]; o += w
    return v1[:64], W3, W1, b1, W2, b2, v1[o]


@pytest.mark.parametrize("width", [32, 24])
def test_wide_gradient_block_unpermutes_to_the_folded_model(width):
    from noise_flow_amd import _lib
    (path, gops, blk), (fops, gen) = _fold(width, (32, 32), _lib.NF_CFG_GRAD_MFMA)
    assert path == _lib.NF_GRAD_PATH_WIDE32
    assert [t for t, _ in gops] == [t for t, _ in fops]
    n_cpl = 0
    for (t, off), (_, foff) in zip(gops, fops):
        if t == NF_OP_MIX:
            A, Ai = blk[off:off + 16].reshape(4, 4).astype(np.float64), blk[off + 16:off + 32].reshape(4, 4).astype(np.float64)
            assert np.array_equal(blk[off:off + 16], gen[foff:foff + 16])
            assert np.abs(A @ Ai - np.eye(4)).max() < 1e-5
        elif t == NF_OP_SCALE:
            assert blk[off] == gen[foff] and abs(float(blk[off]) * float(blk[off + 1]) - 1.0) < 1e-6
        elif t == NF_OP_COUPLING_FWD:
            n_cpl += 1
            img = blk[off:off + SIZE]
            E, W3, W1, b1, W2, b2, sc = _generic(gen[foff:])
            assert np.array_equal(img[:64], E) and img[64] == sc and not img[65:68].any()
            f, b = img[FWD:BWD], img[BWD:]
            at = lambda base, s, l: (base + ((s >> 2) * 64 + l) * 4 + (s & 3))   # noqa: E731
            for l in range(64):
                g, i = l >> 5, l & 31
                a, gp, j = i >> 3, (i >> 2) & 1, i & 3
                for s in range(12):   # l_1: step = tap, K slice = input channel
                    assert f[at(A1, s, l)] == (W1[s, g, i] if s < 9 else 0.0)
                for s in range(20):   # l_last^T: step = (tap, element pair), K slice = element of the pair
                    assert b[at(A3T, s, l)] == (W3[s >> 1, i, 2 * (s & 1) + g] if s < 18 else 0.0)
                for s in range(16):
                    c = chan(s, g)
                    assert f[at(A2, s, l)] == W2[c, i] and b[at(A2T, s, l)] == W2[i, c]
                    assert f[at(A3, s, l)] == W3[TAP_OF[a][gp], c, j]
                    assert b[at(A1T, s, l)] == (W1[8 - TAP_OF[a][gp], j, c] if j < 2 else 0.0)
            for g in range(2):
                for v in range(16):
                    assert f[B1 + g * 16 + v] == b1[chan(v, g)] and f[B2 + g * 16 + v] == b2[chan(v, g)]
                for s in range(16):
                    for j in range(4):
                        k = ((s >> 2) * 8 + g * 4 + j) * 4 + (s & 3)
                        assert f[A3C + k] == W3[4, chan(s, g), j]
                        assert b[A1TC + k] == (W1[4, j, chan(s, g)] if j < 2 else 0.0)
    assert n_cpl == 3


def test_grad_fold_without_the_flag_is_the_scalar_block():
    """flags = 0 (and any padded width <= 16 with the flag): couplings stay in the generic layout."""
    from noise_flow_amd import _lib
    for width, hw, flags in ((32, (16, 16), 0), (8, (16, 16), _lib.NF_CFG_GRAD_MFMA)):
        (path, gops, blk), (fops, gen) = _fold(width, hw, flags)
        assert path == _lib.NF_GRAD_PATH_SCALAR
        wp = 32 if width == 32 else 8
        size = 64 + 36 * wp + 18 * wp + 2 * wp + wp * wp + 4
        for (t, off), (_, foff) in zip(gops, fops):
            if t == NF_OP_COUPLING_FWD:
                assert np.array_equal(blk[off:off + size], gen[foff:foff + size])
    rc, _ = _fold(32, (32, 32), 0)
    assert rc == _lib.NF_EINVAL
