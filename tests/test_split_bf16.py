"""The split-bf16 kernel of the width-4 model on full 32x32 patches (nf_flow_kernel PREC = 3, NF_PATH_SPLIT_BF16).

l_1 and l_last run as "bf16 x 6" on v_mfma_f32_16x16x32_bf16 (csrc/nf_device.h, NF12_*); everything else is the exact-fp32
kernel's arithmetic.  CPU tests hold the host-side weight split and the layout (emulated lane by lane) to the folded fp32 model;
GPU tests hold the kernel to the fp64 oracle in both directions and to the exact-fp32 kernel (NF_CFG_EXACT_FP32).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables

NF2_CPL_W1T, NF2_CPL_W3T, NF2_CPL_SIZE = 76, 188, 332
NF12_CPL_AOFF, NF12_A_A3 = 92, 1536
PITCH = 34


def _fold_layout(arch, variables, path, flags=0, direction=0):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, 4, "loss_first", 1, "LU")
    cfg = _lib.nf_config(32, 32, 4, len(layers), -1, flags)
    ops = (C.c_int32 * 256)()
    n_ops, lw, nf = C.c_int32(), C.c_int32(), C.c_size_t()
    args = (C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, direction, path, ops, 128, C.byref(n_ops),
            C.byref(lw))
    _lib.check(lib.nf_fold_layout(*args, None, 0, C.byref(nf)))
    folded = np.zeros(nf.value, np.float32)
    _lib.check(lib.nf_fold_layout(*args, folded.ctypes.data_as(C.POINTER(C.c_float)), folded.size, C.byref(nf)))
    return [(ops[2 * i], ops[2 * i + 1]) for i in range(n_ops.value)], folded


def _bf16_pieces(words):
    """uint32 words holding two bf16 each -> float64 [..., 2] (element 0 in the low half)."""
    w = np.asarray(words, np.uint32)
    lo = (w << np.uint32(16)).view(np.float32)
    hi = (w & np.uint32(0xFFFF0000)).view(np.float32)
    return np.stack([lo, hi], -1).astype(np.float64)


def _bf16(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _split3(x):
    x = np.asarray(x, np.float32)
    h = _bf16(x)
    r = (x - h).astype(np.float32)
    m = _bf16(r)
    l_ = _bf16((r - m).astype(np.float32))
    return h.astype(np.float64), m.astype(np.float64), l_.astype(np.float64)


def _couplings(arch="unc|unc", seed=5, direction=0):
    from noise_flow_amd import _lib
    v = trained_like_variables(arch, 4, seed=seed)
    ops9, blk9 = _fold_layout(arch, v, _lib.NF_PATH_SPLIT_BF16, direction=direction)
    ops2, blk2 = _fold_layout(arch, v, _lib.NF_PATH_MFMA4, direction=direction)
    out = []
    for (t9, o9), (t2, o2) in zip(ops9, ops2):
        assert t9 == t2
        if t9 in (2, 3):
            aoff = int(blk9[o9 + NF12_CPL_AOFF:o9 + NF12_CPL_AOFF + 1].view(np.int32)[0])
            out.append((blk9, o9, aoff, blk2[o2:o2 + NF2_CPL_SIZE]))
    assert out
    return out


def test_split_layout_reconstructs_every_folded_weight():
    """Each weight of l_1 / l_last in the A images is the sum of its three bf16 pieces to 2^-24 relative, and the LDS part
    carries the exact-fp32 kernel's tables unchanged."""
    for direction in (0, 1):
        for blk9, o9, aoff, v2 in _couplings(direction=direction):
            np.testing.assert_array_equal(blk9[o9:o9 + 92], np.concatenate([v2[0:76], v2[172:188]]))   # E B1 B2 S, W2t
            words = blk9[aoff:aoff + 3072].view(np.uint32)
            a1 = _bf16_pieces(words[:1536]).reshape(3, 2, 64, 8)         # [pair][half][lane][e]
            a3 = _bf16_pieces(words[NF12_A_A3:]).reshape(3, 2, 64, 8)    # [piece][m3][lane][e]
            W1 = v2[NF2_CPL_W1T:NF2_CPL_W1T + 96].astype(np.float64).reshape(4, 3, 8)   # [j][di][2 dj + c]
            W3 = v2[NF2_CPL_W3T:NF2_CPL_W3T + 144].astype(np.float64).reshape(4, 9, 4)  # [j][tap][c]
            seen1 = seen3 = 0
            for l in range(64):
                gk, m = l >> 4, l & 15
                a, p, j = m >> 3, (m >> 2) & 1, m & 3
                for e in range(8):
                    for half in range(2):
                        wc, ws, c = 2 * half + (e >> 2), (e >> 1) & 1, e & 1
                        di, dj = 2 * (gk & 1) + (gk >> 1) - a, wc - p
                        want = W1[j, di, 2 * dj + c] if 0 <= di <= 2 and 0 <= dj <= 2 else 0.0
                        hh, mm, hl = a1[0, half, l, e], a1[1, half, l, e], a1[2, half, l, e]
                        if ws == 0:
                            assert hl == hh     # (a_h | a_l): the high piece meets z_l
                            got = None
                        else:
                            got = hh + mm + hl  # ... and the low piece meets z_h
                        if got is not None:
                            assert abs(got - want) <= 2.0 ** -24 * abs(want), (l, e, half, got, want)
                            seen1 += want != 0.0
                    for m3 in range(2):
                        wc, c = 2 * (gk >> 1) + (e >> 2), e & 3
                        di, dj = 2 * (gk & 1) + m3 - a, wc - p
                        want = W3[j, di * 3 + dj, c] if 0 <= di <= 2 and 0 <= dj <= 2 else 0.0
                        got = a3[:, m3, l, e].sum()
                        assert abs(got - want) <= 2.0 ** -24 * abs(want), (l, e, m3, got, want)
                        seen3 += want != 0.0
            assert seen1 > 0 and seen3 > 0


def _mfma_16x16x32(A, B):
    """v_mfma_f32_16x16x32: A[lane][e] = A-matrix[m = lane & 15][k = 8 (lane >> 4) + e], B[lane][e] = B-matrix[k][n = lane & 15];
    returns D[lane][v] = D-matrix[4 (lane >> 4) + v][n = lane & 15]."""
    Am = np.zeros((16, 32)); Bm = np.zeros((32, 16))
    for l in range(64):
        Am[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = A[l]
        Bm[8 * (l >> 4):8 * (l >> 4) + 8, l & 15] = B[l]
    D = Am @ Bm
    return np.array([[D[4 * (l >> 4) + v, l & 15] for v in range(4)] for l in range(64)])


def test_split_layout_emulated_lane_by_lane_matches_the_fp32_convolutions():
    """The NF12 block consumed exactly as nf_flow_kernel<.., PREC = 3> consumes it — the three LDS regions filled as the lanes
    publish z0 / relu(h2), the K slots' 16-byte reads, the A operands in lane order, the six products per conv — against l_1 and
    l_last evaluated in fp64 on the fp32 weights.  Catches layout / indexing mistakes without a GPU."""
    blk9, o9, aoff, v2 = _couplings(arch="unc")[0]
    words = blk9[aoff:aoff + 3072].view(np.uint32)
    A1 = _bf16_pieces(words[:1536]).reshape(3, 2, 64, 8)
    A3 = _bf16_pieces(words[NF12_A_A3:]).reshape(3, 2, 64, 8)
    B1 = v2[64:68].astype(np.float64)
    E = v2[0:64].astype(np.float64).reshape(16, 4)
    W1 = v2[NF2_CPL_W1T:NF2_CPL_W1T + 96].astype(np.float64).reshape(4, 3, 8)[:, :, :6].reshape(4, 3, 3, 2)   # [j][di][dj][c]
    W3 = v2[NF2_CPL_W3T:NF2_CPL_W3T + 144].astype(np.float64).reshape(4, 3, 3, 4)                          # [j][di][dj][c]
    rng = np.random.RandomState(7)
    z0 = (rng.randn(32, 32, 2) * np.exp(rng.randn(32, 32, 2))).astype(np.float32)
    h2 = np.maximum(rng.randn(32, 32, 4), 0).astype(np.float32) * 3
    zp = np.zeros((34, 34, 2)); zp[1:33, 1:33] = z0
    hp = np.zeros((34, 34, 4)); hp[1:33, 1:33] = h2
    # regions: [slot][word][2 values]
    R = np.zeros((3, 34 * PITCH, 2, 2))
    zh, zm, zl = _split3(z0)
    hh, hm, hl = _split3(h2)
    for r in range(32):
        s = (r + 1) * PITCH + 1
        R[0, s:s + 32, 0], R[0, s:s + 32, 1] = zh[r], zm[r]
        R[1, s:s + 32, 0], R[1, s:s + 32, 1] = zl[r], zh[r]
    Rh = np.zeros((3, 34 * PITCH, 4))
    for r in range(32):
        s = (r + 1) * PITCH + 1
        Rh[0, s:s + 32], Rh[1, s:s + 32], Rh[2, s:s + 32] = hh[r], hm[r], hl[r]
    ref1 = np.zeros((32, 32, 4)); ref3 = np.zeros((32, 32, 4)); mag1 = np.zeros((32, 32, 4)); mag3 = np.zeros((32, 32, 4))
    for r in range(32):
        for c in range(32):
            w1 = zp[r:r + 3, c:c + 3]
            ref1[r, c] = B1 + np.einsum("jabc,abc->j", W1, w1)
            mag1[r, c] = np.abs(B1) + np.einsum("jabc,abc->j", np.abs(W1), np.abs(w1))
            bm = (r == 0) | (r == 31) << 1 | (c == 0) << 2 | (c == 31) << 3
            w3 = hp[r:r + 3, c:c + 3]
            ref3[r, c] = E[bm] + np.einsum("jabc,abc->j", W3, w3)
            mag3[r, c] = np.abs(E[bm]) + np.einsum("jabc,abc->j", np.abs(W3), np.abs(w3))
    got1 = np.zeros((32, 32, 4)); got3 = np.zeros((32, 32, 4))
    lanes = np.arange(64)
    u = ((lanes & 15) + 12) & 15
    g, n = lanes >> 4, np.where(u < 8, 2 * u, 2 * (u - 8) + 1)   # nf12_col: the column pair of a lane column
    assert sorted(n[:16]) == list(range(16))
    for wv in range(4):
        for k in range(4):
            acc1 = np.tile(B1, (64, 1))
            for pair, half in [(2, 0), (2, 1), (1, 0), (1, 1), (0, 0), (0, 1)]:
                base = (8 * wv + 2 * k + 2 * (g & 1) + (g >> 1)) * PITCH + 2 * n + 2 * half
                reg = R[1 if pair == 2 else 0]
                Bop = np.concatenate([reg[base].reshape(64, 4), reg[base + 1].reshape(64, 4)], 1)   # slot, word, channel
                acc1 = acc1 + _mfma_16x16x32(A1[pair, half], Bop)
            rows = 8 * wv + 2 * k + (g >> 1)
            cols = 2 * n + (g & 1)
            bms = (rows == 0) | (rows == 31) << 1 | (cols == 0) << 2 | (cols == 31) << 3
            acc3 = E[bms].copy()
            for pa, pb in [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]:
                for m3 in range(2):
                    base = (8 * wv + 2 * k + 2 * (g & 1) + m3) * PITCH + 2 * n + 2 * (g >> 1)
                    Bop = np.concatenate([Rh[pb, base], Rh[pb, base + 1]], 1)
                    acc3 = acc3 + _mfma_16x16x32(A3[pa, m3], Bop)
            got1[rows, cols] = acc1
            got3[rows, cols] = acc3
    assert np.all(np.abs(got1 - ref1) <= 2.0 ** -22 * mag1 + 1e-30)
    assert np.all(np.abs(got3 - ref3) <= 2.0 ** -22 * mag3 + 1e-30)


def test_exact_fp32_flag_and_other_shapes_have_no_split_block():
    from noise_flow_amd import _lib
    v = trained_like_variables("unc", 4, seed=2)
    with pytest.raises(RuntimeError):
        _fold_layout("unc", v, _lib.NF_PATH_SPLIT_BF16, flags=_lib.NF_CFG_EXACT_FP32)
    with pytest.raises(RuntimeError):
        _fold_layout("unc", v, _lib.NF_PATH_SPLIT_BF16, flags=_lib.NF_CFG_FP16_CNN)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _model(variables, cnn_dtype="fp32", arch=FULL_ARCH):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([32, 32, 4], False, default_hps(arch=arch, width=4), variables=variables, cnn_dtype=cnn_dtype)


def _path(m, direction):
    return m._flow.lib.nf_kernel_path(m._flow.ptr, direction)


@pytest.mark.gpu
def test_split_kernel_is_the_default_and_the_flag_keeps_the_exact_one(shipped_variables):
    from noise_flow_amd import _lib
    m = _model(shipped_variables)
    assert _path(m, 0) == _lib.NF_PATH_SPLIT_BF16 and _path(m, 1) == _lib.NF_PATH_SPLIT_BF16
    e = _model(shipped_variables, "fp32_exact")
    assert _path(e, 0) == _lib.NF_PATH_MFMA4 and _path(e, 1) == _lib.NF_PATH_MFMA4


@pytest.mark.gpu
@pytest.mark.parametrize("iso,cam,b1", [(100, 2, 0.000479), (1600, 4, 0.005)])
def test_split_kernel_against_the_oracle_both_directions(shipped_variables, oracle_full, iso, cam, b1):
    from conftest import close_elem
    x, y = make_inputs(16, seed=iso + 7, b1=b1)
    m = _model(shipped_variables)
    nll, sd_z = m._loss(x, y, [0.0], [0.0], [iso], [cam])
    ref_nll, ref_sd, _ = oracle_full.nll(x, y, iso, cam)
    np.testing.assert_allclose(nll, ref_nll, rtol=1e-5)
    assert abs(sd_z - ref_sd) <= 1e-5 * ref_sd
    z, obj = m.inverse(x, None, y, [0.0], [0.0], [iso], [cam])
    ref_z, ref_obj = oracle_full.inverse(x, y, iso, cam)
    close_elem(z, ref_z, 1e-5)
    np.testing.assert_allclose(obj, ref_obj, rtol=1e-5)
    eps = np.random.RandomState(iso).randn(*x.shape).astype(np.float32)
    for temp in (1.0, 0.6):
        xs = m.sample(y, temp, y, [0.0], [0.0], [iso], [cam], eps=eps)
        close_elem(xs, oracle_full.sample(eps, temp, y, iso, cam), 1e-5)


@pytest.mark.gpu
def test_split_kernel_against_the_exact_fp32_kernel_on_the_golden_inputs(shipped_variables):
    import os
    from conftest import GOLDEN_DIR
    g = np.load(os.path.join(GOLDEN_DIR, "full_arch_shipped.npz"))
    y = g["y"]
    a, b = _model(shipped_variables), _model(shipped_variables, "fp32_exact")
    for iso, cam in ((100, 2), (800, 2), (3200, 1)):
        x = g["x_iso%d_cam%d" % (iso, cam)]
        na, sa = a._loss(x, y, [0], [0], [iso], [cam])
        nb, sb = b._loss(x, y, [0], [0], [iso], [cam])
        np.testing.assert_allclose(na, nb, rtol=1e-6)
        assert abs(sa - sb) <= 1e-6 * sb
        za, _ = a.inverse(x, None, y, [0], [0], [iso], [cam])
        zb, _ = b.inverse(x, None, y, [0], [0], [iso], [cam])
        assert np.abs(za - zb).max() <= 1e-5 * np.abs(zb).max()
    xa = a.sample(y, 1.0, y, [0], [0], [100], [2], eps=g["eps"])
    xb = b.sample(y, 1.0, y, [0], [0], [100], [2], eps=g["eps"])
    assert np.abs(xa - xb).max() <= 1e-5 * np.abs(xb).max()
