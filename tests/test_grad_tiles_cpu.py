"""CPU tier of the tiled input gradients (NF_CFG_GRAD_TILED, csrc/nf_grad.hip TILED): what ``nf_grad_supported`` accepts and refuses
with the flag, the plan ``nf_grad_tile_segments`` reports, and the arithmetic the design rests on — the gradient of a tile
evaluated alone is exact 4 x (couplings) pixels inside every tile border that is not an image border, and one pixel less is not —
pinned in fp64 with ``PinnedRef`` and the tile arithmetic of ``nf_tile_plan``.  No device is touched.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables
from nll_grad_ref import PinnedRef
from test_cond_rows_cpu import cond_variables
from test_nll_grad_ref_cpu import WIDE_ARCH, _supported

VOCAB_ARCH = "sdn5|unc|gain|unc|sdn3"
NO_SDN_ARCH = "unc|gain4|unc"
TILE = 32           # csrc/nf_device.h, NF_GRAD_TILE
CPL = (2, 3)        # NF_OP_COUPLING_FWD / _REV

_VARS = {}


def _vars(arch, width):
    if (arch, width) not in _VARS:
        _VARS[(arch, width)] = cond_variables(arch, width, seed=5) if arch == VOCAB_ARCH else trained_like_variables(arch, width)
    return _VARS[(arch, width)]


def _flag():
    from noise_flow_amd import _lib
    return _lib.NF_CFG_GRAD_TILED


# ---- nf_grad_supported ------------------------------------------------------------------------------------------------------
def test_flag_value_leaves_bit_8_unassigned():
    assert _flag() == 16


@pytest.mark.parametrize("arch,width,hw", [(FULL_ARCH, 4, (96, 80)), (FULL_ARCH, 4, (4096, 4096)), (WIDE_ARCH, 8, (64, 64)),
                                           (WIDE_ARCH, 16, (64, 64)), (WIDE_ARCH, 16, (40, 33)), (FULL_ARCH, 4, (65, 65)),
                                           (WIDE_ARCH, 4, (70, 20)), (VOCAB_ARCH, 4, (70, 36)), (NO_SDN_ARCH, 4, (66, 12))])
def test_supported_with_the_flag_and_refused_without(arch, width, hw):
    from noise_flow_amd import _lib
    rc, msg = _supported(arch, _vars(arch, width), width, hw, _flag())
    assert rc == 0, msg
    rc, msg = _supported(arch, _vars(arch, width), width, hw, _flag() | _lib.NF_CFG_EXACT_FP32 | _lib.NF_CFG_GRAD_MFMA)   # neither matters here
    assert rc == 0, msg
    rc, msg = _supported(arch, _vars(arch, width), width, hw, 0)
    assert rc == _lib.NF_EINVAL and msg, (rc, msg)


@pytest.mark.parametrize("width,hw,extra,word", [(4, (96, 80), "fp16", "fp32"),
                                                 (64, (96, 80), 0, "width"),
                                                 (64, (16, 16), 0, "width"),
                                                 (32, (64, 64), 0, "width 32"),
                                                 (32, (64, 64), "mfma", "32x32"),
                                                 (32, (96, 80), 0, "no tile mode"),
                                                 (32, (96, 80), "mfma", "no tile mode"),
                                                 (4, (4097, 32), 0, "4096"),
                                                 (4, (32, 4097), 0, "4096")])
def test_refusals_with_the_flag(width, hw, extra, word):
    from noise_flow_amd import _lib
    flags = _flag() | {"fp16": _lib.NF_CFG_FP16_CNN, "mfma": _lib.NF_CFG_GRAD_MFMA, 0: 0}[extra]
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, flags)
    assert rc == _lib.NF_EINVAL
    assert msg and word in msg, msg


def test_flags_0_and_8_behave_as_before():
    """Today's refusal texts at flags = 0 (tests/test_nll_grad_ref_cpu.py pins the words), and bit 8 stays unknown."""
    from noise_flow_amd import _lib
    for width, hw, word in ((4, (65, 65), "patches of up to 64x64 (65x65 given; no tiled evaluation)"), (16, (64, 64), "width 16"),
                            (8, (64, 64), "LDS"), (32, (32, 32), "LDS")):
        rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, 0)
        assert rc == _lib.NF_EINVAL and word in msg, msg
    for hw in ((16, 16), (96, 80)):
        for flags in (8, 8 | _flag()):
            rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 8), 8, hw, flags)
            assert rc == _lib.NF_EINVAL and "unknown bits" in msg, msg


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def _plan(arch, width, hw, flags=None):
    """(return code of nf_grad_tile_segments, its rows, the op types of the NLL-order program)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, _vars(arch, width), width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, _flag() if flags is None else flags)
    fp = flat.ctypes.data_as(C.POINTER(C.c_float))
    out = (C.c_int32 * 80)()
    n = lib.nf_grad_tile_segments(C.byref(cfg), descs, fp, flat.size, out, 16)
    ops = (C.c_int32 * 128)()
    n_ops = C.c_int32()
    cfg0 = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, 0)
    assert lib.nf_fold_params(C.byref(cfg0), descs, fp, flat.size, 0, ops, 64, C.byref(n_ops), None, 0, None, None) == 0
    return n, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))], [ops[2 * i] for i in range(n_ops.value)]


def _axis(size, halo):
    """nf_tile_plan of one axis → (n, origin, core0, core1)."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    o, a, b = ((C.c_int32 * 512)() for _ in range(3))
    n = lib.nf_tile_plan(size, min(size, TILE), halo, o, a, b, 512)
    assert 0 < n <= 512, (size, halo, n)
    return n, list(o[:n]), list(a[:n]), list(b[:n])


# (arch, width, (H, W), forced S or None, expected couplings per segment or None); unforced, the cost model has one coupling per
# segment ahead on the shipped model
PLAN_ROWS = [(FULL_ARCH, 4, (96, 80), None, [1] * 8), (FULL_ARCH, 4, (96, 80), 8, [1] * 8), (FULL_ARCH, 4, (96, 80), 4, [2] * 4),
             (FULL_ARCH, 4, (96, 80), 3, [3, 3, 2]), (FULL_ARCH, 4, (65, 64), None, None), (FULL_ARCH, 4, (1000, 33), None, None),
             (WIDE_ARCH, 8, (64, 64), None, None), (WIDE_ARCH, 8, (64, 64), 1, [3]), (WIDE_ARCH, 8, (64, 64), 2, [2, 1]),
             (WIDE_ARCH, 16, (64, 64), 3, [1, 1, 1]), (WIDE_ARCH, 16, (40, 33), None, None), (WIDE_ARCH, 4, (70, 20), None, None),
             (VOCAB_ARCH, 4, (70, 36), None, None), (NO_SDN_ARCH, 4, (66, 12), None, None), (FULL_ARCH, 4, (4096, 4096), None, [1] * 8)]


@pytest.mark.parametrize("arch,width,hw,forced,want", PLAN_ROWS)
def test_plan_properties(monkeypatch, arch, width, hw, forced, want):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    if forced:
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    n, segs, types = _plan(arch, width, hw)
    n_cpl = sum(1 for t in types if t in CPL)
    assert 1 <= n <= 16 and (not forced or n == forced), (n, segs)
    assert segs[0][0] == 0 and segs[-1][1] == len(types)                       # cover all ops
    got = []
    for i, (op0, op1, halo, ny, nx) in enumerate(segs):
        c = sum(1 for t in types[op0:op1] if t in CPL)
        got.append(c)
        assert i == 0 or op0 == segs[i - 1][1]                                 # contiguous
        assert i == n - 1 or types[op1 - 1] in CPL                             # ends after a coupling
        assert halo == 4 * c and TILE - 2 * halo >= 8
        for size, cnt in ((hw[0], ny), (hw[1], nx)):
            m, org, c0, c1 = _axis(size, halo)
            assert cnt == m                                                     # tile counts are nf_tile_plan's
            assert c0[0] == 0 and c1[-1] == size and all(c1[k] == c0[k + 1] for k in range(m - 1))   # cores partition the axis
            assert all(c0[k] < c1[k] for k in range(m))
            t = min(size, TILE)
            for k in range(m):                                                  # >= halo from every tile border that is not the image's
                assert 0 <= org[k] and org[k] + t <= size
                assert org[k] == 0 or c0[k] >= org[k] + halo
                assert org[k] + t == size or c1[k] <= org[k] + t - halo
    assert sum(got) == n_cpl and max(got) - min(got) <= 1 and got == sorted(got, reverse=True)   # dealt as evenly as possible
    if want:
        assert got == want


def test_plan_is_zero_for_shapes_held_whole(monkeypatch):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    for arch, width, hw in ((FULL_ARCH, 4, (32, 32)), (FULL_ARCH, 4, (64, 64)), (WIDE_ARCH, 4, (64, 64)), (WIDE_ARCH, 16, (32, 32)),
                            (WIDE_ARCH, 8, (48, 48)), (WIDE_ARCH, 32, (16, 16))):
        assert _plan(arch, width, hw)[0] == 0, (arch, width, hw)
    assert _plan(FULL_ARCH, 4, (64, 64), flags=0)[0] == 0
    from noise_flow_amd import _lib
    assert _plan(FULL_ARCH, 4, (96, 80), flags=0)[0] == _lib.NF_EINVAL        # refused as nf_grad_supported refuses it


def test_infeasible_forced_count_fails(monkeypatch):
    """4 couplings in one segment would need a halo of 16: no core left in a 32-pixel tile."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    for forced in ("2", "1"):
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", forced)
        assert _plan(FULL_ARCH, 4, (96, 80))[0] == _lib.NF_EINVAL
        assert b"segments" in lib.nf_last_error()
        rc, msg = _supported(FULL_ARCH, _vars(FULL_ARCH, 4), 4, (96, 80), _flag())
        assert rc == _lib.NF_EINVAL and "segments" in msg
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "3")
    assert _plan(FULL_ARCH, 4, (96, 80))[0] == 3
    monkeypatch.setenv("NF_TILE_SEGMENTS", "2")                                # the forward direction's switch is another one
    assert _plan(FULL_ARCH, 4, (96, 80))[0] == 3


# ---- the halo, in fp64 ----------------------------------------------------------------------------------------------------------
def _tiled_gradients(ref, x, y, halo, tile):
    """Every tile's gradient computed alone (zero padding and edge channel at ITS border), only its core kept."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    _, H, W, _ = x.shape
    plans = []
    for size in (H, W):
        o, a, b = ((C.c_int32 * 64)() for _ in range(3))
        n = lib.nf_tile_plan(size, min(size, tile), halo, o, a, b, 64)
        assert 0 < n <= 64
        plans.append((list(o[:n]), list(a[:n]), list(b[:n])))
    gx, gy = np.full(x.shape, np.nan), np.full(y.shape, np.nan)
    th, tw = min(H, tile), min(W, tile)
    for oy, ay, by in zip(*plans[0]):
        for ox, ax, bx in zip(*plans[1]):
            _, tx, ty = ref.nll_and_grads(x[:, oy:oy + th, ox:ox + tw], y[:, oy:oy + th, ox:ox + tw], 800.0, 2.0)
            gx[:, ay:by, ax:bx] = tx[:, ay - oy:by - oy, ax - ox:bx - ox]
            gy[:, ay:by, ax:bx] = ty[:, ay - oy:by - oy, ax - ox:bx - ox]
    return gx, gy


@pytest.mark.parametrize("arch,c", [("sdn5|unc", 1), ("sdn5|unc|unc", 2), (WIDE_ARCH, 3)])
def test_gradient_halo_is_four_per_coupling_in_fp64(arch, c):
    """d nll / d z_in at p sums over q within 2c of p, each Jacobian entry at q depends on z_in within 2c of q: with a halo of 4c
    the tiled gradient IS the whole image's (<= 1e-13 of max|grad|; measured 0), with 4c - 1 it is not (> 1e-12; measured, gx /
    gy: 1 coupling 1.6e-3 / 2.5e-5, 2 couplings 1.9e-6 / 4.0e-8, 3 couplings 1.3e-10 / 1.1e-12 — gy of the deepest case sits AT the
    bound, so gx carries it).  90x70 image, 64-pixel tiles, trained_like_variables(arch, 4, seed=1)."""
    ref = PinnedRef(arch, trained_like_variables(arch, 4, seed=1))
    x, y = make_inputs(1, 90, 70, seed=0)
    x, y = x.astype(np.float64), y.astype(np.float64)
    _, gx, gy = ref.nll_and_grads(x, y, 800.0, 2.0)
    err = {}
    for halo in (4 * c, 4 * c - 1):
        tx, ty = _tiled_gradients(ref, x, y, halo, 64)
        err[halo] = (np.abs(tx - gx).max() / np.abs(gx).max(), np.abs(ty - gy).max() / np.abs(gy).max())
        print("couplings %d halo %2d: gx %.2e gy %.2e" % (c, halo, err[halo][0], err[halo][1]))
    assert max(err[4 * c]) <= 1e-13
    assert err[4 * c - 1][0] > 1e-12
