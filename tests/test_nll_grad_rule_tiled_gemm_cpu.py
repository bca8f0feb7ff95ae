"""CPU tier of the rule for the tiled gradient at coupling widths 33 .. 512 (tests/test_gpu_nll_grad_tiled_gemm.py): the tiled
arithmetic of tests/test_nll_grad_rule_tiled_wide_cpu.py (``tiled_sweep``: the forward pass keeps the tensor in front of every
segment; then, last segment first, every min(H,32) x min(W,32) tile is evaluated on its own and only its core window is kept), run
in float64 on the plan ``nf_grad_tile_segments`` returns under NF_CFG_GRAD_TILED_GEMM, is torch.autograd of the whole image — on the
dense width-64 model, on the planner's own plan and with one coupling per segment.  No device is touched.

The mutant: every halo one pixel short (3 instead of 4 per coupling; ``tiled_sweep`` shortens the segments of ONE coupling, the only
ones in which a pixel shows at fp32 resolution).  With one coupling per segment it reaches a core on both cases — the second tile
of the 40-pixel axis starts at 8 and reports from 11 instead of 12, three pixels behind its border — and must exceed TWICE the
combined bound; the measured ratios are printed (run with -s).
"""
import ctypes as C

import numpy as np
import pytest

import nll_grad_ref as R
from conftest import make_inputs
from test_grad_wide_supported_cpu import paper_like_variables
from test_nll_grad_ref_cpu import WIDE_ARCH
from test_nll_grad_rule_cpu import _ratios
from test_nll_grad_rule_tiled_wide_cpu import tiled_sweep

ISO, CAM = 800.0, 2.0
WIDTH = 64
CASES = [((40, 36), 2, 1), ((2, 40), 4, 0)]      # (shape, B, seed): inputs of tests/test_gpu_nll_grad_tiled_gemm.py
_REF = {}


def _ref():
    if not _REF:
        v = paper_like_variables(WIDE_ARCH, WIDTH)
        _REF["v"], _REF["ref"] = v, R.PinnedRef(WIDE_ARCH, v)
    return _REF["v"], _REF["ref"]


def _plan(ref, variables, hw, forced, monkeypatch):
    """[(first layer, one-past-last layer, couplings)] over the reference's layers, from the library's plan under the new flag."""
    from noise_flow_amd import _lib, params
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    if forced:
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    lib = _lib.load()
    layers, descs, flat = params.pack(WIDE_ARCH, variables, WIDTH, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, _lib.NF_CFG_GRAD_TILED_GEMM)
    out = (C.c_int32 * 80)()
    n = lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, out, 16)
    assert n >= 1 and (not forced or n == forced), (n, lib.nf_last_error())
    counts = [out[5 * i + 2] // 4 for i in range(n)]
    assert all(out[5 * i + 2] == 4 * c and 1 <= c <= 3 for i, c in enumerate(counts))
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    assert sum(counts) == len(cpl)
    plan, lo, k = [], 0, 0
    for s, c in enumerate(counts):
        hi = len(ref.layers) if s == len(counts) - 1 else cpl[k + c - 1] + 1
        plan.append((lo, hi, c))
        lo, k = hi, k + c
    return plan


@pytest.mark.parametrize("forced", [None, 3])
@pytest.mark.parametrize("hw,B,seed", CASES)
def test_tiled_sweep_on_the_gemm_plan_is_autograd(monkeypatch, hw, B, seed, forced):
    v, ref = _ref()
    plan = _plan(ref, v, hw, forced, monkeypatch)
    x, y = make_inputs(B, hw[0], hw[1], seed=seed)
    _, gx64, gy64 = ref.nll_and_grads(x, y, ISO, CAM)
    got = tiled_sweep(ref, x, y, ISO, CAM, plan, np.float64)
    for name, r64, g in (("gx", gx64, got[0]), ("gy", gy64, got[1])):
        d = float(R.patch_rel_err(g, r64).max())
        print("%r segments %r %s: tiled fp64 to autograd fp64 %.2e" % (hw, [c for _, _, c in plan], name, d))
        assert d <= 1e-12, (name, d)


def test_halo_one_pixel_short_exceeds_twice_the_bound(monkeypatch):
    v, ref = _ref()
    ratios = {}
    for hw, B, seed in CASES:
        plan = _plan(ref, v, hw, 3, monkeypatch)      # one coupling per segment
        assert [c for _, _, c in plan] == [1, 1, 1]
        x, y = make_inputs(B, hw[0], hw[1], seed=seed)
        _, gx64, gy64 = ref.nll_and_grads(x, y, ISO, CAM)
        bound = R.combined_bound(ref, x, y, ISO, CAM)
        got = tiled_sweep(ref, x, y, ISO, CAM, plan, np.float64, mutant="short_halo")
        got = tuple(None if g is None else np.nan_to_num(g, nan=0.0) for g in got)
        ratio, raw = _ratios(bound, got, (gx64, gy64))
        print("%r short_halo: %9.3g x the combined bound;  the raw norm alone: %9.3g x" % (hw, ratio, raw))
        ratios[hw] = ratio
    assert max(ratios.values()) >= 2.0, ratios
