"""nf_nll_grad on the matrix-core gradient kernel (NF_CFG_GRAD_MFMA, csrc/nf_grad_wide.hip): coupling widths 17 .. 32, patches
up to 32x32, from the kernel up to torch.autograd.

Comparison rule: that of tests/test_gpu_nll_grad.py (nll_grad_ref.compare_with_kink_rule, max_on_kink = 6): per patch
and tensor  max|kernel - ref64| <= max(1e-5, 4 e32) max|ref64|,  at most 3 of a failing patch's on-kink gates inverted — and the same
once more in the whitened norm of tests/nll_grad_ref.py, which coincides with the raw one on paper_like_variables (flat sdn scale)
and differs on test_full_depth_with_the_shipped_sdn_range (max / median |gy| 1761).  Beyond
it every case asserts FROM THE REFERENCE ALONE, before the kernel's output is looked at, that e32 <= 5e-6 for every patch and
tensor, so the tolerance is never inflated (e32 here: the float32 helper on the float64 helper's gates, nll_grad_ref.PinnedRef); nll_out is
held to the oracle at NLL_RTOL = 1e-5.  Every case asserts that the handle
launches NF_GRAD_PATH_WIDE32.  Models of the deep cases: paper_like_variables (tests/test_grad_wide_supported_cpu.py).

The 24x24 case also runs the unchanged scalar kernel (a handle without the flag) on the same model and inputs and prints its
distances: it meets the rule there (figures in that test's docstring), so the rule above is the bound for the 8-coupling cases too.
Measured distances are printed (run with -s).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs
from nll_grad_ref import PinnedRef, compare_with_kink_rule, reference_conditions
from test_cond_rows_cpu import cond_variables
from test_grad_wide_supported_cpu import NO_SDN_ARCH, paper_like_variables
from test_gpu_nll_grad import ISO, CAM, NLL_RTOL, TUPLES5, VOCAB_ARCH, WIDE_ARCH, _bits, _call, _cond, _dev

pytestmark = pytest.mark.gpu

_REFS = {}


def _model(arch, width, variables=None, **hps):
    """(variables, reference) of a test model, built once."""
    key = (arch, width, tuple(sorted(hps.items())), id(variables) if variables is not None else 0)
    if key not in _REFS:
        v = variables if variables is not None else paper_like_variables(arch, width)
        _REFS[key] = (v, PinnedRef(arch, v, flow_permutation=hps.get("flow_permutation", 1), decomp=hps.get("decomp", "LU")))
    return _REFS[key]


def _flow(arch, variables, hw, width, grad_kernel="mfma", cnn_dtype="fp32", **hps):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, cnn_dtype=cnn_dtype,
                     grad_kernel=grad_kernel)


def _path(m):
    return m._flow.lib.nf_grad_path(m._flow.ptr)


def _check(m, ref, width, x, y, iso, cam, rows=None, wide=True, min_gy_range=None):
    """One launch against the reference: the conditions from the reference alone, then the comparison and kink rules."""
    from noise_flow_amd import _lib
    reference_conditions(ref, width, x, y, iso, cam, min_gy_range=min_gy_range)
    assert _path(m) == (_lib.NF_GRAD_PATH_WIDE32 if wide else _lib.NF_GRAD_PATH_SCALAR)
    xd, yd = _dev(x), (_dev(y) if y is not None else None)
    rc, nll, gx, gy = _call(m, xd, yd, cond=None if rows is not None else (_cond(iso, cam) if iso is not None else _cond()), rows=rows)
    _lib.check(rc)
    nll64, dist = compare_with_kink_rule(ref, width, x, y, iso, cam, gx.cpu().numpy(), gy.cpu().numpy() if gy is not None else None, log=print)
    want = ref.oracle_nll(x, y, iso, cam)
    assert np.all(np.abs(nll64 - want) <= 1e-12 * np.abs(want)), (nll64, want)
    got = nll.cpu().numpy().astype(np.float64)
    print("nll: kernel-to-oracle %s" % " ".join("%.2e" % v for v in np.abs(got - want) / np.abs(want)))
    assert np.all(np.abs(got - want) <= NLL_RTOL * np.abs(want))
    return dist


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------
def _inputs_32x32_w32():
    """The two named 32x32 patches at width 32 (most full patches there have 7 .. 17 on-kink activations of 524 288)."""
    x1, y1 = make_inputs(2, 32, 32, seed=1)
    x3, y3 = make_inputs(2, 32, 32, seed=3)
    return np.stack([x1[0], x3[1]]), np.stack([y1[0], y3[1]])


FULL_DEPTH_CASES = [(17, (32, 32), 3, 1), (32, (32, 32), 0, 0), (32, (30, 27), 2, 0), (32, (17, 31), 3, 0),
                    (32, (9, 32), 3, 0), (32, (7, 32), 3, 0), (32, (32, 5), 3, 0), (32, (8, 8), 3, 0),
                    (32, (1, 32), 3, 0), (32, (32, 1), 3, 0), (32, (1, 1), 3, 0)]
SCALED_CASES = [(WIDE_ARCH, 32, (32, 32)), (WIDE_ARCH, 32, (31, 29)), (WIDE_ARCH, 24, (32, 32)), (NO_SDN_ARCH, 32, (32, 32))]


@pytest.mark.parametrize("width,hw,B,seed", FULL_DEPTH_CASES)
def test_full_depth(width, hw, B, seed):
    v, ref = _model(FULL_ARCH, width)
    x, y = _inputs_32x32_w32() if B == 0 else make_inputs(B, hw[0], hw[1], seed=seed)
    _check(_flow(FULL_ARCH, v, hw, width), ref, width, x, y, ISO, CAM)


def shipped_sdn_variables(shipped_variables, width=32):
    """paper_like_variables(FULL_ARCH, width) with the shipped checkpoint's model/sdn_gain/* values: the deep model with the
    shipped sdn layer's three decades of dynamic range in gx and gy (paper_like_variables alone: max / median |gy| = 3)."""
    v = paper_like_variables(FULL_ARCH, width)
    v.update({k: a for k, a in shipped_variables.items() if k.startswith("model/sdn_gain/")})
    return v


def inputs_32x32_shipped_sdn():
    """Two named 32x32 patches with 4 on-kink activations each on that model (of the 48 patches of seeds 0 .. 11, 11 have at most 6)."""
    x0, y0 = make_inputs(4, 32, 32, seed=0)
    x7, y7 = make_inputs(4, 32, 32, seed=7)
    return np.stack([x0[0], x7[2]]), np.stack([y0[0], y7[2]])


def test_full_depth_with_the_shipped_sdn_range(shipped_variables):
    """The whitened norm's case of this file: max / median |gy| >= 100, asserted from the reference (1761; on-kink [4, 4], pinned e32
    at most 2.7e-6).  Measured on an MI355X, raw / whitened: gx 1.8e-6 / 1.4e-6, gy 1.8e-6 / 1.5e-6."""
    from test_gpu_nll_grad import GY_RANGE
    v, ref = _model(FULL_ARCH, 32, shipped_sdn_variables(shipped_variables))
    x, y = inputs_32x32_shipped_sdn()
    _check(_flow(FULL_ARCH, v, (32, 32), 32), ref, 32, x, y, ISO, CAM, min_gy_range=GY_RANGE)


def test_full_depth_24x24_beside_the_scalar_kernel():
    """The largest 8-coupling shape both kernels hold: the new kernel under the rule, and the distances of the unchanged scalar
    kernel (a handle without the flag) on the same model and inputs, under the same rule.  Measured on an MI355X: the scalar
    kernel 2.1e-6 / 2.0e-6 (gx) and 1.2e-6 / 1.9e-6 (gy) of max|grad|, inside max(1e-5, 4 e32) — so the rule stands as it is for the
    8-coupling cases; the matrix-core kernel 1.2e-6 / 1.1e-6 and 9.7e-7 / 8.5e-7."""
    v, ref = _model(FULL_ARCH, 32)
    x, y = make_inputs(2, 24, 24, seed=0)
    _check(_flow(FULL_ARCH, v, (24, 24), 32), ref, 32, x, y, ISO, CAM)
    print("the scalar kernel on the same case:")
    _check(_flow(FULL_ARCH, v, (24, 24), 32, grad_kernel="scalar"), ref, 32, x, y, ISO, CAM, wide=False)


@pytest.mark.parametrize("arch,width,hw", SCALED_CASES)
def test_scaled_models(arch, width, hw):
    v, ref = _model(arch, width)
    x, y = make_inputs(3, hw[0], hw[1], seed=0)
    if arch == NO_SDN_ARCH:
        _check(_flow(arch, v, hw, width), ref, width, x, None, None, None)
    else:
        _check(_flow(arch, v, hw, width), ref, width, x, y, ISO, CAM)


# ---- 2. vocabulary and conditioning on the new path ------------------------------------------------------------------------------
VW = 32


def _vocab_variables(decomp="LU"):
    """tests/test_gpu_nll_grad.py::_vocab_variables at width 32 (2 couplings: at most 1 on-kink activation per patch and
    e32 <= 2.3e-6 on the inputs below, without any rescaling)."""
    from oracle import nf_oracle as O
    v = cond_variables(VOCAB_ARCH, VW, seed=5)
    for k in v:
        if k == "model/g1":
            v[k] = (v[k] - 6.0).astype(np.float32)
        elif "gain_param_" in k:
            v[k] = (v[k] - 30.0).astype(np.float32)
    if decomp == "NONE":   # the same matrices, as the variable itself
        for lyr, i in O.parse_arch(VOCAB_ARCH):
            if lyr == "unc":
                A = O.conv1x1_from_variables(v, i, "LU", np.float64)[0]
                for name in O.conv1x1_variable_names(i, "LU").values():
                    del v[name]
                v[O.conv1x1_variable_names(i, "NONE")["A"]] = A.astype(np.float32)
    return v


_VOCAB = {}


def _vocab(decomp="LU"):
    if decomp not in _VOCAB:
        _VOCAB[decomp] = _vocab_variables(decomp)
    return _VOCAB[decomp]


def test_vocabulary_per_call_cond():
    v, ref = _model(VOCAB_ARCH, VW, _vocab())
    x, y = make_inputs(3, 12, 12, seed=0)
    _check(_flow(VOCAB_ARCH, v, (12, 12), VW), ref, VW, x, y, 1600.0, 3.0)


def test_vocabulary_mixed_batch_through_rows():
    from noise_flow_amd.noise_flow_model import PatchCond
    v, ref = _model(VOCAB_ARCH, VW, _vocab())
    m = _flow(VOCAB_ARCH, v, (12, 12), VW)
    x, y = make_inputs(5, 12, 12, seed=1)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5], np.float32)
    rows = m._rows_to_dev(PatchCond(table), 0)
    _check(m, ref, VW, x, y, table[:, 0], table[:, 1], rows=rows)


@pytest.mark.parametrize("hps", [{"flow_permutation": 0}, {"decomp": "NONE"}])
def test_vocabulary_mixing_layers(hps):
    v, ref = _model(VOCAB_ARCH, VW, _vocab(hps.get("decomp", "LU")), **hps)
    x, y = make_inputs(3, 12, 12, seed=2)
    _check(_flow(VOCAB_ARCH, v, (12, 12), VW, **hps), ref, VW, x, y, 400.0, 1.0)


# ---- 3. patch independence and the grid-stride loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,per_cu", [((32, 32), 2), ((8, 8), 32)])
def test_patch_independence_and_grid_stride(hw, per_cu):
    """B = per_cu x CUs + 3 patches cycling through 7 distinct ones.  A 32x32 workgroup of the 3-coupling model holds 81 KiB of
    LDS (one per CU), an 8x8 one 44 KiB (at most three per CU): in both launches workgroups take a second
    patch on the tiles, gate words and scratch the first one left behind."""
    import torch
    from noise_flow_amd import _lib
    v, _ = _model(WIDE_ARCH, 32)
    m = _flow(WIDE_ARCH, v, hw, 32)
    assert _path(m) == _lib.NF_GRAD_PATH_WIDE32
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = per_cu * n_cu + 3
    x7, y7 = make_inputs(7, hw[0], hw[1], seed=9)
    idx = np.arange(B) % 7
    rc, nll, gx, gy = _call(m, _dev(x7[idx]), _dev(y7[idx]), cond=_cond())
    _lib.check(rc)
    nll, gx, gy = _bits(nll), _bits(gx), _bits(gy)
    assert np.isfinite(nll.view(np.float32)).all() and np.isfinite(gx.view(np.float32)).all() and np.isfinite(gy.view(np.float32)).all()
    for r in range(7):   # every repeat has the bits of the first occurrence
        assert np.all(nll[r::7] == nll[r]) and np.all(gx[r::7] == gx[r]) and np.all(gy[r::7] == gy[r]), r
    for b in range(7):
        rc, n1, gx1, gy1 = _call(m, _dev(x7[b:b + 1]), _dev(y7[b:b + 1]), cond=_cond())
        _lib.check(rc)
        assert _bits(n1)[0] == nll[b] and np.array_equal(_bits(gx1)[0], gx[b]) and np.array_equal(_bits(gy1)[0], gy[b]), b


# ---- 4. output discipline ------------------------------------------------------------------------------------------------------
def test_output_discipline():
    import torch
    from noise_flow_amd import _lib
    hw, B = (9, 13), 3
    v, _ = _model(WIDE_ARCH, 32)
    m = _flow(WIDE_ARCH, v, hw, 32)
    assert _path(m) == _lib.NF_GRAD_PATH_WIDE32
    x, y = make_inputs(B, hw[0], hw[1], seed=1)
    xd, yd = _dev(x), _dev(y)
    n, band = xd.numel(), 1024                       # 4 KiB of floats on both sides
    sentinel = 1234.5
    bufs = [torch.full((n + 2 * band,), sentinel, device="cuda") for _ in range(2)]
    nll = torch.full((B + 2,), sentinel, device="cuda")
    lib, st = m._flow.lib, m._dev.stream_ptr()
    cond = _cond()
    ptrs = [b.data_ptr() + 4 * band for b in bufs]
    _lib.check(lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), B, C.byref(cond), None, nll.data_ptr() + 4, ptrs[0], ptrs[1], st))
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:band] == sentinel) and np.all(h[-band:] == sentinel)
        assert np.isfinite(h).all() and not np.any(h[band:-band] == sentinel)
    hn = nll.cpu().numpy()
    assert hn[0] == sentinel and hn[-1] == sentinel
    # gx_out = NULL: the other outputs keep their bits
    rc, nll2, _, gy2 = _call(m, xd, yd, cond=cond, gx=False)
    _lib.check(rc)
    assert np.array_equal(_bits(nll2), _bits(nll[1:-1])) and np.array_equal(_bits(gy2).reshape(-1), _bits(bufs[1][band:-band]))
    # nll_out = NULL: the gradients keep their bits
    rc, _, gx3, gy3 = _call(m, xd, yd, cond=cond, nll=False)
    _lib.check(rc)
    assert np.array_equal(_bits(gx3).reshape(-1), _bits(bufs[0][band:-band])) and np.array_equal(_bits(gy3).reshape(-1), _bits(bufs[1][band:-band]))
    # B = 0 returns 0 and touches nothing
    before = [b.clone() for b in bufs]
    assert lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), 0, C.byref(cond), None, nll.data_ptr(), ptrs[0], ptrs[1], st) == 0
    assert lib.nf_nll_grad(m._flow.ptr, None, None, 0, C.byref(cond), None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))


# ---- 5. refusals through nf_nll_grad on a flagged handle -------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    import torch
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond

    def refused(m, x, y, gx, gy, cond, rows):
        before = (gx.clone(), gy.clone())
        rc = m._flow.lib.nf_nll_grad(m._flow.ptr, x, y, 2, cond, rows, None, gx.data_ptr(), gy.data_ptr(), m._dev.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error(), rc
        assert torch.equal(before[0], gx) and torch.equal(before[1], gy)   # no launch

    cond = _cond()
    v, _ = _model(WIDE_ARCH, 32)
    m = _flow(WIDE_ARCH, v, (8, 8), 32)
    assert _path(m) == _lib.NF_GRAD_PATH_WIDE32
    x, y = (_dev(a) for a in make_inputs(2, 8, 8))
    gx, gy = torch.zeros_like(x), torch.zeros_like(y)
    rows = m._rows_to_dev(PatchCond(np.array([(800, 2, 0, 0)] * 2, np.float32)), 0)
    refused(m, x.data_ptr(), y.data_ptr(), gx, gy, C.byref(cond), rows.data_ptr())   # both
    refused(m, x.data_ptr(), y.data_ptr(), gx, gy, None, None)                       # neither
    pad = torch.zeros((x.numel() + 4,), device="cuda")
    refused(m, pad.data_ptr() + 4, y.data_ptr(), gx, gy, C.byref(cond), None)        # x misaligned by 4 bytes
    vn, _ = _model(NO_SDN_ARCH, 32)
    mn = _flow(NO_SDN_ARCH, vn, (8, 8), 32)
    refused(mn, x.data_ptr(), None, gx, gy, C.byref(cond), None)                     # gy_out without y


# ---- 6. the flag has no effect on narrow widths ------------------------------------------------------------------------------------
def test_flag_without_effect_at_width_8():
    from noise_flow_amd import _lib
    v, _ = _model(WIDE_ARCH, 8)
    x, y = make_inputs(3, 16, 16, seed=0)
    out = []
    for gk in ("mfma", "scalar"):
        m = _flow(WIDE_ARCH, v, (16, 16), 8, grad_kernel=gk)
        assert _path(m) == _lib.NF_GRAD_PATH_SCALAR
        rc, nll, gx, gy = _call(m, _dev(x), _dev(y), cond=_cond())
        _lib.check(rc)
        out.append((_bits(nll), _bits(gx), _bits(gy)))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---- 7. Python -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [17, 32])
def test_autograd(width):
    import torch
    hw, B = (32, 32), 4
    v, _ = _model(FULL_ARCH, width)
    m = _flow(FULL_ARCH, v, hw, width)
    x, y = make_inputs(B, hw[0], hw[1], seed=2)
    iso, cam = [100.0, 400.0, 800.0, 1600.0], [0.0, 1.0, 2.0, 3.0]
    nll0, gx, gy = m.nll_and_grad(_dev(x), _dev(y), iso=iso, cam=cam)
    assert torch.isfinite(nll0).all() and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    xt, yt = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
    w = torch.rand((B,), device="cuda") + 0.5
    nll = m.nll_torch(xt, yt, iso=iso, cam=cam)
    (w * nll).sum().backward()
    assert torch.equal(nll.detach(), nll0)
    assert torch.equal(xt.grad, w[:, None, None, None] * gx) and torch.equal(yt.grad, w[:, None, None, None] * gy)
    # numpy in, numpy out
    n_np, gx_np, gy_np = m.nll_and_grad(x, y, iso=iso, cam=cam)
    assert isinstance(gx_np, np.ndarray) and np.array_equal(gx_np, gx.cpu().numpy()) and np.array_equal(gy_np, gy.cpu().numpy())


def test_grad_kernel_keyword():
    from noise_flow_amd import _lib
    v, _ = _model(WIDE_ARCH, 32)
    with pytest.raises(ValueError):
        _flow(WIDE_ARCH, v, (32, 32), 32, grad_kernel="mfma", cnn_dtype="fp16")
    with pytest.raises(ValueError):
        _flow(WIDE_ARCH, v, (32, 32), 32, grad_kernel="tensor")
    # the default at width 32, 32x32: refused by nf_nll_grad as before
    m = _flow(WIDE_ARCH, v, (32, 32), 32, grad_kernel=None)
    assert m.grad_kernel == "scalar" and _path(m) == _lib.NF_EINVAL
    x, y = make_inputs(1, 32, 32, seed=0)
    with pytest.raises(_lib.NoiseFlowLibError):
        m.nll_and_grad(_dev(x), _dev(y), iso=[ISO], cam=[CAM])
