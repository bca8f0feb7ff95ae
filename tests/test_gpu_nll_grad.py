"""nf_nll_grad: d nll / d x and d nll / d y of the evaluation-mode NLL, from the kernel up to torch.autograd.

Comparison rule, for gx and gy alike and per patch:  max|kernel - ref64| <= tol * max|ref64|,  tol = max(1e-5, 4 * e32).
1e-5 is the project's tensor tolerance (conftest.close_elem); e32 is the float32 reference's own distance from the float64
reference on the same tensor and input (tests/nll_grad_ref.py) — nothing the kernel computes enters it; the factor 4 covers a
different summation order plus the rounding of the reversible sweep's reconstruction.  A wrong tap, a missing term or a wrong
border gives 1e-3 or more.

Kink rule: a patch that fails is re-compared against the float64 reference with at most MAX_EXCUSED_KINKS = 3 of THAT patch's
reported on-kink gates inverted (the rule of conftest.grads_match_up_to_kinks).  Kink condition: seeds are fixed so that no
patch has more than 6 on-kink activations, asserted from the reference before the kernel's output is looked at.

The same comparison is made once more in the WHITENED norm, on g / w with e32 measured in that norm; a patch must pass both, and
one subset of gates has to excuse both (tests/nll_grad_ref.py: the rule, the weights, what each norm can see).  Every case first
asserts, from the reference alone, that the pinned e32 is at most E32_MAX = 5e-6 in both norms and the kink count above; the three
larger shipped-model cases also assert max / median |gy| >= 100.

Every case also holds nll_out to the fp64 reference at NLL_RTOL = 1e-5.  Measured distances are printed (run with -s).  On an
MI355X, worst patch of all cases, raw / whitened: gx 2.4e-6 / 3.4e-6, gy 2.6e-6 / 3.2e-6 of the norm's maximum; shipped 32x32: gx
1.5e-6 / 2.3e-6, gy 1.6e-6 / 1.7e-6 (e32 1.3e-6 / 2.3e-6, 9.6e-7 / 2.0e-6).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables
from nll_grad_ref import PinnedRef, compare_with_kink_rule, reference_conditions
from test_cond_rows_cpu import cond_variables

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-5
ISO, CAM = 800.0, 2.0
WIDE_ARCH = "sdn5|unc|unc|gain4|unc"
VOCAB_ARCH = "sdn5|unc|gain|unc|sdn3"
TUPLES5 = [(100, 0), (400, 1), (800, 2), (1600, 3), (3200, 4)]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _flow(arch, variables, hw, width=4, cnn_dtype="fp32", **hps):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, cnn_dtype=cnn_dtype)


def _call(m, x, y, cond=None, rows=None, nll=True, gx=True, gy=True, B=None):
    """nf_nll_grad on device tensors → (return code, nll, gx, gy) with the outputs as device tensors (None where not asked)."""
    import torch
    B = int(x.shape[0]) if B is None else B
    o_nll = torch.empty((max(B, 1),), device="cuda") if nll else None
    o_gx = torch.empty_like(x) if gx else None
    o_gy = torch.empty_like(y) if (gy and y is not None) else None
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, p(x), p(y), B, C.byref(cond) if cond is not None else None, p(rows), p(o_nll), p(o_gx), p(o_gy),
                                 m._dev.stream_ptr())
    return rc, o_nll, o_gx, o_gy


def _cond(iso=ISO, cam=CAM):
    from noise_flow_amd import _lib
    return _lib.nf_cond(float(iso), float(cam), 0.0, 0.0)


def _check(m, ref, width, x, y, iso, cam, rows=None, min_gy_range=None):
    """One launch against the reference: the preconditions from the reference alone, then the comparison and kink rules
    (module docstring)."""
    from noise_flow_amd import _lib
    reference_conditions(ref, width, x, y, iso, cam, min_gy_range=min_gy_range)
    xd, yd = _dev(x), (_dev(y) if y is not None else None)
    rc, nll, gx, gy = _call(m, xd, yd, cond=None if rows is not None else (_cond(iso, cam) if iso is not None else _cond()), rows=rows)
    _lib.check(rc)
    nll64, dist = compare_with_kink_rule(ref, width, x, y, iso, cam, gx.cpu().numpy(), gy.cpu().numpy() if gy is not None else None, log=print)
    # nll_out against NoiseFlowOracle.nll itself; the helper whose gradients are the reference must BE that function on this model
    # and input (fp64, another summation order: held to 1e-12 as in tests/test_nll_grad_ref_cpu.py)
    want = ref.oracle_nll(x, y, iso, cam)
    assert np.all(np.abs(nll64 - want) <= 1e-12 * np.abs(want)), (nll64, want)
    got = nll.cpu().numpy().astype(np.float64)
    print("nll: kernel-to-oracle %s" % " ".join("%.2e" % v for v in np.abs(got - want) / np.abs(want)))
    assert np.all(np.abs(got - want) <= NLL_RTOL * np.abs(want))
    return dist


# ---- 1. the shipped model ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped_ref(shipped_variables):
    return PinnedRef(FULL_ARCH, shipped_variables)


# on-kink activations per patch and the largest pinned e32 over patches, tensors and both norms, on the CPU reference:
# (32,32) [0,2,1] 1.5e-6   (9,13) [0,0,0] 9.4e-7   (64,64) [2,3,3] 2.8e-6   (1,1) [0,0,0] 2.0e-6   (1,5) seed 2 [0,0,0] 1.2e-6
# ((1,5) at seed 0 misses the precondition: pinned e32 of gx 5.3e-6 raw / 5.7e-6 whitened on patch 2; seed 1 meets it at 3.8e-6
# on one host CPU and 4.0e-6 on another, too near the cap to rely on); max / median |gy| of the three range cases: 1746, 1791, 4307.
# Across two host CPUs the e32 of a case moves by up to a third: (64,64) 2.8e-6 / 3.6e-6.
SHIPPED_CASES = [((32, 32), 0), ((9, 13), 0), ((64, 64), 0), ((1, 1), 0), ((1, 5), 2)]
GY_RANGE_CASES = ((32, 32), (64, 64), (9, 13))     # max / median |gy| >= GY_RANGE, asserted from the reference
GY_RANGE = 100.0


@pytest.mark.parametrize("hw,seed", SHIPPED_CASES)
def test_shipped_model(shipped_variables, shipped_ref, hw, seed):
    x, y = make_inputs(3, hw[0], hw[1], seed=seed)
    _check(_flow(FULL_ARCH, shipped_variables, hw), shipped_ref, 4, x, y, ISO, CAM, min_gy_range=GY_RANGE if hw in GY_RANGE_CASES else None)


# ---- 2. perturbed models, widths 4 / 8 / 16 / 32 ----------------------------------------------------------------------------------
# on-kink per patch, largest pinned e32 (seed 0): width 4 [0,0,0] 2.3e-7   8 [0,1,0] 2.8e-7   16 (16,16) [0,0,1] 1.1e-6
# 16 (32,32) [0,1,0] 1.4e-6   8 (48,48) [3,2,3] 4.0e-7   32 [0,1,1] 1.8e-6; the whitened norm coincides with the raw one on these models
TRAINED_CASES = [(4, (16, 16), 0), (8, (16, 16), 0), (16, (16, 16), 0), (16, (32, 32), 0),
                 (8, (48, 48), 0),      # width 8 beyond 32x32: 4 pixels per lane at 1 024 threads
                 (32, (16, 16), 0)]     # width 32: one pixel per lane


@pytest.mark.parametrize("width,hw,seed", TRAINED_CASES)
def test_trained_like_widths(width, hw, seed):
    v = trained_like_variables(WIDE_ARCH, width)
    x, y = make_inputs(3, hw[0], hw[1], seed=seed)
    _check(_flow(WIDE_ARCH, v, hw, width), PinnedRef(WIDE_ARCH, v), width, x, y, ISO, CAM)


# ---- 3. vocabulary and conditioning ------------------------------------------------------------------------------------------
def _vocab_variables(decomp="LU"):
    """As tests/test_gpu_percond.py::_model: conditional layers off their initial values, gain scales of O(1) at every ISO."""
    from oracle import nf_oracle as O
    v = cond_variables(VOCAB_ARCH, 4, seed=5)
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


# on-kink per patch, largest pinned e32: per-call [0,0,0] 1.1e-6   rows [0,0,0,0,0] 1.3e-6   perm0 [0,0,0] 3.1e-7   NONE [0,0,0] 8.0e-7
# no-sdn 8x8 [0,0,0] 2.2e-7
def test_vocabulary_per_call_cond():
    v = _vocab_variables()
    x, y = make_inputs(3, 12, 12, seed=0)
    _check(_flow(VOCAB_ARCH, v, (12, 12)), PinnedRef(VOCAB_ARCH, v), 4, x, y, 1600.0, 3.0)


def test_vocabulary_mixed_batch_through_rows():
    from noise_flow_amd.noise_flow_model import PatchCond
    v = _vocab_variables()
    m = _flow(VOCAB_ARCH, v, (12, 12))
    x, y = make_inputs(5, 12, 12, seed=1)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5], np.float32)
    rows = m._rows_to_dev(PatchCond(table), 0)
    _check(m, PinnedRef(VOCAB_ARCH, v), 4, x, y, table[:, 0], table[:, 1], rows=rows)


@pytest.mark.parametrize("hps", [{"flow_permutation": 0}, {"decomp": "NONE"}])
def test_vocabulary_mixing_layers(hps):
    v = _vocab_variables(hps.get("decomp", "LU"))
    x, y = make_inputs(3, 12, 12, seed=2)
    ref = PinnedRef(VOCAB_ARCH, v, flow_permutation=hps.get("flow_permutation", 1), decomp=hps.get("decomp", "LU"))
    _check(_flow(VOCAB_ARCH, v, (12, 12), **hps), ref, 4, x, y, 400.0, 1.0)


# ---- 4. a model without an SDN layer: y = NULL ---------------------------------------------------------------------------------
def test_model_without_sdn():
    import torch
    from noise_flow_amd import _lib
    arch = "unc|gain4|unc"
    v = trained_like_variables(arch, 4, seed=3)
    m = _flow(arch, v, (8, 8))
    x = np.random.RandomState(0).randn(3, 8, 8, 4).astype(np.float32)
    _check(m, PinnedRef(arch, v), 4, x, None, None, None)
    xd = _dev(x)
    gy = torch.empty_like(xd)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), None, 3, C.byref(_cond()), None, None, None, gy.data_ptr(), m._dev.stream_ptr())
    assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error()


# ---- 5. patch independence and the grid-stride loop ------------------------------------------------------------------------------
def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


@pytest.mark.parametrize("hw,per_cu", [((8, 8), 4), ((8, 8), 32), ((32, 32), 4)])
def test_patch_independence_and_grid_stride(shipped_variables, hw, per_cu):
    """B = per_cu * (number of CUs) + 3 patches cycling through 7 distinct ones.  The launch is a persistent grid of at most
    (resident workgroups per CU) x CUs workgroups, so a workgroup takes a SECOND patch only when B exceeds that: at 8x8 the
    launcher's cap is 32 per CU (B = 32 CUs + 3 exceeds it whatever the occupancy; B = 4 CUs + 3 is one patch per workgroup),
    at 32x32 the 36 KiB of LDS per workgroup allow at most 4 per CU (the kernel's registers: 2), so B = 4 CUs + 3 makes every
    workgroup run the loop at least twice — on tiles, gate words and reduction scratch the previous patch left behind."""
    import torch
    from noise_flow_amd import _lib
    m = _flow(FULL_ARCH, shipped_variables, hw)
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


# ---- 6. output discipline ----------------------------------------------------------------------------------------------------
def test_output_discipline(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    hw, B = (9, 13), 3
    m = _flow(FULL_ARCH, shipped_variables, hw)
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
    # B = 0 returns 0 and touches nothing
    before = [b.clone() for b in bufs]
    assert lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), 0, C.byref(cond), None, nll.data_ptr(), ptrs[0], ptrs[1], st) == 0
    assert lib.nf_nll_grad(m._flow.ptr, None, None, 0, C.byref(cond), None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))


# ---- 7. refusals through nf_nll_grad itself -------------------------------------------------------------------------------------
def test_refusals(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond

    def refused(m, x, y, gx, gy, cond, rows):
        before = (gx.clone(), gy.clone())
        rc = m._flow.lib.nf_nll_grad(m._flow.ptr, x, y, 2, cond, rows, None, gx.data_ptr() if isinstance(gx, torch.Tensor) else gx,
                                     gy.data_ptr(), m._dev.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error(), rc
        assert torch.equal(before[0], gx) and torch.equal(before[1], gy)   # no launch

    cond = _cond()
    for hw, dtype in (((32, 32), "fp16"), ((65, 65), "fp32")):
        m = _flow(FULL_ARCH, shipped_variables, hw, cnn_dtype=dtype)
        x, y = (_dev(a) for a in make_inputs(2, hw[0], hw[1]))
        refused(m, x.data_ptr(), y.data_ptr(), torch.zeros_like(x), torch.zeros_like(y), C.byref(cond), None)
    m = _flow(FULL_ARCH, shipped_variables, (8, 8))
    x, y = (_dev(a) for a in make_inputs(2, 8, 8))
    gx, gy = torch.zeros_like(x), torch.zeros_like(y)
    rows = m._rows_to_dev(PatchCond(np.array([(800, 2, 0, 0)] * 2, np.float32)), 0)
    refused(m, x.data_ptr(), y.data_ptr(), gx, gy, C.byref(cond), rows.data_ptr())   # both
    refused(m, x.data_ptr(), y.data_ptr(), gx, gy, None, None)                       # neither
    pad = torch.zeros((x.numel() + 4,), device="cuda")
    refused(m, pad.data_ptr() + 4, y.data_ptr(), gx, gy, C.byref(cond), None)        # x misaligned by 4 bytes


# ---- 8. autograd ---------------------------------------------------------------------------------------------------------------
def test_autograd(shipped_variables):
    import torch
    hw, B = (16, 16), 4
    m = _flow(FULL_ARCH, shipped_variables, hw)
    x, y = make_inputs(B, hw[0], hw[1], seed=2)
    iso, cam = [100.0, 400.0, 800.0, 1600.0], [0.0, 1.0, 2.0, 3.0]
    nll0, gx, gy = m.nll_and_grad(_dev(x), _dev(y), iso=iso, cam=cam)
    xt, yt = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
    w = torch.rand((B,), device="cuda") + 0.5
    nll = m.nll_torch(xt, yt, iso=iso, cam=cam)
    (w * nll).sum().backward()
    assert torch.equal(nll.detach(), nll0)
    assert torch.equal(xt.grad, w[:, None, None, None] * gx) and torch.equal(yt.grad, w[:, None, None, None] * gy)
    # numpy in, numpy out
    n_np, gx_np, gy_np = m.nll_and_grad(x, y, iso=iso, cam=cam)
    assert isinstance(gx_np, np.ndarray) and np.array_equal(gx_np, gx.cpu().numpy()) and np.array_equal(gy_np, gy.cpu().numpy())
    # only x needs a gradient
    x2 = _dev(x).requires_grad_(True)
    m.nll_torch(x2, _dev(y), iso=iso, cam=cam).sum().backward()
    assert torch.equal(x2.grad, gx)
    # the backward pass treats gx / gy as constants: a second differentiation raises instead of returning zeros
    x3 = _dev(x).requires_grad_(True)
    g1, = torch.autograd.grad(m.nll_torch(x3, _dev(y), iso=iso, cam=cam).sum(), x3, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # without autograd: the bits of _loss
    with torch.no_grad():
        plain = m.nll_torch(xt, yt, iso=iso, cam=cam)
    assert not plain.requires_grad and torch.equal(plain, m._loss(_dev(x), _dev(y), iso=iso, cam=cam)[0])
    # wrapper pass-throughs exist; batch-statistics models raise
    from noise_flow_amd import NoiseFlow, NoiseFlowWrapper, default_hps
    assert callable(NoiseFlowWrapper.nll_torch) and callable(NoiseFlowWrapper.nll_and_grad)
    mt = NoiseFlow([hw[0], hw[1], 4], True, default_hps(arch=FULL_ARCH, width=4), variables=shipped_variables)
    with pytest.raises(NotImplementedError):
        mt.nll_and_grad(_dev(x), _dev(y), iso=[ISO], cam=[CAM])
    with pytest.raises(NotImplementedError):
        mt.nll_torch(xt, yt, iso=[ISO], cam=[CAM])


# ---- 9. use level: gradient descent on x lowers the NLL -----------------------------------------------------------------------------
def test_descent_on_x_lowers_nll(shipped_variables):
    m = _flow(FULL_ARCH, shipped_variables, (16, 16))
    x, y = make_inputs(1, 16, 16, seed=5)
    xd, yd = _dev(3.0 * x), _dev(y)                    # a noisy start: 3 x the model's noise level
    nll, gx, _ = m.nll_and_grad(xd, yd, iso=[ISO], cam=[CAM])
    # Step from the first gradient: (g.g) / (x.g) is the gradient-weighted mean curvature of the NLL along x; the largest
    # curvature around this input is well above it (the noise variance of the sdn layer spans three decades over y in [0, 1],
    # and the couplings add their own).  On the CPU reference (tests/nll_grad_ref.py, fp64) 1/32 of the inverse mean curvature
    # still overshoots on some of the 20 steps, 1/64 and 1/128 descend monotonically; 1/128 is used, where the smallest
    # decrease of a step is 1.3 nats — 1e4 ulps of the reported fp32 NLL.
    step = float((xd * gx).sum() / (gx * gx).sum()) / 128.0
    trace = [float(nll[0])]
    for _ in range(20):
        xd = xd - step * gx
        nll, gx, _ = m.nll_and_grad(xd, yd, iso=[ISO], cam=[CAM])
        trace.append(float(nll[0]))
    print("nll along the descent:", " ".join("%.1f" % v for v in trace))
    assert all(b < a for a, b in zip(trace, trace[1:])), trace
