"""nf_sample_vjp: d L / d y, d L / d eps and d L / d temp of x = sample(y, eps, temp), from the kernel up to torch.autograd.

The rule, its weights, preconditions and kink handling are those of tests/sample_vjp_ref.py (constants of tests/nll_grad_ref.py); the
cases are the ones the CPU tier runs the reversible float32 sweep on (tests/test_sample_vjp_rule_cpu.py).  x_out is held to
``NoiseFlowOracle.sample`` by conftest.close_elem at 1e-5.  Measured distances are printed (run with -s).

Measured on an MI355X, worst patch of the 17 accuracy cases, distance to fp64 (pinned e32 of that patch): geps 4.7e-6 raw (1.5e-6; 0.47
of the bound, shipped 9x13) and 2.1e-6 whitened (2.4e-6), gy 2.1e-6 in both norms (1.3e-6), gtemp 1.2e-7 (3.5e-7).  No patch needs the
kink rule.  The (8, 48x48) case runs the 768-thread geometry of padded width 8 (csrc/nf_sample_grad.hip, dispatch_sgrad): that width's
1 024-thread build gave geps 1.06 / 1.25 / 0.88 of max|geps| on its three patches (x and gy right) and is not instantiated.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, close_elem, make_inputs
from sample_vjp_ref import (CAM, CASES, ISO, TUPLES5, WIDE_ARCH, case_model, compare_with_kink_rule, get_case, oracle_sample, reference_conditions,
                            sampling_variables)

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _flow(arch, variables, hw, width=4, cnn_dtype="fp32", **kw):
    from noise_flow_amd import NoiseFlow, default_hps
    hps = {k: kw.pop(k) for k in ("flow_permutation", "decomp") if k in kw}
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, cnn_dtype=cnn_dtype, **kw)


def _cond(iso=ISO, cam=CAM):
    from noise_flow_amd import _lib
    return _lib.nf_cond(float(iso if iso is not None else ISO), float(cam if cam is not None else CAM), 0.0, 0.0)


def _call(m, y, eps, g, temp, cond=None, rows=None, x=True, gy=True, geps=True, gtemp=True, B=None, seed=0, base=0):
    """nf_sample_vjp on device tensors → (return code, x, gy, geps, gtemp), device tensors or None where not asked."""
    import torch
    B = int(g.shape[0]) if B is None else B
    o_x = torch.empty_like(g) if x else None
    o_gy = torch.empty_like(g) if (gy and y is not None) else None
    o_ge = torch.empty_like(g) if geps else None
    o_gt = torch.empty((max(B, 1),), device="cuda") if gtemp else None
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = m._flow.lib.nf_sample_vjp(m._flow.ptr, p(y), p(eps), seed, base, float(temp), B, C.byref(cond) if cond is not None else None, p(rows),
                                   p(g), p(o_x), p(o_gy), p(o_ge), p(o_gt), m._dev.stream_ptr())
    return rc, o_x, o_gy, o_ge, o_gt


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


# ---- 1. the rule on every case -------------------------------------------------------------------------------------------------------
def _model_of(name, shipped_variables, hw):
    arch, v, width, hps = case_model(name, shipped_variables)
    return _flow(arch, v, hw, width, **hps)


@pytest.mark.parametrize("name", CASES, ids=repr)
def test_rule(shipped_variables, name):
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond
    ref, width, y, eps, g, temp, iso, cam = get_case(name, shipped_variables)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    hw = eps.shape[1:3]
    m = _model_of(name, shipped_variables, hw)
    rows = None
    if name[0] == "vocab" and name[1].get("rows"):
        rows = m._rows_to_dev(PatchCond(np.array([(i, c, 0, 0) for i, c in TUPLES5], np.float32)), 1)
    rc, x, gy, ge, gt = _call(m, _dev(y) if y is not None else None, _dev(eps), _dev(g), temp, cond=None if rows is not None else _cond(iso, cam), rows=rows)
    _lib.check(rc)
    got = (gy.cpu().numpy() if gy is not None else None, ge.cpu().numpy(), gt.cpu().numpy())
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got, log=print)
    print("x: worst masked element %.2e" % close_elem(x.cpu().numpy(), oracle_sample(ref, y, eps, temp, iso, cam), 1e-5))


def test_model_without_sdn_refuses_gy(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    ref, width, y, eps, g, temp, iso, cam = get_case(("nosdn",), shipped_variables)
    m = _model_of(("nosdn",), shipped_variables, (8, 8))
    gd = _dev(g)
    gy = torch.zeros_like(gd)
    rc = m._flow.lib.nf_sample_vjp(m._flow.ptr, None, _dev(eps).data_ptr(), 0, 0, 1.0, 3, C.byref(_cond()), None, gd.data_ptr(), None,
                                   gy.data_ptr(), None, None, m._dev.stream_ptr())
    assert rc == _lib.NF_EINVAL and b"gy_out must be NULL" in m._flow.lib.nf_last_error()


# ---- 2. eps = NULL: the bits of the same call fed nf_sample_eps's draw -------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(9, 13), (32, 32)])
def test_philox_eps_is_nf_sample_eps(shipped_variables, hw):
    import torch
    from noise_flow_amd import _lib
    m = _flow(FULL_ARCH, shipped_variables, hw)
    B, seed, base = 5, 1234567, 40
    y = _dev(make_inputs(B, hw[0], hw[1], seed=3)[1])
    g = _dev(np.random.RandomState(5).randn(B, hw[0], hw[1], 4).astype(np.float32))
    e = torch.empty_like(g)
    _lib.check(m._flow.lib.nf_sample_eps(seed, base, B, hw[0], hw[1], e.data_ptr(), m._dev.stream_ptr()))
    a = _call(m, y, None, g, 0.6, cond=_cond(), seed=seed, base=base)
    b = _call(m, y, e, g, 0.6, cond=_cond())
    _lib.check(a[0])
    _lib.check(b[0])
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(_bits(u), _bits(v))
    # and x is nf_sample's own sample of that draw, to the tensor tolerance (another kernel: not the same bits)
    xs = m.sample(y, eps_std=0.6, yy=y, iso=[ISO], cam=[CAM], eps=e)
    close_elem(a[1].cpu().numpy(), xs.cpu().numpy(), 1e-5)


# ---- 3. patch independence and the grid-stride loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,per_cu", [((8, 8), 4), ((8, 8), 32), ((32, 32), 4)])
def test_patch_independence_and_grid_stride(shipped_variables, hw, per_cu):
    """As tests/test_gpu_nll_grad.py: B = per_cu x CUs + 3 patches cycling through 7 distinct ones, so that at 32 per CU (8x8) and at 4
    per CU (32x32: 36 KiB of LDS per workgroup) every workgroup runs the loop more than once, on tiles, gate words and reduction
    scratch the previous patch left behind."""
    import torch
    from noise_flow_amd import _lib
    m = _flow(FULL_ARCH, shipped_variables, hw)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = per_cu * n_cu + 3
    y7 = make_inputs(7, hw[0], hw[1], seed=9)[1]
    rng = np.random.RandomState(11)
    e7, g7 = (rng.randn(7, hw[0], hw[1], 4).astype(np.float32) for _ in range(2))
    idx = np.arange(B) % 7
    out = _call(m, _dev(y7[idx]), _dev(e7[idx]), _dev(g7[idx]), 0.6, cond=_cond())
    _lib.check(out[0])
    outs = [_bits(t) for t in out[1:]]
    assert all(np.isfinite(o.view(np.float32)).all() for o in outs)
    for r in range(7):   # every repeat has the bits of the first occurrence
        assert all(np.all(o[r::7] == o[r]) for o in outs), r
    for b in range(7):
        one = _call(m, _dev(y7[b:b + 1]), _dev(e7[b:b + 1]), _dev(g7[b:b + 1]), 0.6, cond=_cond())
        _lib.check(one[0])
        assert all(np.array_equal(_bits(t)[0], o[b]) for t, o in zip(one[1:], outs)), b


# ---- 4. output discipline ------------------------------------------------------------------------------------------------------------
def test_output_discipline(shipped_variables):
    import itertools
    import torch
    from noise_flow_amd import _lib
    hw, B = (9, 13), 3
    m = _flow(FULL_ARCH, shipped_variables, hw)
    y = _dev(make_inputs(B, hw[0], hw[1], seed=1)[1])
    rng = np.random.RandomState(2)
    eps, g = (_dev(rng.randn(B, hw[0], hw[1], 4).astype(np.float32)) for _ in range(2))
    n, band = g.numel(), 1024                        # 4 KiB of floats on both sides
    sentinel = 1234.5
    bufs = [torch.full((n + 2 * band,), sentinel, device="cuda") for _ in range(3)]
    gt = torch.full((B + 2,), sentinel, device="cuda")
    lib, st = m._flow.lib, m._dev.stream_ptr()
    cond = _cond()
    ptrs = [b.data_ptr() + 4 * band for b in bufs]
    _lib.check(lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 0.6, B, C.byref(cond), None, g.data_ptr(), ptrs[0], ptrs[1],
                                 ptrs[2], gt.data_ptr() + 4, st))
    for b in bufs:
        h = b.cpu().numpy()
        assert np.all(h[:band] == sentinel) and np.all(h[-band:] == sentinel)
        assert np.isfinite(h).all() and not np.any(h[band:-band] == sentinel)
    hn = gt.cpu().numpy()
    assert hn[0] == sentinel and hn[-1] == sentinel and np.isfinite(hn).all() and not np.any(hn[1:-1] == sentinel)
    full = [_bits(b[band:-band]) for b in bufs] + [_bits(gt[1:-1])]
    # every subset of the outputs keeps the other outputs' bits
    for keep in itertools.product((False, True), repeat=4):
        rc, *outs = _call(m, y, eps, g, 0.6, cond=cond, x=keep[0], gy=keep[1], geps=keep[2], gtemp=keep[3])
        _lib.check(rc)
        for k, o, f in zip(keep, outs, full):
            assert (o is None) == (not k)
            if k:
                assert np.array_equal(_bits(o).reshape(-1), f), keep
    # B = 0 returns 0 and touches nothing
    before = [b.clone() for b in bufs] + [gt.clone()]
    assert lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 0.6, 0, C.byref(cond), None, g.data_ptr(), ptrs[0], ptrs[1], ptrs[2],
                             gt.data_ptr(), st) == 0
    assert lib.nf_sample_vjp(m._flow.ptr, None, None, 0, 0, 0.6, 0, C.byref(cond), None, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs + [gt]))


# ---- 5. refusals through nf_sample_vjp itself, and their messages ------------------------------------------------------------------------
def test_refusals(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond

    def refused(m, y, eps, g, out, cond, rows, word, B=2):
        before = out.clone()
        rc = m._flow.lib.nf_sample_vjp(m._flow.ptr, y, eps, 0, 0, 1.0, B, cond, rows, g, None, None, out.data_ptr(), None, m._dev.stream_ptr())
        torch.cuda.synchronize()
        msg = (m._flow.lib.nf_last_error() or b"").decode()
        assert rc == _lib.NF_EINVAL and word in msg, (rc, msg)
        assert torch.equal(before, out)   # no launch

    cond = _cond()
    # handles the kernel does not serve: fp16, a shape not held whole (with and without NF_CFG_GRAD_TILED), the matrix-core layout
    for hw, kw, word in (((32, 32), {"cnn_dtype": "fp16"}, "fp32 handles only"), ((65, 65), {}, "64x64"),
                         ((65, 65), {"grad_tiles": True}, "no tile mode")):
        m = _flow(FULL_ARCH, shipped_variables, hw, **kw)
        y, eps = (_dev(a) for a in make_inputs(2, hw[0], hw[1]))
        refused(m, y.data_ptr(), eps.data_ptr(), eps.data_ptr(), torch.zeros_like(eps), C.byref(cond), None, word)
    m = _flow(WIDE_ARCH, sampling_variables(WIDE_ARCH, 32), (16, 16), 32, grad_kernel="mfma")
    y, eps = (_dev(a) for a in make_inputs(2, 16, 16))
    refused(m, y.data_ptr(), eps.data_ptr(), eps.data_ptr(), torch.zeros_like(eps), C.byref(cond), None, "matrix-core layout")
    # arguments
    m = _flow(FULL_ARCH, shipped_variables, (8, 8))
    y, eps = (_dev(a) for a in make_inputs(2, 8, 8))
    out = torch.zeros_like(eps)
    rows = m._rows_to_dev(PatchCond(np.array([(800, 2, 0, 0)] * 2, np.float32)), 1)
    refused(m, y.data_ptr(), eps.data_ptr(), eps.data_ptr(), out, C.byref(cond), rows.data_ptr(), "exactly one of cond / rows")   # both
    refused(m, y.data_ptr(), eps.data_ptr(), eps.data_ptr(), out, None, None, "exactly one of cond / rows")                        # neither
    refused(m, y.data_ptr(), eps.data_ptr(), None, out, C.byref(cond), None, "gx_in is NULL")
    refused(m, None, eps.data_ptr(), eps.data_ptr(), out, C.byref(cond), None, "y is NULL")
    refused(m, y.data_ptr(), eps.data_ptr(), eps.data_ptr(), out, C.byref(cond), None, "B must be >= 0", B=-1)
    pad = torch.zeros((eps.numel() + 4,), device="cuda")
    refused(m, y.data_ptr(), eps.data_ptr(), pad.data_ptr() + 4, out, C.byref(cond), None, "16-byte aligned")    # gx_in misaligned by 4 bytes


# ---- 6. sample_and_vjp and sample_torch ------------------------------------------------------------------------------------------------
def test_sample_torch(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 4
    m = _flow(FULL_ARCH, shipped_variables, hw)
    y = make_inputs(B, hw[0], hw[1], seed=2)[1]
    rng = np.random.RandomState(3)
    eps, g = (rng.randn(B, hw[0], hw[1], 4).astype(np.float32) for _ in range(2))
    iso, cam = [100.0, 400.0, 800.0, 1600.0], [0.0, 1.0, 2.0, 3.0]
    x0, gy0, ge0, gt0 = m.sample_and_vjp(_dev(y), _dev(g), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=_dev(eps))
    # x is the wrapper's own sample; numpy in, numpy out
    close_elem(x0.cpu().numpy(), m.sample(_dev(y), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=_dev(eps)).cpu().numpy(), 1e-5)
    out_np = m.sample_and_vjp(y, g, eps_std=0.6, yy=y, iso=iso, cam=cam, eps=eps)
    assert all(isinstance(a, np.ndarray) and np.array_equal(a, b.cpu().numpy()) for a, b in zip(out_np, (x0, gy0, ge0, gt0)))
    # autograd: the backward pass's bits are the direct call's
    yt, et = _dev(y).requires_grad_(True), _dev(eps).requires_grad_(True)
    std = torch.tensor(0.6, device="cuda", requires_grad=True)
    x = m.sample_torch(yt, eps=et, eps_std=std, iso=iso, cam=cam)
    assert x.requires_grad and torch.equal(x.detach(), m.sample(_dev(y), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=_dev(eps)))
    (x * _dev(g)).sum().backward()
    assert torch.equal(yt.grad, gy0) and torch.equal(et.grad, ge0) and torch.equal(std.grad, gt0.sum())
    # only yy needs a gradient; the in-kernel draw under a seed is the one sample() makes, and its gradient the direct call's on that draw
    m2 = _flow(FULL_ARCH, shipped_variables, hw)
    y2 = _dev(y).requires_grad_(True)
    x2 = m2.sample_torch(y2, seed=77, eps_std=0.6, iso=iso, cam=cam)
    (x2 * _dev(g)).sum().backward()
    e77 = torch.empty_like(x2)
    _lib.check(m2._flow.lib.nf_sample_eps(77, 0, B, hw[0], hw[1], e77.data_ptr(), m2._dev.stream_ptr()))
    _, gy77, _, _ = m2.sample_and_vjp(_dev(y), _dev(g), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=e77)
    assert torch.equal(y2.grad, gy77)
    # nothing requires grad, or grad mode is off: no graph
    assert not m.sample_torch(_dev(y), eps=_dev(eps), iso=iso, cam=cam).requires_grad
    with torch.no_grad():
        assert not m.sample_torch(yt, eps=et, iso=iso, cam=cam).requires_grad
    # the backward pass treats its results as constants: a second differentiation raises instead of returning zeros
    y3 = _dev(y).requires_grad_(True)
    g1, = torch.autograd.grad((m.sample_torch(y3, eps=_dev(eps), iso=iso, cam=cam) * _dev(g)).sum(), y3, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # evaluation mode only
    from noise_flow_amd import NoiseFlow, default_hps
    mt = NoiseFlow([hw[0], hw[1], 4], True, default_hps(arch=FULL_ARCH, width=4), variables=shipped_variables)
    with pytest.raises(NotImplementedError):
        mt.sample_torch(yt, eps=et, iso=[ISO], cam=[CAM])
    with pytest.raises(NotImplementedError):
        mt.sample_and_vjp(_dev(y), _dev(g), yy=_dev(y), iso=[ISO], cam=[CAM], eps=_dev(eps))
