"""nf_sample_vjp on the GEMM kernel (NF_CFG_SVJP_GEMM, csrc/nf_sample_grad_gemm.hip): coupling widths 33 .. 512, whole patches up to
32x32, from the kernel up to torch.autograd.

The rule, its weights, preconditions and kink handling are those of tests/sample_vjp_ref.py (constants of tests/nll_grad_ref.py): per
patch max|got - g64| <= max(1e-5, 4 e32) max|g64| in the raw and in the whitened norm, gtemp against sum|g eps|, ``reference_conditions``
asserted from the reference before any kernel output is read; x_out is held to ``NoiseFlowOracle.sample`` by conftest.close_elem at
1e-5.  Models and cases: tests/sample_vjp_gemm_cases.py, the ones tests/test_sample_vjp_gemm_cpu.py runs the reversible float32 sweep
on.  Every case asserts that the handle launches NF_SVJP_PATH_GEMM.  Measured distances are printed (run with -s).

Measured on an MI355X, worst patch of the 24 accuracy cases, distance to fp64 (pinned e32 of that patch): geps 1.23e-6 in both norms
(6.9e-7; 0.12 of the bound), gy 7.6e-7 in both norms (4.9e-7), gtemp 2.1e-7 (5.1e-8).  No patch needs the kink rule.  x_out: within
9.8e-5 relative on every element above 1e-3 of the patch scale (bound 1e-5 of the scale).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import close_elem, make_inputs
from sample_vjp_gemm_cases import EMBEDDED_WIDTHS, NAMES, embedded_case, get_case, model
from sample_vjp_ref import (TUPLES5, WIDE_ARCH, case_inputs, compare_with_kink_rule, oracle_sample, reference_conditions, sampling_variables)
from test_gpu_sample_vjp import _bits, _call, _cond, _dev

pytestmark = pytest.mark.gpu


def _flow(arch, variables, hw, width, cnn_dtype="fp32", sample_vjp_kernel="gemm", **kw):
    from noise_flow_amd import NoiseFlow, default_hps
    hps = {k: kw.pop(k) for k in ("flow_permutation", "decomp") if k in kw}
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, cnn_dtype=cnn_dtype,
                     sample_vjp_kernel=sample_vjp_kernel, **kw)


def _path(m):
    return m._flow.lib.nf_sample_vjp_path(m._flow.ptr)


_V = {}


def _wide64(hw, **kw):
    if 64 not in _V:
        _V[64] = sampling_variables(WIDE_ARCH, 64)
    return _flow(WIDE_ARCH, _V[64], hw, 64, **kw)


def _raw_handle(lib, descs, flat, hw, n_layers, flags):
    """nf_create on the current device with `flags` as they are (the keywords refuse some combinations before a handle is made)."""
    from noise_flow_amd import _lib
    cfg = _lib.nf_config(hw[0], hw[1], 4, n_layers, -1, flags)
    h = C.c_void_p()
    _lib.check(lib.nf_create(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, C.byref(h)))
    return h


def _check(m, ref, width, y, eps, g, temp, iso, cam, rows=None):
    """One launch against the reference (`width`: that of the REFERENCE model): the preconditions from the reference alone, then the
    rule and x_out."""
    from noise_flow_amd import _lib
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    assert _path(m) == _lib.NF_SVJP_PATH_GEMM
    rc, x, gy, ge, gt = _call(m, _dev(y) if y is not None else None, _dev(eps), _dev(g), temp, cond=None if rows is not None else _cond(iso, cam), rows=rows)
    _lib.check(rc)
    got = (gy.cpu().numpy() if gy is not None else None, ge.cpu().numpy(), gt.cpu().numpy())
    dist = compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got, log=print)
    print("x: worst masked element %.2e" % close_elem(x.cpu().numpy(), oracle_sample(ref, y, eps, temp, iso, cam), 1e-5))
    return dist


# ---- 1. the rule and x_out on every case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rule(name):
    from noise_flow_amd.noise_flow_model import PatchCond
    key, ref, width, y, eps, g, temp, iso, cam, by_rows = get_case(name)
    arch, v, _, hps, _ = model(key)
    m = _flow(arch, v, eps.shape[1:3], width, **hps)
    rows = m._rows_to_dev(PatchCond(np.array([(i, c, 0, 0) for i, c in TUPLES5], np.float32)), 1) if by_rows else None
    _check(m, ref, width, y, eps, g, temp, iso, cam, rows=rows)


@pytest.mark.parametrize("W", EMBEDDED_WIDTHS)
def test_full_patch_embedded_model(W):
    """The full 32x32 patch at the real widths (4 and 16 bands, 8 couplings): the width-32 deep model embedded in a width-W one, held
    to the width-32 reference."""
    arch, vW, ref, width, y, eps, g, temp, iso, cam = embedded_case(W)
    _check(_flow(arch, vW, (32, 32), W), ref, width, y, eps, g, temp, iso, cam)


# ---- 2. eps = NULL: the bits of the same call fed nf_sample_eps's draw -------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(9, 13), (32, 32)])
def test_philox_eps_is_nf_sample_eps(hw):
    import torch
    from noise_flow_amd import _lib
    m = _wide64(hw)
    assert _path(m) == _lib.NF_SVJP_PATH_GEMM
    B, seed, base = 5, 1234567, 40
    y = _dev(make_inputs(B, hw[0], hw[1], seed=3)[1])
    g = _dev(np.random.RandomState(5).randn(B, hw[0], hw[1], 4).astype(np.float32))
    e = torch.empty_like(g)
    _lib.check(m._flow.lib.nf_sample_eps(seed, base, B, hw[0], hw[1], e.data_ptr(), m._dev.stream_ptr()))
    a = _call(m, y, None, g, 1.0, cond=_cond(), seed=seed, base=base)
    b = _call(m, y, e, g, 1.0, cond=_cond())
    _lib.check(a[0])
    _lib.check(b[0])
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(_bits(u), _bits(v))


# ---- 3. patch independence and the grid-stride loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 8), (32, 32)])
def test_patch_independence_and_grid_stride(hw):
    """B = 2 x CUs + 3 patches cycling through 7 distinct ones: one workgroup per CU, so every workgroup runs the loop more than once, on
    the band, tiles, reduction scratch and gate record the previous patch left behind."""
    import torch
    from noise_flow_amd import _lib
    m = _wide64(hw)
    assert _path(m) == _lib.NF_SVJP_PATH_GEMM
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * n_cu + 3
    y7 = make_inputs(7, hw[0], hw[1], seed=9)[1]
    rng = np.random.RandomState(11)
    e7, g7 = (rng.randn(7, hw[0], hw[1], 4).astype(np.float32) for _ in range(2))
    idx = np.arange(B) % 7
    out = _call(m, _dev(y7[idx]), _dev(e7[idx]), _dev(g7[idx]), 1.0, cond=_cond())
    _lib.check(out[0])
    outs = [_bits(t) for t in out[1:]]
    assert all(np.isfinite(o.view(np.float32)).all() for o in outs)
    for r in range(7):   # every repeat has the bits of the first occurrence
        assert all(np.all(o[r::7] == o[r]) for o in outs), r
    for b in range(7):
        one = _call(m, _dev(y7[b:b + 1]), _dev(e7[b:b + 1]), _dev(g7[b:b + 1]), 1.0, cond=_cond())
        _lib.check(one[0])
        assert all(np.array_equal(_bits(t)[0], o[b]) for t, o in zip(one[1:], outs)), b


# ---- 4. output discipline ------------------------------------------------------------------------------------------------------------
def test_output_discipline():
    import itertools
    import torch
    from noise_flow_amd import _lib
    hw, B = (9, 13), 3
    m = _wide64(hw)
    assert _path(m) == _lib.NF_SVJP_PATH_GEMM
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
    _lib.check(lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 1.0, B, C.byref(cond), None, g.data_ptr(), ptrs[0], ptrs[1],
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
        rc, *outs = _call(m, y, eps, g, 1.0, cond=cond, x=keep[0], gy=keep[1], geps=keep[2], gtemp=keep[3])
        _lib.check(rc)
        for k, o, f in zip(keep, outs, full):
            assert (o is None) == (not k)
            if k:
                assert np.array_equal(_bits(o).reshape(-1), f), keep
    # B = 0 returns 0 and touches nothing
    before = [b.clone() for b in bufs] + [gt.clone()]
    assert lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 1.0, 0, C.byref(cond), None, g.data_ptr(), ptrs[0], ptrs[1], ptrs[2],
                             gt.data_ptr(), st) == 0
    assert lib.nf_sample_vjp(m._flow.ptr, None, None, 0, 0, 1.0, 0, C.byref(cond), None, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs + [gt]))


# ---- 5. the bit changes nothing else ---------------------------------------------------------------------------------------------------
def test_nll_grad_bits_are_those_of_grad_kernel_gemm():
    from noise_flow_amd import _lib
    from test_gpu_nll_grad import _call as nll_call
    hw = (16, 16)
    x, y = (_dev(a) for a in make_inputs(3, hw[0], hw[1], seed=4))
    outs = []
    for kw in ({"sample_vjp_kernel": "gemm"}, {"sample_vjp_kernel": "scalar", "grad_kernel": "gemm"}):
        m = _wide64(hw, **kw)
        assert m._flow.lib.nf_grad_path(m._flow.ptr) == _lib.NF_GRAD_PATH_GEMM
        rc, nll, gx, gy = nll_call(m, x, y, cond=_cond())
        _lib.check(rc)
        outs.append([_bits(t) for t in (nll, gx, gy)])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_width_8_stays_on_the_scalar_kernel():
    """The keyword is refused at width 8 (ValueError), so the bit goes into nf_config.flags directly: the same path, the same bits."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 3
    v = sampling_variables(WIDE_ARCH, 8)
    y, eps, g = (_dev(a) for a in case_inputs(B, hw[0], hw[1], 0))
    m = _flow(WIDE_ARCH, v, hw, 8, sample_vjp_kernel="scalar")
    assert _path(m) == _lib.NF_SVJP_PATH_SCALAR
    rc, *base = _call(m, y, eps, g, 1.0, cond=_cond())
    _lib.check(rc)
    # a second handle of the same model with the bit set
    cfg, descs, flat = m._flow._model_args
    lib = m._flow.lib
    h2 = _raw_handle(lib, descs, flat, hw, cfg.n_layers, cfg.flags | _lib.NF_CFG_SVJP_GEMM)
    try:
        assert lib.nf_sample_vjp_path(h2) == _lib.NF_SVJP_PATH_SCALAR
        outs = [torch.empty_like(g) for _ in range(3)] + [torch.empty((B,), device="cuda")]
        cond = _cond()
        _lib.check(lib.nf_sample_vjp(h2, y.data_ptr(), eps.data_ptr(), 0, 0, 1.0, B, C.byref(cond), None, g.data_ptr(), outs[0].data_ptr(),
                                     outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), m._dev.stream_ptr()))
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(base, outs))
    finally:
        lib.nf_destroy(h2)


def test_width_32_with_the_matrix_core_bit_keeps_its_path():
    """NF_CFG_SVJP_MFMA at width 32 on 32x32, with and without the new bit in nf_config.flags: NF_SVJP_PATH_WIDE32 and the same bits."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (32, 32), 2
    m = _flow(WIDE_ARCH, sampling_variables(WIDE_ARCH, 32), hw, 32, sample_vjp_kernel="mfma")
    assert _path(m) == _lib.NF_SVJP_PATH_WIDE32
    y, eps, g = (_dev(a) for a in case_inputs(B, hw[0], hw[1], 0))
    rc, *base = _call(m, y, eps, g, 1.0, cond=_cond())
    _lib.check(rc)
    cfg, descs, flat = m._flow._model_args
    lib = m._flow.lib
    h2 = _raw_handle(lib, descs, flat, hw, cfg.n_layers, cfg.flags | _lib.NF_CFG_SVJP_GEMM)
    try:
        assert lib.nf_sample_vjp_path(h2) == _lib.NF_SVJP_PATH_WIDE32 and lib.nf_grad_path(h2) == lib.nf_grad_path(m._flow.ptr)
        outs = [torch.empty_like(g) for _ in range(3)] + [torch.empty((B,), device="cuda")]
        cond = _cond()
        _lib.check(lib.nf_sample_vjp(h2, y.data_ptr(), eps.data_ptr(), 0, 0, 1.0, B, C.byref(cond), None, g.data_ptr(), outs[0].data_ptr(),
                                     outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), m._dev.stream_ptr()))
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(base, outs))
    finally:
        lib.nf_destroy(h2)


# ---- 6. workspace --------------------------------------------------------------------------------------------------------------------
def test_workspace():
    """The gate record is the only scratch: what nf_nll_grad needs on the same handle and B.  16 x 16 at width 64: one band, two
    couplings' records of 8 KiB per launched workgroup."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 5
    y, eps, g = (_dev(a) for a in case_inputs(B, hw[0], hw[1], 1))
    outs = []
    for reserve in (False, True):
        m = _wide64(hw)
        lib, h = m._flow.lib, m._flow.ptr
        assert _path(m) == _lib.NF_SVJP_PATH_GEMM
        n_cpl = 3                                    # WIDE_ARCH
        for b in (1, B, 100000):
            need = lib.nf_workspace_bytes(h, 3, b)
            groups = min(b, torch.cuda.get_device_properties(0).multi_processor_count)
            assert need == lib.nf_workspace_bytes(h, 2, b) and need > 0
            assert need == (groups * n_cpl * 1 * 4096 * 2 + 255) // 256 * 256, (b, need)
        assert lib.nf_workspace_bytes(h, 3, 0) == 0
        if reserve:
            _lib.check(lib.nf_reserve_sample_vjp_workspace(h, B, 2))
        rc, *o = _call(m, y, eps, g, 1.0, cond=_cond())
        _lib.check(rc)
        outs.append([_bits(t) for t in o])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    # a handle of the scalar path keeps its 0
    m8 = _flow(WIDE_ARCH, sampling_variables(WIDE_ARCH, 8), hw, 8, sample_vjp_kernel="scalar")
    assert m8._flow.lib.nf_workspace_bytes(m8._flow.ptr, 3, B) == 0


# ---- 7. refusals through nf_sample_vjp itself launch nothing -------------------------------------------------------------------------------
def test_refusals():
    """Handles made through nf_create with the flags as they are: 33x32; 65x64 with NF_CFG_GRAD_TILED_GEMM; fp16; 33 bare couplings
    sharing one parameter block (the architecture grammar cannot exceed 32: tests/test_grad_gemm_cpu.py)."""
    import torch
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    bit, cond = _lib.NF_CFG_SVJP_GEMM, _cond()
    layers, descs, flat = params.pack(WIDE_ARCH, sampling_variables(WIDE_ARCH, 64), 64, "loss_first")
    _, d1, f1 = params.pack("unc", sampling_variables("unc", 64), 64, "loss_first")
    cpl = [d for d in d1 if d.width == 64][0]
    many = (_lib.nf_layer_desc * 33)(*[_lib.nf_layer_desc(cpl.type, cpl.width, cpl.param_offset) for _ in range(33)])
    st = int(torch.cuda.current_stream().cuda_stream)
    for ds, fl, n, hw, flags, word in ((descs, flat, len(layers), (33, 32), bit, "no tile mode"),
                                       (descs, flat, len(layers), (65, 64), bit | _lib.NF_CFG_GRAD_TILED_GEMM, "no tile mode"),
                                       (descs, flat, len(layers), (16, 16), bit | _lib.NF_CFG_FP16_CNN, "fp32 handles only"),
                                       (many, f1, 33, (8, 8), bit, "at most 32 couplings")):
        h = _raw_handle(lib, ds, fl, hw, n, flags)
        try:
            y, eps = (_dev(a) for a in make_inputs(2, hw[0], hw[1]))
            out = torch.zeros_like(eps)
            rc = lib.nf_sample_vjp(h, y.data_ptr() if ds is descs else None, eps.data_ptr(), 0, 0, 1.0, 2, C.byref(cond), None, eps.data_ptr(), None, None,
                                   out.data_ptr(), None, st)
            torch.cuda.synchronize()
            msg = (lib.nf_last_error() or b"").decode()
            assert rc == _lib.NF_EINVAL and msg.startswith("nf_sample_vjp") and word in msg, (hw, flags, rc, msg)
            assert not out.any()   # no launch
            assert lib.nf_sample_vjp_path(h) == _lib.NF_EINVAL
        finally:
            lib.nf_destroy(h)


# ---- 8. sample_and_vjp and sample_torch ------------------------------------------------------------------------------------------------
def test_sample_torch():
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 4
    m = _wide64(hw)
    assert _path(m) == _lib.NF_SVJP_PATH_GEMM
    y = make_inputs(B, hw[0], hw[1], seed=2)[1]
    rng = np.random.RandomState(3)
    eps, g = (rng.randn(B, hw[0], hw[1], 4).astype(np.float32) for _ in range(2))
    iso, cam = [100.0, 400.0, 800.0, 1600.0], [0.0, 1.0, 2.0, 3.0]
    x0, gy0, ge0, gt0 = m.sample_and_vjp(_dev(y), _dev(g), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=_dev(eps))
    close_elem(x0.cpu().numpy(), m.sample(_dev(y), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=_dev(eps)).cpu().numpy(), 1e-5)
    # autograd: the backward pass's bits are the direct call's
    yt, et = _dev(y).requires_grad_(True), _dev(eps).requires_grad_(True)
    std = torch.tensor(0.6, device="cuda", requires_grad=True)
    x = m.sample_torch(yt, eps=et, eps_std=std, iso=iso, cam=cam)
    assert x.requires_grad
    (x * _dev(g)).sum().backward()
    assert torch.equal(yt.grad, gy0) and torch.equal(et.grad, ge0) and torch.equal(std.grad, gt0.sum())
    # the in-kernel draw under a seed is the one sample() makes, and its gradient the direct call's on that draw
    m2 = _wide64(hw)
    y2 = _dev(y).requires_grad_(True)
    x2 = m2.sample_torch(y2, seed=77, eps_std=0.6, iso=iso, cam=cam)
    (x2 * _dev(g)).sum().backward()
    e77 = torch.empty_like(x2)
    _lib.check(m2._flow.lib.nf_sample_eps(77, 0, B, hw[0], hw[1], e77.data_ptr(), m2._dev.stream_ptr()))
    assert torch.equal(x2.detach(), m2.sample(_dev(y), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=e77))
    _, gy77, _, _ = m2.sample_and_vjp(_dev(y), _dev(g), eps_std=0.6, yy=_dev(y), iso=iso, cam=cam, eps=e77)
    assert torch.equal(y2.grad, gy77)
    # nll_torch works on the same model: one gradient block serves both calls
    assert m._flow.lib.nf_grad_path(m._flow.ptr) == _lib.NF_GRAD_PATH_GEMM
    # the keyword is validated by NoiseFlow too, and hps.sample_vjp_kernel selects it
    from noise_flow_amd import NoiseFlow, default_hps
    with pytest.raises(ValueError):
        NoiseFlow([16, 16, 4], False, default_hps(arch=WIDE_ARCH, width=64), variables=_V[64], cnn_dtype="fp16", sample_vjp_kernel="gemm")
    hp = default_hps(arch=WIDE_ARCH, width=64)
    hp.sample_vjp_kernel = "gemm"
    assert _path(NoiseFlow([16, 16, 4], False, hp, variables=_V[64])) == _lib.NF_SVJP_PATH_GEMM
