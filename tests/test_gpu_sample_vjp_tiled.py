"""nf_sample_vjp beyond the shapes held whole (NF_CFG_SVJP_TILED, ``sample_vjp_tiles=True``): tiles and segments of nf_nll_grad's plan
on nf_sample_grad_kernel<.., TILED>.

The rule, its weights, preconditions and kink handling are those of tests/sample_vjp_ref.py (constants of tests/nll_grad_ref.py), the
reference is whole-image autograd in fp64; x_out is held to ``NoiseFlowOracle.sample`` by conftest.close_elem at 1e-5.  The CPU tier
(tests/test_sample_vjp_tiles_cpu.py) runs the same call sequence on the reference.  Every case meets ``reference_conditions`` (seed 0,
ISO 800 / cam 2 unless said): on-kink activations per image and the largest pinned e32 —
  shipped (65,64) [3,3] 2.2e-6   (64,65) [5,3] 1.5e-6   (96,80) [4,5] 1.4e-6      width 8 (64,64) [5,2] 3.3e-7   (56,56) [2,2] 6.1e-7
  width 16 (40,33) [1,4] 5.3e-7   width 4 (70,20) [0,0] 3.0e-7   vocabulary model (70,36), ISO 1600 / cam 3 [0,0,0] 3.2e-7, per-image rows
  [1,0,0] 3.2e-7   unc|gain4|unc (66,12) [0,0] 4.5e-7.
Measured distances are printed (run with -s).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, SHIPPED_DIR, close_elem, make_inputs
from sample_vjp_ref import (CAM, ISO, SHIPPED_TEMP, TUPLES5, SampleVjpRef, case_inputs, case_model, compare_with_kink_rule, oracle_sample,
                            reference_conditions)
from test_gpu_sample_vjp import _bits, _call, _cond, _dev, _flow

pytestmark = pytest.mark.gpu


def _tiled(arch, variables, hw, width=4, **kw):
    return _flow(arch, variables, hw, width, sample_vjp_tiles=True, **kw)


def _path(m):
    return m._flow.lib.nf_sample_vjp_path(m._flow.ptr)


def _segments(m):
    cfg, descs, flat = m._flow._model_args
    out = (C.c_int32 * 80)()
    n = m._flow.lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, out, 16)
    return n, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))]


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------------------
# (model of sample_vjp_ref.case_model, (H, W), B, temperature, iso, cam, per-image rows)
RULE_CASES = [
    (("shipped", None), (65, 64), 2, SHIPPED_TEMP, ISO, CAM, False),
    (("shipped", None), (64, 65), 2, SHIPPED_TEMP, ISO, CAM, False),
    (("shipped", None), (96, 80), 2, SHIPPED_TEMP, ISO, CAM, False),
    (("width", 8), (64, 64), 2, 1.0, ISO, CAM, False),
    (("width", 8), (56, 56), 2, 1.0, ISO, CAM, False),
    (("width", 16), (40, 33), 2, 1.0, ISO, CAM, False),
    (("width", 4), (70, 20), 2, 1.0, ISO, CAM, False),
    (("vocab", {}), (70, 36), 3, 1.0, 1600.0, 3.0, False),
    (("vocab", {}), (70, 36), 3, 1.0, np.array([t[0] for t in TUPLES5[:3]], np.float64), np.array([t[1] for t in TUPLES5[:3]], np.float64), True),
    (("nosdn",), (66, 12), 2, 1.0, None, None, False),
]
_REFS = {}


def _case(shipped_variables, name, hw, B, temp, iso, cam):
    """→ (arch, variables, width, hps, ref, y, eps, g): the reference and the inputs are made once per model / shape."""
    arch, v, width, hps = case_model(name, shipped_variables)
    key = (repr(name), hw, B)
    if key not in _REFS:
        y, eps, g = case_inputs(B, hw[0], hw[1], 0)
        _REFS[key] = (SampleVjpRef(arch, v, **hps), None if name[0] == "nosdn" else y, eps, g)
    return (arch, v, width, hps) + _REFS[key]


def _rule(m, ref, width, y, eps, g, temp, iso, cam, rows=False):
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    assert _path(m) == _lib.NF_SVJP_PATH_TILED
    rd = m._rows_to_dev(PatchCond(np.array([(i, c, 0, 0) for i, c in zip(iso, cam)], np.float32)), 1) if rows else None
    rc, x, gy, ge, gt = _call(m, _dev(y) if y is not None else None, _dev(eps), _dev(g), temp, cond=None if rows else _cond(iso, cam), rows=rd)
    _lib.check(rc)
    got = (gy.cpu().numpy() if gy is not None else None, ge.cpu().numpy(), gt.cpu().numpy())
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got, log=print)
    print("x: worst masked element %.2e" % close_elem(x.cpu().numpy(), oracle_sample(ref, y, eps, temp, iso, cam), 1e-5))


@pytest.mark.parametrize("name,hw,B,temp,iso,cam,rows", RULE_CASES, ids=lambda v: repr(v) if not isinstance(v, np.ndarray) else "rows")
def test_rule(monkeypatch, shipped_variables, name, hw, B, temp, iso, cam, rows):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    arch, v, width, hps, ref, y, eps, g = _case(shipped_variables, name, hw, B, temp, iso, cam)
    _rule(_tiled(arch, v, hw, width, **hps), ref, width, y, eps, g, temp, iso, cam, rows)


# ---- 2. forced plans --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced,halos", [(8, [4] * 8), (4, [8] * 4), (3, [12, 12, 8])])
def test_forced_plans(monkeypatch, shipped_variables, forced, halos):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    arch, v, width, hps, ref, y, eps, g = _case(shipped_variables, ("shipped", None), (96, 80), 2, SHIPPED_TEMP, ISO, CAM)
    m = _tiled(arch, v, (96, 80))
    n, segs = _segments(m)
    assert n == forced and [s[2] for s in segs] == halos, segs
    _rule(m, ref, width, y, eps, g, SHIPPED_TEMP, ISO, CAM)


def test_infeasible_forced_plan_is_refused_before_anything_is_written(monkeypatch, shipped_variables):
    import torch
    from noise_flow_amd import _lib
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")
    m = _tiled(FULL_ARCH, shipped_variables, (96, 80))
    y, eps, g = (_dev(a) for a in case_inputs(2, 96, 80, 0))
    outs = [torch.full_like(g, 1234.5) for _ in range(3)] + [torch.full((2,), 1234.5, device="cuda")]
    rc = m._flow.lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 0.6, 2, C.byref(_cond()), None, g.data_ptr(),
                                   outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.NF_EINVAL and b"segments" in m._flow.lib.nf_last_error()
    assert all(bool((o == 1234.5).all()) for o in outs)


# ---- 3. eps = NULL ------------------------------------------------------------------------------------------------------------------------
def test_philox_eps_is_nf_sample_eps(monkeypatch, shipped_variables):
    """Every output has the bits of the same call fed nf_sample_eps's draw (the regenerated draw is keyed by image index and image pixel);
    x is nf_sample's own sample of that draw to the tensor tolerance."""
    import torch
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    hw, B, seed, base = (65, 64), 3, 1234567, 40
    m = _tiled(FULL_ARCH, shipped_variables, hw)
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
    xs = m.sample(y, eps_std=0.6, yy=y, iso=[ISO], cam=[CAM], eps=e)
    close_elem(a[1].cpu().numpy(), xs.cpu().numpy(), 1e-5)
    print("x_out bit-equal to nf_sample of the same draw: %s" % bool(torch.equal(a[1], xs)))


# ---- 4. image independence and the persistent grid ---------------------------------------------------------------------------------------
def test_image_independence_and_grid_stride(monkeypatch, shipped_variables):
    """B x tiles > 8 x CUs: every workgroup of the persistent grid walks several tiles of several images, on LDS tiles, gate words,
    reduction scratch and per-tile geometry the previous tile left behind.  Images cycle through 7 distinct ones: every repeat has
    the bits of the first occurrence, and a second call the bits of the first (gtemp included: no atomics)."""
    import torch
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    hw = (65, 64)
    m = _tiled(FULL_ARCH, shipped_variables, hw)
    n, segs = _segments(m)
    tiles = min(s[3] * s[4] for s in segs)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * n_cu // tiles + 3
    assert B * tiles > 8 * n_cu
    y7 = make_inputs(7, hw[0], hw[1], seed=9)[1]
    rng = np.random.RandomState(11)
    e7, g7 = (rng.randn(7, hw[0], hw[1], 4).astype(np.float32) for _ in range(2))
    idx = np.arange(B) % 7
    yd, ed, gd = _dev(y7[idx]), _dev(e7[idx]), _dev(g7[idx])
    out = _call(m, yd, ed, gd, 0.6, cond=_cond())
    _lib.check(out[0])
    outs = [_bits(t) for t in out[1:]]
    assert all(np.isfinite(o.view(np.float32)).all() for o in outs)
    for r in range(7):
        assert all(np.all(o[r::7] == o[r]) for o in outs), r
    again = _call(m, yd, ed, gd, 0.6, cond=_cond())
    _lib.check(again[0])
    assert all(np.array_equal(_bits(t), o) for t, o in zip(again[1:], outs))


# ---- 5. output discipline ------------------------------------------------------------------------------------------------------------------
def test_output_discipline(monkeypatch, shipped_variables):
    import torch
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    hw, B = (70, 33), 2
    m = _tiled(FULL_ARCH, shipped_variables, hw)
    assert _path(m) == _lib.NF_SVJP_PATH_TILED
    y = _dev(make_inputs(B, hw[0], hw[1], seed=1)[1])
    rng = np.random.RandomState(2)
    eps, g = (_dev(rng.randn(B, hw[0], hw[1], 4).astype(np.float32)) for _ in range(2))
    n, band = g.numel(), 1024                        # 4 KiB of floats on both sides
    sentinel = 1234.5
    lib, st = m._flow.lib, m._dev.stream_ptr()
    cond = _cond()

    def run(keep):
        """One call into sentinel-filled buffers with guard bands → the four outputs' bits (None where not asked)."""
        bufs = [torch.full((n + 2 * band,), sentinel, device="cuda") for _ in range(3)]
        gt = torch.full((B + 2,), sentinel, device="cuda")
        ptrs = [b.data_ptr() + 4 * band if k else None for b, k in zip(bufs, keep[:3])]
        _lib.check(lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 0.6, B, C.byref(cond), None, g.data_ptr(), ptrs[0], ptrs[1],
                                     ptrs[2], gt.data_ptr() + 4 if keep[3] else None, st))
        res = []
        for b, k in zip(bufs, keep[:3]):
            h = b.cpu().numpy()
            assert np.all(h[:band] == sentinel) and np.all(h[-band:] == sentinel)
            if k:   # every pixel is in exactly one core
                assert np.isfinite(h).all() and not np.any(h[band:-band] == sentinel)
            else:   # an output that was not asked for keeps the sentinel
                assert np.all(h == sentinel)
            res.append(_bits(b[band:-band]) if k else None)
        hn = gt.cpu().numpy()
        assert hn[0] == sentinel and hn[-1] == sentinel
        assert (np.isfinite(hn).all() and not np.any(hn[1:-1] == sentinel)) if keep[3] else np.all(hn == sentinel)
        res.append(_bits(gt[1:-1]) if keep[3] else None)
        return res

    full = run((True, True, True, True))
    for keep in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (False, True, True, True)):      # each output alone; x_out = NULL: the call sample_torch's backward pass makes
        got = run(keep)
        for k, o, f in zip(keep, got, full):
            assert (o is None) == (not k)
            if k:
                assert np.array_equal(o, f), keep
    # gy_out with y = NULL is refused and nothing is launched
    gy = torch.full_like(g, sentinel)
    rc = lib.nf_sample_vjp(m._flow.ptr, None, eps.data_ptr(), 0, 0, 0.6, B, C.byref(cond), None, g.data_ptr(), None, gy.data_ptr(), None, None, st)
    torch.cuda.synchronize()
    assert rc == _lib.NF_EINVAL and lib.nf_last_error() and bool((gy == sentinel).all())


# ---- 6. workspace --------------------------------------------------------------------------------------------------------------------------
def test_workspace_is_owned_by_the_handle_and_reservable(monkeypatch, shipped_variables):
    """As tests/test_gpu_nll_grad_tiled.py: nf_workspace_bytes(h, 3, B) says what a tiled nf_sample_vjp call needs — (segments - 1)
    kept tensors, 2 gradient tensors, the tile sums —, nf_reserve_sample_vjp_workspace sets it aside, and calls after that run with the
    device's free memory unchanged."""
    import torch
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    hw, B = (96, 80), 3
    small = _tiled(FULL_ARCH, shipped_variables, (32, 32))
    assert small._flow.lib.nf_workspace_bytes(small._flow.ptr, 3, 1024) == 0
    _lib.check(small._flow.lib.nf_reserve_sample_vjp_workspace(small._flow.ptr, 16, 2))          # nothing to do
    plain = _flow(FULL_ARCH, shipped_variables, hw, grad_tiles=True)
    assert plain._flow.lib.nf_workspace_bytes(plain._flow.ptr, 3, B) == 0
    m = _tiled(FULL_ARCH, shipped_variables, hw)
    lib = m._flow.lib
    n, segs = _segments(m)
    assert n == 8
    need = lib.nf_workspace_bytes(m._flow.ptr, 3, B)
    img = B * hw[0] * hw[1] * 16
    assert (7 + 2) * img < need <= (7 + 2) * (img + 256) + B * segs[-1][3] * segs[-1][4] * 4 + 256
    _lib.check(lib.nf_reserve_sample_vjp_workspace(m._flow.ptr, B, 2))
    y, eps, g = (_dev(a) for a in case_inputs(B, hw[0], hw[1], 4))
    cond = _cond()
    # outputs allocated up front, so that torch's caching allocator is out of the measurement
    outs = [(torch.empty_like(g), torch.empty_like(g), torch.empty_like(g), torch.empty((B,), device="cuda")) for _ in range(7)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]

    def call(o, stream):
        _lib.check(lib.nf_sample_vjp(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 0.6, B, C.byref(cond), None, g.data_ptr(), o[0].data_ptr(),
                                     o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), stream))

    for o in outs[:3]:
        call(o, m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    # two streams on one handle, calls in flight on both: each has a buffer of its own, the bits are those of the serial calls
    for i, o in enumerate(outs[3:]):
        call(o, streams[i & 1].cuda_stream)
    torch.cuda.synchronize()
    assert all(np.isfinite(t.cpu().numpy()).all() for t in outs[0])
    for o in outs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(o, outs[0]))
    with pytest.raises(Exception):
        _lib.check(lib.nf_reserve_sample_vjp_workspace(m._flow.ptr, B, 0))


# ---- 7. nothing else moves -------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(monkeypatch, shipped_variables):
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    # nf_nll_grad on a handle with the flag: the bits of a grad_tiles=True handle
    x, y = make_inputs(2, 65, 64, seed=3)
    a = _tiled(FULL_ARCH, shipped_variables, (65, 64)).nll_and_grad(x, y, iso=[ISO], cam=[CAM])
    b = _flow(FULL_ARCH, shipped_variables, (65, 64), grad_tiles=True).nll_and_grad(x, y, iso=[ISO], cam=[CAM])
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # nf_sample_vjp at 32x32: the whole-patch kernel, the bits of a handle without any flag
    y, eps, g = case_inputs(3, 32, 32, 0)
    m1, m0 = _tiled(FULL_ARCH, shipped_variables, (32, 32)), _flow(FULL_ARCH, shipped_variables, (32, 32))
    assert _path(m1) == _lib.NF_SVJP_PATH_SCALAR
    a = m1.sample_and_vjp(y, g, eps_std=0.6, yy=y, iso=[ISO], cam=[CAM], eps=eps)
    b = m0.sample_and_vjp(y, g, eps_std=0.6, yy=y, iso=[ISO], cam=[CAM], eps=eps)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # grad_tiles=True alone keeps refusing
    y, eps, g = case_inputs(1, 65, 65, 0)
    with pytest.raises(_lib.NoiseFlowLibError, match="no tile mode"):
        _flow(FULL_ARCH, shipped_variables, (65, 65), grad_tiles=True).sample_and_vjp(y, g, yy=y, iso=[ISO], cam=[CAM], eps=eps)


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------------------
def test_python_surface(monkeypatch, shipped_variables):
    import torch
    from noise_flow_amd import NoiseFlow, NoiseFlowWrapper, _lib, default_hps
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    hw, B = (65, 64), 2
    m = _tiled(FULL_ARCH, shipped_variables, hw)
    y, eps, g = case_inputs(B, hw[0], hw[1], 0)
    x0, gy0, ge0, gt0 = m.sample_and_vjp(_dev(y), _dev(g), eps_std=0.6, yy=_dev(y), iso=[ISO], cam=[CAM], eps=_dev(eps))
    clean, et = _dev(y).requires_grad_(True), _dev(eps).requires_grad_(True)
    std = torch.tensor(0.6, device="cuda", requires_grad=True)
    x = m.sample_torch(clean, eps=et, eps_std=std, iso=[ISO], cam=[CAM])
    assert x.requires_grad
    (x * _dev(g)).sum().backward()
    assert torch.equal(clean.grad, gy0) and torch.equal(et.grad, ge0) and torch.equal(std.grad, gt0.sum())
    # hps.sample_vjp_tiles is the same switch
    hp = default_hps(arch=FULL_ARCH, width=4)
    hp.sample_vjp_tiles = True
    assert _path(NoiseFlow([65, 65, 4], False, hp, variables=shipped_variables)) == _lib.NF_SVJP_PATH_TILED
    # the wrapper on crops: numpy in, numpy out
    nf = NoiseFlowWrapper(SHIPPED_DIR, patch_shape=(96, 80), sample_vjp_tiles=True)
    assert _path(nf.nf_model) == _lib.NF_SVJP_PATH_TILED
    y, eps, g = case_inputs(2, 96, 80, 0)
    out = nf.nf_model.sample_and_vjp(y, g, eps_std=0.6, yy=y, iso=[ISO], cam=[CAM], eps=eps)
    assert all(isinstance(a, np.ndarray) for a in out)
    assert out[0].shape == y.shape and out[1].shape == y.shape and out[2].shape == y.shape and out[3].shape == (2,)
    assert all(np.isfinite(a).all() for a in out)
