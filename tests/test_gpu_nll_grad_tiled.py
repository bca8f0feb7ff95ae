"""nf_nll_grad beyond what one workgroup holds (NF_CFG_GRAD_TILED): the tiled, segmented gradient of whole images.

The rules are those of tests/test_gpu_nll_grad.py, unchanged: per image and tensor max|kernel - ref64| <= tol * max|ref64| with
tol = max(1e-5, 4 * e32) (``compare_with_kink_rule``), nll_out to the fp64 oracle at NLL_RTOL = 1e-5, and at most 6 on-kink
activations per image, asserted from the reference before the kernel's output is looked at.  Input seeds are the first from 0
upward that meet the kink condition on the CPU reference (seed 0 in every case; counts per image in the comments).  A halo that
is one pixel short shows at fp32 resolution only when a segment holds ONE coupling (1.2e-3; tests/test_grad_tiles_cpu.py pins the
deeper segments in fp64): the S = 8 cases of the shipped model are the ones that catch a core / halo slip.

Both norms of tests/nll_grad_ref.py are enforced (raw and whitened; the reference is the shared pinned one), and every case first
asserts from the reference alone that the pinned e32 is at most E32_MAX = 5e-6 in both norms; (65,64) and (96,80) also assert
max / median |gy| >= 100.  Measured on an MI355X, worst image of all cases, raw / whitened: gx 2.6e-6 / 3.1e-6, gy 4.9e-6 / 3.3e-6
(the 80x72 image of test_python_surface: 0.49 of the bound).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables
from nll_grad_ref import PinnedRef, compare_with_kink_rule, reference_conditions
from test_gpu_nll_grad import GY_RANGE, ISO, CAM, NLL_RTOL, TUPLES5, VOCAB_ARCH, WIDE_ARCH, _bits, _call, _check, _cond, _dev, _vocab_variables

pytestmark = pytest.mark.gpu

NO_SDN_ARCH = "unc|gain4|unc"


def _flow(arch, variables, hw, width=4, grad_tiles=True, **kw):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width), variables=variables, grad_tiles=grad_tiles, **kw)


def _path(m):
    return m._flow.lib.nf_grad_path(m._flow.ptr)


def _segments(m):
    """nf_grad_tile_segments of the model's handle arguments (host arithmetic, reads NF_GRAD_TILE_SEGMENTS as nf_create did)."""
    cfg, descs, flat = m._flow._model_args
    out = (C.c_int32 * 80)()
    n = m._flow.lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, out, 16)
    return n, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))]


@pytest.fixture(scope="module")
def shipped_ref(shipped_variables):
    return PinnedRef(FULL_ARCH, shipped_variables)


@pytest.fixture(autouse=True)
def _no_forced_count(monkeypatch):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)


# ---- 1. the shipped model -------------------------------------------------------------------------------------------------------
# on-kink activations per image (seed 0): (65,64) [3,4]  (64,65) [2,2]  (96,80) [4,5]  (120,66) [3,6]
# largest pinned e32 over images, tensors and both norms: 2.0e-6  2.7e-6  1.9e-6  2.2e-6; max / median |gy| of (65,64) 1903, of (96,80) 3969
SHIPPED_CASES = [(65, 64), (64, 65), (96, 80), (120, 66)]
GY_RANGE_CASES = ((65, 64), (96, 80))             # max / median |gy| >= GY_RANGE, asserted from the reference
TRAINED_CASES = [(8, (64, 64), 0), (16, (40, 33), 0), (4, (70, 20), 0), (8, (56, 56), 0)]


@pytest.mark.parametrize("hw", SHIPPED_CASES)
def test_shipped_model(shipped_variables, shipped_ref, hw):
    from noise_flow_amd import _lib
    m = _flow(FULL_ARCH, shipped_variables, hw)
    assert _path(m) == _lib.NF_GRAD_PATH_TILED and _segments(m)[0] >= 3      # at most 3 couplings per segment
    x, y = make_inputs(2, hw[0], hw[1], seed=0)
    _check(m, shipped_ref, 4, x, y, ISO, CAM, min_gy_range=GY_RANGE if hw in GY_RANGE_CASES else None)


@pytest.mark.parametrize("forced,halos", [(8, [4] * 8), (4, [8] * 4), (3, [12, 12, 8])])
def test_forced_segment_counts(monkeypatch, shipped_variables, shipped_ref, forced, halos):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    m = _flow(FULL_ARCH, shipped_variables, (96, 80))
    n, segs = _segments(m)
    assert n == forced and [s[2] for s in segs] == halos
    x, y = make_inputs(2, 96, 80, seed=0)
    _check(m, shipped_ref, 4, x, y, ISO, CAM)


def test_infeasible_forced_count_is_refused(monkeypatch, shipped_variables):
    import torch
    from noise_flow_amd import _lib
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")          # 4 couplings per segment: halo 16, no core in a 32-pixel tile
    m = _flow(FULL_ARCH, shipped_variables, (96, 80))
    x, y = (_dev(a) for a in make_inputs(1, 96, 80))
    gx = torch.zeros_like(x)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, x.data_ptr(), y.data_ptr(), 1, C.byref(_cond()), None, None, gx.data_ptr(), None, m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.NF_EINVAL and b"segments" in m._flow.lib.nf_last_error() and not gx.any()
    nll, _ = m._loss(x, y, [0], [0], [ISO], [CAM])             # the forward direction is not touched by the switch
    assert np.isfinite(nll.cpu().numpy()).all()


# ---- 2. widths 4 / 8 / 16 ---------------------------------------------------------------------------------------------------------
# on-kink per image (seed 0): width 8 (64,64) [1,1]   width 16 (40,33) [1,1]   width 4 (70,20) [0,1]   width 8 (56,56) [0,2]
# largest pinned e32: 2.7e-7  1.1e-6  3.2e-7  3.2e-7
# (56x56 at width 8 is the smallest square the whole-patch kernel's LDS does not hold; its forward launches are the scalar-weight
#  kernel's, those of 64x64 the width-32 matrix-core kernel's, those of width 16 the width-16 kernel's, of width 4 the MFMA4 one's)
@pytest.mark.parametrize("width,hw,seed", TRAINED_CASES)
def test_trained_like_widths(width, hw, seed):
    from noise_flow_amd import _lib
    v = trained_like_variables(WIDE_ARCH, width)
    m = _flow(WIDE_ARCH, v, hw, width)
    assert _path(m) == _lib.NF_GRAD_PATH_TILED
    x, y = make_inputs(2, hw[0], hw[1], seed=seed)
    _check(m, PinnedRef(WIDE_ARCH, v), width, x, y, ISO, CAM)


# ---- 3. vocabulary and conditioning: the trailing sdn3 makes gy come from two segments -------------------------------------------------
# on-kink per image (seed 0): per-call cond [0,1,1], per-image rows [0,0,0]; largest pinned e32 1.4e-6, 1.3e-6
def test_vocabulary_per_call_cond(monkeypatch):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")      # sdn5 in the first segment, sdn3 in the second, whatever the cost model says
    v = _vocab_variables()
    m = _flow(VOCAB_ARCH, v, (70, 36))
    assert _segments(m)[0] == 2
    x, y = make_inputs(3, 70, 36, seed=0)
    _check(m, PinnedRef(VOCAB_ARCH, v), 4, x, y, 1600.0, 3.0)


def test_vocabulary_per_image_rows(monkeypatch):
    from noise_flow_amd.noise_flow_model import PatchCond
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")
    v = _vocab_variables()
    m = _flow(VOCAB_ARCH, v, (70, 36))
    x, y = make_inputs(3, 70, 36, seed=0)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5[:3]], np.float32)
    rows = m._rows_to_dev(PatchCond(table), 0)
    _check(m, PinnedRef(VOCAB_ARCH, v), 4, x, y, table[:, 0], table[:, 1], rows=rows)


# ---- 4. a model without an SDN layer: y = NULL ---------------------------------------------------------------------------------------
def test_model_without_sdn():
    import torch
    from noise_flow_amd import _lib
    v = trained_like_variables(NO_SDN_ARCH, 4, seed=3)
    m = _flow(NO_SDN_ARCH, v, (66, 12))
    assert _path(m) == _lib.NF_GRAD_PATH_TILED
    x = np.random.RandomState(0).randn(2, 66, 12, 4).astype(np.float32)     # on-kink per image: [0, 0], pinned e32 1.8e-7
    _check(m, PinnedRef(NO_SDN_ARCH, v), 4, x, None, None, None)
    xd = _dev(x)
    gy = torch.empty_like(xd)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), None, 2, C.byref(_cond()), None, None, None, gy.data_ptr(), m._dev.stream_ptr())
    assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error()


# ---- 5. image independence and the persistent grid -------------------------------------------------------------------------------------
def test_image_independence_and_grid_stride(shipped_variables):
    """B x tiles > 8 x CUs, so every workgroup of the persistent grid (at most 2 resident per CU at 32x32 tiles) walks several tiles,
    of several images — on LDS tiles, gate words and per-tile geometry the previous tile left behind.  Images cycle through 3
    distinct ones: every repeat and every single-image call has the same bits."""
    import torch
    from noise_flow_amd import _lib
    hw = (96, 80)
    m = _flow(FULL_ARCH, shipped_variables, hw)
    n, segs = _segments(m)
    tiles = min(s[3] * s[4] for s in segs)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * n_cu // tiles + 3
    assert B * tiles > 8 * n_cu
    x3, y3 = make_inputs(3, hw[0], hw[1], seed=9)
    idx = np.arange(B) % 3
    rc, nll, gx, gy = _call(m, _dev(x3[idx]), _dev(y3[idx]), cond=_cond())
    _lib.check(rc)
    nll, gx, gy = _bits(nll), _bits(gx), _bits(gy)
    assert all(np.isfinite(a.view(np.float32)).all() for a in (nll, gx, gy))
    for r in range(3):
        assert np.all(nll[r::3] == nll[r]) and np.all(gx[r::3] == gx[r]) and np.all(gy[r::3] == gy[r]), r
    for b in range(3):
        rc, n1, gx1, gy1 = _call(m, _dev(x3[b:b + 1]), _dev(y3[b:b + 1]), cond=_cond())
        _lib.check(rc)
        assert _bits(n1)[0] == nll[b] and np.array_equal(_bits(gx1)[0], gx[b]) and np.array_equal(_bits(gy1)[0], gy[b]), b


# ---- 6. output discipline -------------------------------------------------------------------------------------------------------------
def test_output_discipline(shipped_variables):
    import torch
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond
    hw, B = (70, 33), 2
    m = _flow(FULL_ARCH, shipped_variables, hw)
    x, y = make_inputs(B, hw[0], hw[1], seed=1)
    xd, yd = _dev(x), _dev(y)
    n, band = xd.numel(), 1024
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
        assert np.isfinite(h).all() and not np.any(h[band:-band] == sentinel)      # every pixel is in exactly one core
    hn = nll.cpu().numpy()
    assert hn[0] == sentinel and hn[-1] == sentinel and not np.any(hn[1:-1] == sentinel)
    full = (_bits(nll[1:-1]), _bits(bufs[0][band:-band]), _bits(bufs[1][band:-band]))
    # any subset of the outputs: the ones asked for keep their bits
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        rc, *outs = _call(m, xd, yd, cond=cond, nll=bool(want[0]), gx=bool(want[1]), gy=bool(want[2]))
        _lib.check(rc)
        for w, o, f in zip(want, outs, full):
            assert (o is None) == (not w)
            if w:
                assert np.array_equal(_bits(o).reshape(-1), f), want
    # B = 0 returns 0 and touches nothing; refusals launch nothing
    before = [b.clone() for b in bufs] + [nll.clone()]
    assert lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), 0, C.byref(cond), None, nll.data_ptr(), ptrs[0], ptrs[1], st) == 0
    rows = m._rows_to_dev(PatchCond(np.array([(800, 2, 0, 0)] * B, np.float32)), 0)
    pad = torch.zeros((n + 4,), device="cuda")
    for args in ((xd.data_ptr(), yd.data_ptr(), C.byref(cond), rows.data_ptr()),      # both cond and rows
                 (xd.data_ptr(), yd.data_ptr(), None, None),                          # neither
                 (pad.data_ptr() + 4, yd.data_ptr(), C.byref(cond), None),            # x misaligned by 4 bytes
                 (xd.data_ptr(), None, C.byref(cond), None)):                         # the model has an SDN layer: y is required
        rc = lib.nf_nll_grad(m._flow.ptr, args[0], args[1], B, args[2], args[3], nll.data_ptr() + 4, ptrs[0], ptrs[1], st)
        assert rc == _lib.NF_EINVAL and lib.nf_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs + [nll]))


# ---- 7. workspace ----------------------------------------------------------------------------------------------------------------------
def test_workspace_is_owned_by_the_handle_and_reservable(shipped_variables):
    """As test_gpu_large_patches.py::test_tiled_workspace_is_owned_by_the_handle_and_reservable: nf_workspace_bytes(h, 2, B) says
    what a tiled nf_nll_grad call needs — (segments - 1) tensors, 2 gradient tensors, the tile sums —, nf_reserve_grad_workspace
    sets it aside, and calls after that run with the device's free memory unchanged."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (96, 80), 3
    small = _flow(FULL_ARCH, shipped_variables, (32, 32))
    assert small._flow.lib.nf_workspace_bytes(small._flow.ptr, 2, 1024) == 0
    _lib.check(small._flow.lib.nf_reserve_grad_workspace(small._flow.ptr, 16, 2))          # nothing to do
    plain = _flow(FULL_ARCH, shipped_variables, hw, grad_tiles=False)
    assert plain._flow.lib.nf_workspace_bytes(plain._flow.ptr, 2, B) == 0
    m = _flow(FULL_ARCH, shipped_variables, hw)
    lib = m._flow.lib
    need = lib.nf_workspace_bytes(m._flow.ptr, 2, B)
    img = B * hw[0] * hw[1] * 16
    assert (7 + 2) * img < need <= (7 + 2) * (img + 256) + 8 * B * 4 * 16 + 256           # 8 segments; <= 4 forward tiles per segment
    _lib.check(lib.nf_reserve_grad_workspace(m._flow.ptr, B, 2))
    x, y = make_inputs(B, hw[0], hw[1], seed=4)
    xt, yt = _dev(x), _dev(y)
    cond = _cond()
    # outputs allocated up front, so that torch's caching allocator is out of the measurement: what moves the device's free
    # memory after this line is the library's
    outs = [(torch.empty((B,), device="cuda"), torch.empty_like(xt), torch.empty_like(yt)) for _ in range(7)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]

    def call(o, stream):
        _lib.check(lib.nf_nll_grad(m._flow.ptr, xt.data_ptr(), yt.data_ptr(), B, C.byref(cond), None, o[0].data_ptr(), o[1].data_ptr(),
                                   o[2].data_ptr(), stream))

    for o in outs[:3]:
        call(o, m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    # two streams on one handle, calls in flight on both: each has a buffer of its own, the bits are those of the serial calls
    for i, o in enumerate(outs[3:]):
        call(o, streams[i & 1].cuda_stream)
    torch.cuda.synchronize()      # (no memory figure here: the runtime sets a new stream's queue up at its first launch)
    assert np.isfinite(outs[0][1].cpu().numpy()).all()
    for o in outs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(o, outs[0]))
    with pytest.raises(Exception):
        _lib.check(lib.nf_reserve_grad_workspace(m._flow.ptr, B, 0))


# ---- 8. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface(shipped_variables, shipped_ref):
    import torch
    from noise_flow_amd import _lib, default_hps, NoiseFlow
    hw, B = (80, 72), 2
    m = _flow(FULL_ARCH, shipped_variables, hw)
    assert _path(m) == _lib.NF_GRAD_PATH_TILED
    x, y = make_inputs(B, hw[0], hw[1], seed=0)                                            # on-kink per image: [5, 4], pinned e32 1.6e-6
    reference_conditions(shipped_ref, 4, x, y, ISO, CAM)
    n_np, gx_np, gy_np = m.nll_and_grad(x, y, iso=[ISO], cam=[CAM])                        # numpy in, numpy out
    assert isinstance(gx_np, np.ndarray) and gx_np.shape == x.shape and gy_np.shape == y.shape
    compare_with_kink_rule(shipped_ref, 4, x, y, ISO, CAM, gx_np, gy_np, log=print)
    want = shipped_ref.oracle_nll(x, y, ISO, CAM)
    assert np.all(np.abs(n_np - want) <= NLL_RTOL * np.abs(want))
    nll0, gx, gy = m.nll_and_grad(_dev(x), _dev(y), iso=[ISO], cam=[CAM])
    assert np.array_equal(gx.cpu().numpy(), gx_np) and np.array_equal(gy.cpu().numpy(), gy_np) and np.array_equal(nll0.cpu().numpy(), n_np)
    xt, yt = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
    nll = m.nll_torch(xt, yt, iso=[ISO], cam=[CAM])
    nll.sum().backward()
    assert torch.equal(nll.detach(), nll0) and torch.equal(xt.grad, gx) and torch.equal(yt.grad, gy)
    # hps.grad_tiles is the same switch; a default model still refuses
    hp = default_hps(arch=FULL_ARCH, width=4)
    hp.grad_tiles = True
    assert _path(NoiseFlow([65, 65, 4], False, hp, variables=shipped_variables)) == _lib.NF_GRAD_PATH_TILED
    plain = _flow(FULL_ARCH, shipped_variables, (65, 65), grad_tiles=False)
    x65, y65 = make_inputs(1, 65, 65)
    with pytest.raises(_lib.NoiseFlowLibError, match="64x64"):
        plain.nll_and_grad(x65, y65, iso=[ISO], cam=[CAM])
    # a shape the whole-patch kernel holds stays on it with the flag: same bits as without
    x32, y32 = make_inputs(2, 32, 32, seed=3)
    a = _flow(FULL_ARCH, shipped_variables, (32, 32)).nll_and_grad(x32, y32, iso=[ISO], cam=[CAM])
    b = _flow(FULL_ARCH, shipped_variables, (32, 32), grad_tiles=False).nll_and_grad(x32, y32, iso=[ISO], cam=[CAM])
    assert _path(_flow(FULL_ARCH, shipped_variables, (32, 32))) == _lib.NF_GRAD_PATH_SCALAR
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
