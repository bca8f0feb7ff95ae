"""nf_nll_grad at coupling widths 33 .. 512 beyond 32x32 (NF_CFG_GRAD_TILED_GEMM): tiles of the GEMM gradient kernel
(csrc/nf_grad_gemm.hip, TILED), one launch per segment.

The rule is ``_check`` of tests/test_gpu_nll_grad.py, unchanged: per image and tensor both norms of tests/nll_grad_ref.py with
tol = max(1e-5, 4 e32), at most 3 excused kinks, nll_out to the fp64 oracle at NLL_RTOL = 1e-5; the preconditions — pinned e32 <=
5e-6 in both norms, at most 6 on-kink activations per image — are asserted from the reference alone before the kernel's output is
read.  Every case asserts that the handle launches NF_GRAD_PATH_TILED_GEMM.

Dense models (every channel live) run where the cap of 6 lets them: all four padded widths, both tiling axes at width 64, tile
heights 32 / 4 / 2 / 1.  Full 40x36 tiling at widths >= 128 has too many kinks when dense and runs on the EMBEDDED model
(tests/test_grad_gemm_cpu.py), held to the width-32 reference on the inputs of tests/test_gpu_nll_grad_tiled_wide.py.  A halo one
pixel short shows at fp32 resolution only in a segment of ONE coupling (tests/test_nll_grad_rule_tiled_gemm_cpu.py): the 8-coupling
cases at S = 8 are the ones that catch a halo or core slip.  The on-kink counts per image (CPU reference) stand beside every case;
every pinned e32 is <= 2.3e-6.
Measured distances are printed (run with -s).  On an MI355X, worst image of all cases, either norm: gx 1.2e-6 (0.12 of its bound)
and gy 1.5e-6 of the norm's maximum (0.14 of its bound), both on the 8-coupling embedded model at 8x66, nll_out 3.8e-7 relative.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs
from test_grad_gemm_cpu import embedded_variables
from test_grad_wide_supported_cpu import NO_SDN_ARCH
from test_gpu_nll_grad import ISO, CAM, TUPLES5, VOCAB_ARCH, WIDE_ARCH, _bits, _call, _check, _cond, _dev
from test_gpu_nll_grad_gemm import VW, _vocab_variables
from test_gpu_nll_grad_tiled import _path, _segments
from test_gpu_nll_grad_wide import _model

pytestmark = pytest.mark.gpu

_INPUTS, _EMB, _VOCAB = {}, {}, {}


def _inputs(B, hw, seed):
    """make_inputs, once per case: the reference memoises on the arrays themselves."""
    key = (B, hw, seed)
    if key not in _INPUTS:
        _INPUTS[key] = make_inputs(B, hw[0], hw[1], seed=seed)
    return _INPUTS[key]


def _embedded(arch, W):
    """(variables of the width-W embedding, width-32 reference) of the width-32 test model."""
    v32, ref = _model(arch, 32)
    if (arch, W) not in _EMB:
        _EMB[(arch, W)] = embedded_variables(v32, W)
    return _EMB[(arch, W)], ref


def _vocab():
    if not _VOCAB:
        _VOCAB["v"] = _vocab_variables()
    return _VOCAB["v"]


def _flow(arch, variables, hw, width, grad_tiles=True, grad_kernel="gemm", **hps):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, grad_kernel=grad_kernel,
                     grad_tiles=grad_tiles)


def _tiled(m):
    from noise_flow_amd import _lib
    assert _path(m) == _lib.NF_GRAD_PATH_TILED_GEMM == 5
    return m


@pytest.fixture(autouse=True)
def _no_forced_count(monkeypatch):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)


# ---- 1. dense, three couplings: every padded width, both tiling axes at 64, tile heights 32 / 4 / 2 / 1 -----------------------------
# (width, shape, B, seed) [on-kink per image]
DENSE_CASES = [(40, (40, 36), 2, 0),      # [1,1]
               (64, (40, 36), 2, 1),      # [6,4]
               (64, (33, 33), 2, 2),      # [4,6]
               (64, (4, 40), 4, 0),       # [0,0,0,2]
               (64, (2, 40), 4, 0),       # [0,0,0,1]
               (128, (4, 40), 2, 0),      # [0,2]
               (128, (2, 40), 4, 0),      # [0,0,1,1]
               (300, (2, 36), 2, 0),      # [5,1]
               (512, (1, 40), 2, 0),      # [1,2]
               (512, (2, 34), 2, 3)]      # [1,5]


@pytest.mark.parametrize("width,hw,B,seed", DENSE_CASES)
def test_dense_three_couplings(width, hw, B, seed):
    v, ref = _model(WIDE_ARCH, width)
    x, y = _inputs(B, hw, seed)
    _check(_tiled(_flow(WIDE_ARCH, v, hw, width)), ref, width, x, y, ISO, CAM)


# ---- 2. both axes at the wide widths: the embedded width-32 model -------------------------------------------------------------------
# on-kink per image: (40,36) seed 1 [2,4]   (70,12) [1,1]   (12,70) [1,6,2,0]   64x64 seed 2 [6]
@pytest.mark.parametrize("W", [128, 256, 512])
@pytest.mark.parametrize("forced,halos", [(1, [12]), (2, [8, 4]), (3, [4, 4, 4])])
def test_embedded_forced_counts(monkeypatch, W, forced, halos):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    v, ref = _embedded(WIDE_ARCH, W)
    m = _tiled(_flow(WIDE_ARCH, v, (40, 36), W))
    n, segs = _segments(m)
    assert n == forced and [s[2] for s in segs] == halos
    x, y = _inputs(2, (40, 36), 1)
    _check(m, ref, 32, x, y, ISO, CAM)


@pytest.mark.parametrize("W", [128, 256, 512])
@pytest.mark.parametrize("hw,B,seed", [((70, 12), 2, 0), ((12, 70), 4, 0)])
def test_embedded_one_axis(W, hw, B, seed):
    v, ref = _embedded(WIDE_ARCH, W)
    x, y = _inputs(B, hw, seed)
    _check(_tiled(_flow(WIDE_ARCH, v, hw, W)), ref, 32, x, y, ISO, CAM)


def test_embedded_64x64_at_width_512():
    v, ref = _embedded(WIDE_ARCH, 512)
    x, y = _inputs(1, (64, 64), 2)
    _check(_tiled(_flow(WIDE_ARCH, v, (64, 64), 512)), ref, 32, x, y, ISO, CAM)


# ---- 3. eight couplings, embedded: (8,66), B = 4, seed 1, on-kink [4,5,6,1] ----------------------------------------------------------
@pytest.mark.parametrize("W", [128, 512])
@pytest.mark.parametrize("forced,halos", [(None, None), (8, [4] * 8), (4, [8] * 4), (3, [12, 12, 8])])
def test_full_depth(monkeypatch, W, forced, halos):
    if forced:
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    v, ref = _embedded(FULL_ARCH, W)
    m = _tiled(_flow(FULL_ARCH, v, (8, 66), W))
    n, segs = _segments(m)
    assert [s[2] for s in segs] == (halos or [4] * 8)      # unforced: the planner's own choice is one coupling per segment, too
    x, y = _inputs(4, (8, 66), 1)
    _check(m, ref, 32, x, y, ISO, CAM)


# ---- 4. vocabulary and conditioning at width 64: the trailing sdn3 makes gy come from two launches -----------------------------------
# (36,33), B = 3, seed 0 (the first tried): on-kink per image, per-call cond [6,5,6], per-image rows [4,3,5]; pinned e32 <= 2.3e-6
VOCAB_HW, VOCAB_SEED, VOCAB_ROWS_SEED = (36, 33), 0, 0


def test_vocabulary_per_call_cond(monkeypatch):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")      # sdn5 in the first segment, sdn3 in the second
    v, ref = _model(VOCAB_ARCH, VW, _vocab())
    m = _tiled(_flow(VOCAB_ARCH, v, VOCAB_HW, VW))
    assert _segments(m)[0] == 2
    x, y = _inputs(3, VOCAB_HW, VOCAB_SEED)
    _check(m, ref, VW, x, y, 1600.0, 3.0)


def test_vocabulary_per_image_rows(monkeypatch):
    from noise_flow_amd.noise_flow_model import PatchCond
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")
    v, ref = _model(VOCAB_ARCH, VW, _vocab())
    m = _tiled(_flow(VOCAB_ARCH, v, VOCAB_HW, VW))
    x, y = _inputs(3, VOCAB_HW, VOCAB_ROWS_SEED)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5[:3]], np.float32)
    rows = m._rows_to_dev(PatchCond(table), 0)
    _check(m, ref, VW, x, y, table[:, 0], table[:, 1], rows=rows)


# ---- 5. a model without an SDN layer: y = NULL ---------------------------------------------------------------------------------------
def test_model_without_sdn():
    import torch
    from noise_flow_amd import _lib
    v, ref = _model(NO_SDN_ARCH, 64)
    m = _tiled(_flow(NO_SDN_ARCH, v, (66, 12), 64))
    x = np.random.RandomState(0).randn(2, 66, 12, 4).astype(np.float32)     # on-kink per image: [5, 5], pinned e32 5.9e-7
    _check(m, ref, 64, x, None, None, None)
    xd = _dev(x)
    gy = torch.empty_like(xd)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), None, 2, C.byref(_cond()), None, None, None, gy.data_ptr(), m._dev.stream_ptr())
    assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error()


# ---- 6. width 33, zero-padded to 64 --------------------------------------------------------------------------------------------------
W33_HW, W33_SEED = (40, 36), 0        # the first seed tried: on-kink per image [1, 1], pinned e32 5.2e-7


def test_width_33():
    v, ref = _model(WIDE_ARCH, 33)
    x, y = _inputs(2, W33_HW, W33_SEED)
    _check(_tiled(_flow(WIDE_ARCH, v, W33_HW, 33)), ref, 33, x, y, ISO, CAM)


# ---- 7. output discipline, image independence ---------------------------------------------------------------------------------------
def test_output_discipline():
    import torch
    from noise_flow_amd import _lib
    hw, B = (40, 36), 3
    v, _ = _model(WIDE_ARCH, 64)
    m = _tiled(_flow(WIDE_ARCH, v, hw, 64))
    x, y = make_inputs(B, hw[0], hw[1], seed=2)
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
    # every subset of the outputs: the ones asked for keep their bits
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        rc, *outs = _call(m, xd, yd, cond=cond, nll=bool(want[0]), gx=bool(want[1]), gy=bool(want[2]))
        _lib.check(rc)
        for w, o, f in zip(want, outs, full):
            assert (o is None) == (not w)
            if w:
                assert np.array_equal(_bits(o).reshape(-1), f), want
    # outputs of image b are the same bits at B = 1 and B = 3
    for b in range(B):
        rc, n1, gx1, gy1 = _call(m, xd[b:b + 1], yd[b:b + 1], cond=cond)
        _lib.check(rc)
        per = n // B
        assert _bits(n1)[0] == full[0][b] and np.array_equal(_bits(gx1).reshape(-1), full[1][b * per:(b + 1) * per])
        assert np.array_equal(_bits(gy1).reshape(-1), full[2][b * per:(b + 1) * per])
    # B = 0 returns 0 and touches nothing
    before = [b.clone() for b in bufs] + [nll.clone()]
    assert lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), 0, C.byref(cond), None, nll.data_ptr(), ptrs[0], ptrs[1], st) == 0
    assert lib.nf_nll_grad(m._flow.ptr, None, None, 0, C.byref(cond), None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, bufs + [nll]))


def test_infeasible_forced_count_is_refused(monkeypatch):
    import torch
    from noise_flow_amd import _lib
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")          # 4 couplings per segment: halo 16, no core in a 32-pixel tile
    v, _ = _embedded(FULL_ARCH, 128)
    m = _flow(FULL_ARCH, v, (8, 66), 128)
    assert _path(m) == _lib.NF_EINVAL
    x, y = (_dev(a) for a in make_inputs(1, 8, 66))
    gx, gy = torch.full_like(x, 1234.5), torch.full_like(y, 1234.5)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, x.data_ptr(), y.data_ptr(), 1, C.byref(_cond()), None, None, gx.data_ptr(), gy.data_ptr(),
                                 m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.NF_EINVAL and b"segments" in m._flow.lib.nf_last_error()
    assert bool((gx == 1234.5).all()) and bool((gy == 1234.5).all())
    nll, _ = m._loss(x, y, [0], [0], [ISO], [CAM])             # the forward direction is not touched by the switch
    assert np.isfinite(nll.cpu().numpy()).all()


# ---- 8. workspace ----------------------------------------------------------------------------------------------------------------------
def test_workspace_is_owned_by_the_handle_and_reservable(monkeypatch):
    """nf_workspace_bytes(h, 2, B) is the sum of its named parts — the tile sums, (segments - 1) kept tensors, 2 gradient tensors, one
    gate record per workgroup of the largest backward launch, sized for the couplings of the largest segment on one tile — plus
    alignment padding; nf_reserve_grad_workspace sets it aside, and calls after that leave the device's free memory alone."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (40, 36), 3
    v, _ = _model(WIDE_ARCH, 64)
    small, plain = _flow(WIDE_ARCH, v, (32, 32), 64), _flow(WIDE_ARCH, v, (32, 32), 64, grad_tiles=False)
    assert _path(small) == _path(plain) == _lib.NF_GRAD_PATH_GEMM
    for nb in (1, 16, 1024):                  # held whole: the gate-record bytes of NF_GRAD_PATH_GEMM, unchanged
        a, b = (f._flow.lib.nf_workspace_bytes(f._flow.ptr, 2, nb) for f in (small, plain))
        assert a == b > 0
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "3")          # one coupling per segment (unforced, 4 tiles are cheapest in one segment)
    m = _tiled(_flow(WIDE_ARCH, v, hw, 64))
    lib = m._flow.lib
    S, segs = _segments(m)
    assert S == 3
    need = lib.nf_workspace_bytes(m._flow.ptr, 2, B)
    img = B * hw[0] * hw[1] * 16
    sums = S * B * 1 * 16                     # one forward tile per segment and image (40x36 is held whole by the forward kernels)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    groups = min(n_cu, max(B * ny * nx for _, _, _, ny, nx in segs))
    bands = -(-32 * 32 // (32768 // 64))      # the tile is 32x32, a band of width 64 has 512 pixels
    gates = groups * 1 * bands * 4096 * 2     # nfgg_gate_halves(1024, 64, 1 coupling) uint16 per workgroup
    parts = sums + (S - 1) * img + 2 * img + gates
    print("workspace: %d bytes = sums %d + %d tensors of %d + gate records %d (+ padding %d)" % (need, sums, S + 1, img, gates, need - parts))
    assert parts <= need <= parts + (1 + (S - 1) + 2 + 1) * 255
    x, y = make_inputs(B, hw[0], hw[1], seed=4)
    xt, yt = _dev(x), _dev(y)
    cond = _cond()
    outs = [(torch.empty((B,), device="cuda"), torch.empty_like(xt), torch.empty_like(yt)) for _ in range(7)]
    streams = [torch.cuda.Stream() for _ in range(2)]

    def call(o, stream, model=m):
        _lib.check(lib.nf_nll_grad(model._flow.ptr, xt.data_ptr(), yt.data_ptr(), B, C.byref(cond), None, o[0].data_ptr(), o[1].data_ptr(),
                                   o[2].data_ptr(), stream))

    # The kernel keeps spilled registers in scratch memory, which the HIP runtime sets aside per hardware queue at a queue's first such
    # launch (not the library's memory).  ANOTHER handle of the same model, shape and plan — the same kernel instantiations, the same
    # scratch size — makes that happen on the three streams first; the handle under test makes no call before the free memory is read
    other = _tiled(_flow(WIDE_ARCH, v, hw, 64))
    assert _segments(other) == (S, segs)
    for st in [m._dev.stream_ptr()] + [s.cuda_stream for s in streams]:
        call(outs[0], st, other)
        torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    _lib.check(lib.nf_reserve_grad_workspace(m._flow.ptr, B, 2))
    free0 = torch.cuda.mem_get_info()[0]
    print("reservation: free memory %d -> %d (2 x need = %d)" % (before, free0, 2 * need))
    assert before - free0 >= 2 * need          # two buffers of everything a call needs, the gate records included
    for o in outs[:3]:
        call(o, m._dev.stream_ptr())
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    for i, o in enumerate(outs[3:]):          # two streams on one handle: each call in flight has a buffer of its own
        call(o, streams[i & 1].cuda_stream)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert np.isfinite(outs[0][1].cpu().numpy()).all()
    for o in outs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(o, outs[0]))


# ---- 9. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface():
    import torch
    from noise_flow_amd import _lib, default_hps, NoiseFlow
    hw, B = (64, 64), 2
    v, _ = _model(WIDE_ARCH, 64)
    m = _tiled(_flow(WIDE_ARCH, v, hw, 64))
    x, y = make_inputs(B, hw[0], hw[1], seed=0)
    n_np, gx_np, gy_np = m.nll_and_grad(x, y, iso=[ISO], cam=[CAM])                        # numpy in, numpy out
    assert isinstance(gx_np, np.ndarray) and gx_np.shape == x.shape and gy_np.shape == y.shape
    assert np.isfinite(n_np).all() and np.isfinite(gx_np).all() and np.isfinite(gy_np).all()
    nll0, gx, gy = m.nll_and_grad(_dev(x), _dev(y), iso=[ISO], cam=[CAM])
    assert np.array_equal(gx.cpu().numpy(), gx_np) and np.array_equal(gy.cpu().numpy(), gy_np) and np.array_equal(nll0.cpu().numpy(), n_np)
    xt, yt = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
    nll = m.nll_torch(xt, yt, iso=[ISO], cam=[CAM])
    nll.sum().backward()
    assert torch.equal(nll.detach(), nll0) and torch.equal(xt.grad, gx) and torch.equal(yt.grad, gy)
    # hps.grad_tiles / hps.grad_kernel are the same switches
    hp = default_hps(arch=WIDE_ARCH, width=64)
    hp.grad_tiles, hp.grad_kernel = True, "gemm"
    assert _path(NoiseFlow([64, 64, 4], False, hp, variables=v)) == _lib.NF_GRAD_PATH_TILED_GEMM
    # grad_kernel="gemm" without grad_tiles still refuses beyond 32x32, and so does grad_tiles without the kernel
    with pytest.raises(_lib.NoiseFlowLibError, match="32x32"):
        _flow(WIDE_ARCH, v, hw, 64, grad_tiles=False).nll_and_grad(x, y, iso=[ISO], cam=[CAM])
    with pytest.raises(_lib.NoiseFlowLibError):
        _flow(WIDE_ARCH, v, hw, 64, grad_kernel="scalar").nll_and_grad(x, y, iso=[ISO], cam=[CAM])
    # a shape the whole-patch GEMM kernel holds stays on it: the bits of a handle without grad_tiles
    x32, y32 = make_inputs(2, 32, 32, seed=3)
    a = _flow(WIDE_ARCH, v, (32, 32), 64).nll_and_grad(x32, y32, iso=[ISO], cam=[CAM])
    b = _flow(WIDE_ARCH, v, (32, 32), 64, grad_tiles=False).nll_and_grad(x32, y32, iso=[ISO], cam=[CAM])
    assert _path(_flow(WIDE_ARCH, v, (32, 32), 64)) == _lib.NF_GRAD_PATH_GEMM == 4
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
