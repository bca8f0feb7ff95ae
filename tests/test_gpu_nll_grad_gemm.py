"""nf_nll_grad on the GEMM gradient kernel (NF_CFG_GRAD_GEMM, csrc/nf_grad_gemm.hip): coupling widths 33 .. 512 (padded to
64 / 128 / 256 / 512), whole patches up to 32x32, from the kernel up to torch.autograd.

Comparison rule: that of tests/test_gpu_nll_grad.py, unchanged (nll_grad_ref.compare_with_kink_rule, max_on_kink = 6): per patch and
tensor  max|kernel - ref64| <= max(1e-5, 4 e32) max|ref64|  in the raw and in the whitened norm, at most 3 of a failing patch's
on-kink gates inverted.  Every case first asserts FROM THE REFERENCE ALONE that e32 <= 5e-6 and that no patch has more than 6
on-kink activations (nll_grad_ref.reference_conditions); nll_out is held to the oracle at NLL_RTOL = 1e-5; every case asserts that
the handle launches NF_GRAD_PATH_GEMM.

Dense models (every channel live): paper_like_variables at small shapes — a full 32x32 patch at width >= 128 has 15 .. 128 on-kink
activations, beyond the cap of the rule, which stays where it is.  The full 32x32 shape at widths 128 and 512 is covered by the
EMBEDDED model (tests/test_grad_gemm_cpu.py: the width-32 model's 32 channels scattered over the wide one, every other channel
dead), held to the reference of the width-32 model on the two named patches of tests/test_gpu_nll_grad_wide.py.
Measured distances are printed (run with -s).  On an MI355X, worst patch of all cases, raw and whitened norm alike: gx 1.8e-6 of
max|grad| (the embedded model at width 512: 0.18 of its bound, e32 1.6e-6), gy 1.2e-6; nll_out at most 4.3e-7 relative.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs
from nll_grad_ref import PinnedRef, compare_with_kink_rule, reference_conditions
from test_cond_rows_cpu import cond_variables
from test_grad_gemm_cpu import embedded_variables
from test_grad_wide_supported_cpu import NO_SDN_ARCH, paper_like_variables
from test_gpu_nll_grad import ISO, CAM, NLL_RTOL, TUPLES5, VOCAB_ARCH, WIDE_ARCH, _bits, _call, _cond, _dev
from test_gpu_nll_grad_wide import _inputs_32x32_w32, _model

pytestmark = pytest.mark.gpu


def _flow(arch, variables, hw, width, grad_kernel="gemm", cnn_dtype="fp32", **hps):
    from noise_flow_amd import NoiseFlow, default_hps
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width, **hps), variables=variables, cnn_dtype=cnn_dtype,
                     grad_kernel=grad_kernel)


def _path(m):
    return m._flow.lib.nf_grad_path(m._flow.ptr)


def _check(m, ref, width, x, y, iso, cam, rows=None):
    """One launch against the reference (`width`: that of the REFERENCE model): the conditions from the reference alone, then the
    comparison and kink rules."""
    from noise_flow_amd import _lib
    reference_conditions(ref, width, x, y, iso, cam)
    assert _path(m) == _lib.NF_GRAD_PATH_GEMM
    xd, yd = _dev(x), (_dev(y) if y is not None else None)
    rc, nll, gx, gy = _call(m, xd, yd, cond=None if rows is not None else (_cond(iso, cam) if iso is not None else _cond()), rows=rows)
    _lib.check(rc)
    nll64, dist = compare_with_kink_rule(ref, width, x, y, iso, cam, gx.cpu().numpy(), gy.cpu().numpy() if gy is not None else None, log=print)
    want = ref.oracle_nll(x, y, iso, cam)
    assert np.all(np.abs(nll64 - want) <= 1e-12 * np.abs(want)), (nll64, want)
    got = nll.cpu().numpy().astype(np.float64)
    print("nll: kernel-to-oracle %s" % " ".join("%.2e" % v for v in np.abs(got - want) / np.abs(want)))
    assert np.all(np.abs(got - want) <= NLL_RTOL * np.abs(want))
    return (nll, gx, gy), dist


# ---- 1. dense accuracy at small shapes: every channel live, every padded width -------------------------------------------------
# on-kink per patch from the reference alone (e32 <= 2.2e-6):
# 40 32x32 [3,1,2,0]   64 32x32 [6,3,4,5]   128 16x16 [3,4,4,6]   128 11x14 [2,2,0,3]   300 7x10 [2,3,3,3]   512 5x9 [5,5,2,5]
# 33 16x16 [3,1]   200 9x13 [1,2]
DENSE_CASES = [(40, (32, 32), 4, 0), (64, (32, 32), 4, 2), (128, (16, 16), 4, 1), (128, (11, 14), 4, 0), (300, (7, 10), 4, 1),
               (512, (5, 9), 4, 2), (33, (16, 16), 2, 0), (200, (9, 13), 2, 0)]


@pytest.mark.parametrize("width,hw,B,seed", DENSE_CASES)
def test_dense_accuracy(width, hw, B, seed):
    v, ref = _model(WIDE_ARCH, width)
    x, y = make_inputs(B, hw[0], hw[1], seed)
    _check(_flow(WIDE_ARCH, v, hw, width), ref, width, x, y, ISO, CAM)


# ---- 2. full 32x32 at the real widths: the embedded width-32 model ----------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 512])
def test_full_patch_embedded_model(W):
    v32, ref = _model(FULL_ARCH, 32)
    x, y = _inputs_32x32_w32()
    _check(_flow(FULL_ARCH, embedded_variables(v32, W), (32, 32), W), ref, 32, x, y, ISO, CAM)


# ---- 3. odd shapes at width 64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 32), (32, 1), (7, 32), (32, 5), (17, 31)])
def test_odd_shapes_at_width_64(hw):
    v, ref = _model(WIDE_ARCH, 64)
    x, y = make_inputs(3, hw[0], hw[1], seed=0)
    _check(_flow(WIDE_ARCH, v, hw, 64), ref, 64, x, y, ISO, CAM)


# ---- 4. vocabulary and conditioning ------------------------------------------------------------------------------------------
VW = 64


def _vocab_variables():
    """tests/test_gpu_nll_grad.py::_vocab_variables at width 64, with the width scaling of paper_like_variables."""
    v = cond_variables(VOCAB_ARCH, VW, seed=5)
    for k in v:
        if k == "model/g1":
            v[k] = (v[k] - 6.0).astype(np.float32)
        elif "gain_param_" in k:
            v[k] = (v[k] - 30.0).astype(np.float32)
        elif k.endswith("l_2/W"):
            v[k] = (v[k] * np.sqrt(4.0 / VW)).astype(np.float32)
        elif k.endswith("l_last/W"):
            v[k] = (v[k] * np.sqrt(5.0 / (VW + 1))).astype(np.float32)
    return v


def test_vocabulary_mixed_batch_through_rows():
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import PatchCond
    v, ref = _model(VOCAB_ARCH, VW, _vocab_variables())
    m = _flow(VOCAB_ARCH, v, (16, 16), VW)
    x, y = make_inputs(5, 16, 16, seed=1)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5], np.float32)
    rows = m._rows_to_dev(PatchCond(table), 0)
    (nll, gx, gy), _ = _check(m, ref, VW, x, y, table[:, 0], table[:, 1], rows=rows)
    # every patch has the bits the per-call entry gives it under the same condition
    for b, (iso, cam) in enumerate(TUPLES5):
        rc, n1, gx1, gy1 = _call(m, _dev(x[b:b + 1]), _dev(y[b:b + 1]), cond=_cond(iso, cam))
        _lib.check(rc)
        assert _bits(n1)[0] == _bits(nll)[b] and np.array_equal(_bits(gx1)[0], _bits(gx)[b]) and np.array_equal(_bits(gy1)[0], _bits(gy)[b]), b


# ---- 5. contract -------------------------------------------------------------------------------------------------------------
def test_output_subsets_and_empty_batch():
    import torch
    from noise_flow_amd import _lib
    hw, B = (9, 13), 3
    v, _ = _model(WIDE_ARCH, 64)
    m = _flow(WIDE_ARCH, v, hw, 64)
    assert _path(m) == _lib.NF_GRAD_PATH_GEMM
    x, y = make_inputs(B, hw[0], hw[1], seed=1)
    xd, yd = _dev(x), _dev(y)
    rc, nll, gx, gy = _call(m, xd, yd, cond=_cond())
    _lib.check(rc)
    full = {"nll": _bits(nll), "gx": _bits(gx), "gy": _bits(gy)}
    assert all(np.isfinite(a.view(np.float32)).all() for a in full.values())
    for mask in range(7):
        want = {"nll": bool(mask & 1), "gx": bool(mask & 2), "gy": bool(mask & 4)}
        rc, *outs = _call(m, xd, yd, cond=_cond(), **want)
        _lib.check(rc)
        for name, t in zip(("nll", "gx", "gy"), outs):
            assert (t is not None) == want[name]
            if t is not None:
                assert np.array_equal(_bits(t), full[name]), (mask, name)
    # B = 0 returns 0 and touches nothing
    before = (gx.clone(), gy.clone(), nll.clone())
    lib, st, cond = m._flow.lib, m._dev.stream_ptr(), _cond()
    assert lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), yd.data_ptr(), 0, C.byref(cond), None, nll.data_ptr(), gx.data_ptr(), gy.data_ptr(), st) == 0
    assert lib.nf_nll_grad(m._flow.ptr, None, None, 0, C.byref(cond), None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (gx, gy, nll)))
    assert lib.nf_workspace_bytes(m._flow.ptr, 2, 0) == 0 and lib.nf_workspace_bytes(m._flow.ptr, 2, 1) > 0


def test_model_without_sdn_takes_no_y():
    import torch
    from noise_flow_amd import _lib
    v, ref = _model(NO_SDN_ARCH, 64)
    m = _flow(NO_SDN_ARCH, v, (8, 8), 64)
    x = make_inputs(3, 8, 8, seed=0)[0]
    _check(m, ref, 64, x, None, None, None)
    xd = _dev(x)
    gy = torch.empty_like(xd)
    rc = m._flow.lib.nf_nll_grad(m._flow.ptr, xd.data_ptr(), None, 3, C.byref(_cond()), None, None, None, gy.data_ptr(), m._dev.stream_ptr())
    assert rc == _lib.NF_EINVAL and m._flow.lib.nf_last_error()


def test_batch_independence_on_the_persistent_grid():
    """The launch is one workgroup per CU: B = 3 x CUs makes every workgroup take three patches on the tiles, the band and the gate
    record the previous one left behind.  Patches cycle through 7 distinct ones: equal inputs give equal bits, those of the B = 1 call."""
    import torch
    from noise_flow_amd import _lib
    hw = (8, 8)
    v, _ = _model(WIDE_ARCH, 64)
    m = _flow(WIDE_ARCH, v, hw, 64)
    assert _path(m) == _lib.NF_GRAD_PATH_GEMM
    B = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    x7, y7 = make_inputs(7, hw[0], hw[1], seed=9)
    idx = np.arange(B) % 7
    rc, nll, gx, gy = _call(m, _dev(x7[idx]), _dev(y7[idx]), cond=_cond())
    _lib.check(rc)
    nll, gx, gy = _bits(nll), _bits(gx), _bits(gy)
    assert np.isfinite(nll.view(np.float32)).all() and np.isfinite(gx.view(np.float32)).all() and np.isfinite(gy.view(np.float32)).all()
    for r in range(7):
        assert np.all(nll[r::7] == nll[r]) and np.all(gx[r::7] == gx[r]) and np.all(gy[r::7] == gy[r]), r
    for b in range(7):
        rc, n1, gx1, gy1 = _call(m, _dev(x7[b:b + 1]), _dev(y7[b:b + 1]), cond=_cond())
        _lib.check(rc)
        assert _bits(n1)[0] == nll[b] and np.array_equal(_bits(gx1)[0], gx[b]) and np.array_equal(_bits(gy1)[0], gy[b]), b


def test_two_host_threads_on_two_streams():
    """Two calls on one handle from two host threads, each on a stream of its own, after nf_reserve_grad_workspace(h, B, 2): each has
    a gate-record buffer of its own and gives the bits of the serial call."""
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 6
    v, _ = _model(WIDE_ARCH, 64)
    m = _flow(WIDE_ARCH, v, hw, 64)
    lib, h = m._flow.lib, m._flow.ptr
    assert _path(m) == _lib.NF_GRAD_PATH_GEMM
    _lib.check(lib.nf_reserve_grad_workspace(h, B, 2))
    data = [tuple(_dev(a) for a in make_inputs(B, hw[0], hw[1], seed=s)) for s in (3, 4)]
    serial = []
    for xd, yd in data:
        rc, nll, gx, gy = _call(m, xd, yd, cond=_cond())
        _lib.check(rc)
        serial.append((_bits(nll), _bits(gx), _bits(gy)))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in data]
    outs = [(torch.empty((B,), device="cuda"), torch.empty_like(xd), torch.empty_like(yd)) for xd, yd in data]
    rcs = [None, None]
    gate = threading.Barrier(2)

    def work(i):
        cond = _cond()
        xd, yd = data[i]
        gate.wait()
        for _ in range(4):   # the same call four times over: the buffers are taken and released while the other thread does the same
            rcs[i] = lib.nf_nll_grad(h, xd.data_ptr(), yd.data_ptr(), B, C.byref(cond), None, outs[i][0].data_ptr(), outs[i][1].data_ptr(),
                                     outs[i][2].data_ptr(), streams[i].cuda_stream)
            if rcs[i] != 0:
                break

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert rcs == [0, 0], rcs
    for i in range(2):
        assert all(np.array_equal(_bits(o), s) for o, s in zip(outs[i], serial[i])), i


# ---- 6. the flag only adds -----------------------------------------------------------------------------------------------------
def test_flag_leaves_the_forward_kernels_alone():
    from noise_flow_amd import _lib
    v, _ = _model(WIDE_ARCH, 64)
    x, y = make_inputs(3, 16, 16, seed=0)
    out = []
    for gk in ("gemm", "scalar"):
        m = _flow(WIDE_ARCH, v, (16, 16), 64, grad_kernel=gk)
        nll, sd = m._loss(_dev(x), _dev(y), iso=[ISO], cam=[CAM])
        out.append((m._flow.lib.nf_kernel_path(m._flow.ptr, 0), m._flow.lib.nf_kernel_path(m._flow.ptr, 1), _bits(nll).tolist(), float(sd)))
    assert out[0] == out[1], out
    assert _path(m) == _lib.NF_EINVAL and b"GEMM families" in m._flow.lib.nf_last_error()


def test_flag_without_effect_at_width_32():
    from noise_flow_amd import _lib
    v, _ = _model(WIDE_ARCH, 32)
    x, y = make_inputs(3, 16, 16, seed=0)
    out = []
    for gk in ("gemm", "scalar"):
        m = _flow(WIDE_ARCH, v, (16, 16), 32, grad_kernel=gk)
        assert _path(m) == _lib.NF_GRAD_PATH_SCALAR
        rc, nll, gx, gy = _call(m, _dev(x), _dev(y), cond=_cond())
        _lib.check(rc)
        out.append((_bits(nll), _bits(gx), _bits(gy)))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---- 7. autograd -------------------------------------------------------------------------------------------------------------
def test_autograd_at_width_64():
    import torch
    from noise_flow_amd import _lib
    hw, B = (16, 16), 4
    v, _ = _model(WIDE_ARCH, 64)
    m = _flow(WIDE_ARCH, v, hw, 64)
    x, y = make_inputs(B, hw[0], hw[1], seed=2)
    iso, cam = [100.0, 400.0, 800.0, 1600.0], [0.0, 1.0, 2.0, 3.0]
    nll0, gx, gy = m.nll_and_grad(_dev(x), _dev(y), iso=iso, cam=cam)
    assert torch.isfinite(nll0).all() and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    xt, yt = _dev(x).requires_grad_(True), _dev(y).requires_grad_(True)
    nll = m.nll_torch(xt, yt, iso=iso, cam=cam)
    nll.mean().backward()
    assert torch.equal(nll.detach(), nll0)
    assert torch.equal(xt.grad, gx / B) and torch.equal(yt.grad, gy / B)
    # a denoiser loss: the gradient reaches `clean` through both arguments, d/d clean nll(noisy - clean, clean) = gy - gx
    noisy, clean = _dev(x + y), _dev(y).requires_grad_(True)
    m.nll_torch(noisy - clean, clean, iso=iso, cam=cam).mean().backward()
    _, gx2, gy2 = m.nll_and_grad((noisy - clean).detach(), clean.detach(), iso=iso, cam=cam)
    assert torch.equal(clean.grad, gy2 / B - gx2 / B)
    # without grad_kernel="gemm" the same call raises as before
    m0 = _flow(WIDE_ARCH, v, hw, 64, grad_kernel=None)
    with pytest.raises(_lib.NoiseFlowLibError, match="GEMM families"):
        m0.nll_torch(_dev(x).requires_grad_(True), _dev(y), iso=iso, cam=cam).mean().backward()
