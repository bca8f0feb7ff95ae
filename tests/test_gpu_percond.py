"""Per-patch conditioning (nf_nll_percond / nf_sample_percond, length-B iso / cam lists on the Python surface).

1. A mixed batch through the per-patch entries gives every patch the BITS the per-call entries give it alone under its own
   (ISO, camera) — on every kernel family, the tiled path included.  Batch independence of every kernel is a tested property
   (tests/test_gpu_batch_independence.py), so equality needs no tolerance.
2. The row is the patch's, not the workgroup's: more patches than any launch keeps resident, the tuple cycling with period 7.
3. Against the fp64 oracle on the shipped model, all 25 (ISO, camera) pairs in one call, at the project's tolerances — after
   checking on the oracle that the test could tell any two of the 25 apart.
4. The surface: NoiseFlowWrapper.sample_noise_nf with lists, rejected inputs, B = 0.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import SHIPPED_DIR, close_elem, make_inputs
from test_cond_rows_cpu import cond_variables

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-5
ARCH = "sdn5|unc|gain|unc|sdn3"     # leading SDN (prefetch path), a mid-program gain with a per-patch log-det, a trailing SDN
TUPLES5 = [(100, 0), (400, 1), (800, 2), (1600, 3), (3200, 4)]
TUPLES7 = TUPLES5 + [(100, 3), (1600, 0)]
BASE = 17


def _model(arch, width, hw, cnn_dtype, seed=5):
    from noise_flow_amd import NoiseFlow, default_hps
    v = cond_variables(arch, width, seed=seed)
    for k in v:   # scales of O(1) at every ISO (the reference's initial values give gain scales of 5 .. 150 and an sdn3 gain of
        #           0.7 .. 21: samples of 1e4, beyond what the fp16 CNNs can hold): sigmoid(g1 - 6) * iso, exp(0.1 (t - 30)) * iso
        if k == "model/g1":
            v[k] = (v[k] - 6.0).astype(np.float32)
        elif "gain_param_" in k:
            v[k] = (v[k] - 30.0).astype(np.float32)
    if width > 4:
        for k in v:   # activations of O(1) at every width, as tests/test_gpu_gemm.py::_variables
            if k.endswith("l_2/W") or k.endswith("l_last/W"):
                v[k] = (v[k] * np.float32((4.0 / width) ** 0.5)).astype(np.float32)
    return NoiseFlow([hw[0], hw[1], 4], False, default_hps(arch=arch, width=width), variables=v, cnn_dtype=cnn_dtype)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _rows(m, table, direction):
    from noise_flow_amd.noise_flow_model import PatchCond
    return m._rows_to_dev(PatchCond(np.asarray(table, np.float32)), direction)


def _nll(m, x, y, rows=None, cond=None):
    """nf_nll_percond (rows) or nf_nll (cond) on device tensors → [nll, sd, logdet, z] as numpy."""
    import torch
    from noise_flow_amd import _lib
    B = int(x.shape[0])
    nll, sd, ld = (torch.empty((B,), device="cuda") for _ in range(3))
    z = torch.empty_like(x)
    lib, st = m._flow.lib, m._dev.stream_ptr()
    if rows is not None:
        rc = lib.nf_nll_percond(m._flow.ptr, x.data_ptr(), y.data_ptr(), B, rows.data_ptr(), nll.data_ptr(), sd.data_ptr(), ld.data_ptr(),
                                z.data_ptr(), None, 0, st)
    else:
        rc = lib.nf_nll(m._flow.ptr, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(), ld.data_ptr(),
                        z.data_ptr(), None, 0, st)
    _lib.check(rc)
    return [t.cpu().numpy() for t in (nll, sd, ld, z)]


def _sample(m, y, eps, base, rows=None, cond=None, seed=1234):
    """nf_sample_percond / nf_sample; eps = None: the in-kernel Philox draw keyed (seed, base + b, pixel)."""
    import torch
    from noise_flow_amd import _lib
    B = int(y.shape[0])
    out = torch.empty_like(y)
    lib, st = m._flow.lib, m._dev.stream_ptr()
    ep = eps.data_ptr() if eps is not None else None
    if rows is not None:
        rc = lib.nf_sample_percond(m._flow.ptr, y.data_ptr(), ep, seed, base, 1.0, B, rows.data_ptr(), out.data_ptr(), st)
    else:
        rc = lib.nf_sample(m._flow.ptr, y.data_ptr(), ep, seed, base, 1.0, B, C.byref(cond), out.data_ptr(), st)
    _lib.check(rc)
    return out.cpu().numpy()


def _bits_equal(a, b, what):
    assert np.isfinite(a).all(), what
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), what


def _inputs(B, hw, seed):
    x, y = make_inputs(B, hw[0], hw[1], seed=seed)
    eps = np.random.RandomState(seed + 1).randn(*x.shape).astype(np.float32)
    return _dev(x), _dev(y), _dev(eps)


def _check_mixed_against_one_per_call(m, B, hw, tuples, seed=11):
    """The mixed batch through the per-patch entries == every patch alone (B = 1, patch_index_base = BASE + b) per call."""
    from noise_flow_amd import _lib
    x, y, eps = _inputs(B, hw, seed)
    table = np.array([(tuples[b % len(tuples)][0], tuples[b % len(tuples)][1], 0, 0) for b in range(B)], np.float32)
    got = _nll(m, x, y, rows=_rows(m, table, 0))
    rows1 = _rows(m, table, 1)
    got_eps = _sample(m, y, eps, 0, rows=rows1)
    got_phx = _sample(m, y, None, BASE, rows=rows1)
    for b in range(B):
        cond = _lib.nf_cond(float(table[b, 0]), float(table[b, 1]), 0.0, 0.0)
        s = slice(b, b + 1)
        for name, g, w in zip(("nll", "sd", "logdet", "z"), got, _nll(m, x[s], y[s], cond=cond)):
            _bits_equal(g[s], w, (name, b))
        _bits_equal(got_eps[s], _sample(m, y[s], eps[s], 0, cond=cond), ("x from eps", b))
        _bits_equal(got_phx[s], _sample(m, y[s], None, BASE + b, cond=cond), ("x from Philox", b))
    # ... and the batch is really mixed: patches of different tuples differ from what ONE tuple for the whole call gives
    cond0 = _lib.nf_cond(float(table[0, 0]), float(table[0, 1]), 0.0, 0.0)
    one = _nll(m, x, y, cond=cond0)
    assert all(not np.array_equal(one[3][b], got[3][b]) for b in range(B) if tuple(table[b]) != tuple(table[0]))


# (arch, width, (H, W), cnn_dtype, kernel path)
FAMILIES = [
    (ARCH, 4, (32, 32), "fp32", "SPLIT_BF16"),
    (ARCH, 4, (32, 32), "fp32_exact", "MFMA4"),       # every conv on v_mfma_f32_4x4x1
    (ARCH, 4, (5, 7), "fp32", "MFMA4"),               # a ragged shape at width 4 is the masked matrix-core instantiation ...
    (ARCH, 8, (5, 7), "fp32", "SCALAR"),              # ... the scalar-weight kernel is what width 8 runs on
    (ARCH, 4, (32, 32), "fp16", "FP16"),
    (ARCH, 4, (64, 64), "fp16", "FP16"),
    (ARCH, 16, (16, 16), "fp32", "WIDE16"),
    (ARCH, 32, (16, 16), "fp32", "WIDE32"),
    (ARCH, 32, (16, 16), "fp16", "WIDE32_FP16"),
    (ARCH, 48, (8, 8), "fp32", "GEMM"),
    (ARCH, 48, (8, 8), "fp16", "GEMM_FP16"),
    ("gain2|unc|sdn6", 4, (8, 8), "fp32", None),       # GAIN2's H*W*C log-det, SDN6's camera
]


@pytest.mark.parametrize("arch,width,hw,cnn_dtype,path", FAMILIES,
                         ids=["%s-w%d-%dx%d-%s" % (f[0].split("|")[0], f[1], f[2][0], f[2][1], f[3]) for f in FAMILIES])
def test_mixed_batch_has_the_bits_of_the_per_call_path(arch, width, hw, cnn_dtype, path):
    from noise_flow_amd import _lib
    m = _model(arch, width, hw, cnn_dtype)
    if path is not None:
        for direction in (0, 1):
            assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == getattr(_lib, "NF_PATH_" + path)
    _check_mixed_against_one_per_call(m, 10, hw, TUPLES5)


@pytest.mark.parametrize("segments", [None, 2])
def test_tiled_images_take_the_row_of_the_image(monkeypatch, segments):
    """80x72 images run as overlapping tiles (NF_K_TILED): `b` of the launch is a tile, the row is the image's — in every
    segment's launch and in the kernel that adds the tiles' sums up.  Once with the library's own segment plan, once cut in two."""
    if segments is None:
        monkeypatch.delenv("NF_TILE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("NF_TILE_SEGMENTS", str(segments))
    m = _model("sdn5|unc|unc|gain|unc|unc", 4, (80, 72), "fp32")
    cfg, descs, flat = m._flow._model_args
    out5 = (C.c_int32 * 80)()
    n = m._flow.lib.nf_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, 0, out5, 16)
    assert n >= 1 and (segments is None or n == segments)
    assert out5[3] * out5[4] > 1          # more than one tile per image: tile index != image index
    _check_mixed_against_one_per_call(m, 3, (80, 72), TUPLES5[1:4])


@pytest.mark.parametrize("width,hw,path", [(4, (32, 32), "SPLIT_BF16"), (16, (8, 8), "WIDE16"), (32, (8, 8), "WIDE32"), (48, (8, 8), "GEMM")],
                         ids=["w4-32x32", "w16-8x8", "w32-8x8", "w48-8x8"])
def test_the_row_is_the_patch_s_not_the_workgroup_s(width, hw, path):
    """B = 1 100: the persistent workgroups walk several patches each (256 CUs x at most 4 resident workgroups of these shapes'
    kernels < 1 100), the tuple cycling with period 7 — coprime to any grid size that is a multiple of the CU count, so a row
    taken by workgroup instead of by patch cannot come out right.  Against seven per-call launches of the patches k, k + 7, ..."""
    from noise_flow_amd import _lib
    B = 1100
    m = _model(ARCH, width, hw, "fp32")
    assert m._flow.lib.nf_kernel_path(m._flow.ptr, 0) == getattr(_lib, "NF_PATH_" + path)
    x, y, eps = _inputs(B, hw, 23)
    table = np.array([(TUPLES7[b % 7][0], TUPLES7[b % 7][1], 0, 0) for b in range(B)], np.float32)
    got = _nll(m, x, y, rows=_rows(m, table, 0))
    got_x = _sample(m, y, eps, 0, rows=_rows(m, table, 1))
    for k in range(7):
        cond = _lib.nf_cond(float(TUPLES7[k][0]), float(TUPLES7[k][1]), 0.0, 0.0)
        xs, ys, es = (t[k::7].contiguous() for t in (x, y, eps))
        for name, g, w in zip(("nll", "sd", "logdet", "z"), got, _nll(m, xs, ys, cond=cond)):
            _bits_equal(g[k::7], w, (name, k))
        _bits_equal(got_x[k::7], _sample(m, ys, es, 0, cond=cond), ("x", k))


def test_all_25_conditions_in_one_call_match_the_oracle(shipped_variables, oracle_full):
    """Shipped model, B = 25: every ISO x camera pair, one per patch, through _loss / inverse / sample with length-B lists; the
    oracle is called per patch with that patch's pair.  First, on the oracle alone: any two of the 25 pairs move the latent of
    one patch by at least 1e-3 of its scale (measured: 1.0e-2 for the closest two, (800, 0) and (1600, 0)) — 100 x the tolerance
    below, so a row swapped for any other one fails."""
    from noise_flow_amd import NoiseFlow, default_hps
    pairs = [(iso, cam) for iso in (100, 400, 800, 1600, 3200) for cam in range(5)]
    x1, y1 = make_inputs(1, seed=1)
    z1 = [oracle_full.inverse(x1, y1, iso, cam)[0] for iso, cam in pairs]
    sep = min(np.abs(a - b).max() / max(np.abs(a).max(), np.abs(b).max()) for a, b in itertools.combinations(z1, 2))
    print("closest two conditions differ by %.3e of the latent's scale" % sep)
    assert sep >= 1e-3

    B = len(pairs)
    x, y = make_inputs(B, seed=1)
    eps = np.random.RandomState(2).randn(*x.shape).astype(np.float32)
    iso, cam = [float(p[0]) for p in pairs], [float(p[1]) for p in pairs]
    m = NoiseFlow([32, 32, 4], False, default_hps(), variables=shipped_variables)
    nll, sd_z = m._loss(x, y, [0.0], [0.0], iso, cam)
    z, obj = m.inverse(x, None, y, [0.0], [0.0], np.asarray(iso), np.asarray(cam))
    smp = m.sample(y, 1.0, y, [0.0], [0.0], iso, cam, eps=eps)
    ref_nll, ref_sd, ref_z, ref_obj, ref_x = [], [], [], [], []
    for b, (i, c) in enumerate(pairs):
        s = slice(b, b + 1)
        n_, sd_, z_ = oracle_full.nll(x[s], y[s], i, c)
        ref_nll.append(n_[0]); ref_sd.append(sd_); ref_z.append(z_[0])
        ref_obj.append(oracle_full.inverse(x[s], y[s], i, c)[1][0])
        ref_x.append(oracle_full.sample(eps[s], 1.0, y[s], i, c)[0])
    np.testing.assert_allclose(nll, np.asarray(ref_nll), rtol=NLL_RTOL)
    assert abs(sd_z - np.mean(ref_sd)) <= NLL_RTOL * np.mean(ref_sd)
    np.testing.assert_allclose(obj, np.asarray(ref_obj), rtol=NLL_RTOL)
    for b in range(B):     # per patch: the scale of a latent / sample is its own condition's
        close_elem(z[b], ref_z[b], 1e-5)
        close_elem(smp[b], ref_x[b], 1e-5)


def test_wrapper_takes_lists(shipped_variables):
    """NoiseFlowWrapper.sample_noise_nf(batch, 0, 0, iso_list, cam_list) == the same patches one per call, numpy and torch."""
    import torch
    from noise_flow_amd.NoiseFlowWrapper import NoiseFlowWrapper
    B = 6
    _, y = make_inputs(B, seed=4)
    iso = [100.0, 400.0, 800.0, 1600.0, 3200.0, 800.0]
    cam = [0.0, 1.0, 2.0, 3.0, 4.0, 0.0]
    for as_torch in (False, True):
        w = NoiseFlowWrapper(SHIPPED_DIR, seed=9)
        batch = torch.as_tensor(y).cuda() if as_torch else y
        got = w.sample_noise_nf(batch, 0.0, 0.0, iso, cam)           # draws patches 0 .. B-1 of the seed's stream
        assert isinstance(got, torch.Tensor) == as_torch and tuple(got.shape) == y.shape
        got = got.cpu().numpy() if as_torch else got
        w1 = NoiseFlowWrapper(SHIPPED_DIR, seed=9)
        for b in range(B):                                           # one patch per call: the running counter gives patch b
            one = w1.sample_noise_nf(batch[b:b + 1], 0.0, 0.0, iso[b], cam[b])
            _bits_equal(got[b:b + 1], one.cpu().numpy() if as_torch else one, ("wrapper", as_torch, b))
        assert not np.array_equal(got[2], w.sample_noise_nf(batch, 0.0, 0.0, 100.0, 0.0)[2].cpu().numpy() if as_torch
                                  else w.sample_noise_nf(batch, 0.0, 0.0, 100.0, 0.0)[2])


def test_rejected_inputs_and_empty_batches(shipped_variables):
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    m = NoiseFlow([32, 32, 4], False, default_hps(), variables=shipped_variables)
    lib, st = m._flow.lib, m._dev.stream_ptr()
    B = 4
    x, y, eps = _inputs(B, (32, 32), 3)
    table = np.array([(i, c, 0, 0) for i, c in TUPLES5[:B]], np.float32)
    rows = _rows(m, table, 0)
    nll = torch.empty((B,), device="cuda")
    out = torch.empty_like(x)

    def nll_rc(rows_ptr, n=B):
        return lib.nf_nll_percond(m._flow.ptr, x.data_ptr(), y.data_ptr(), n, rows_ptr, nll.data_ptr(), None, None, None, None, 0, st)

    def smp_rc(rows_ptr, n=B):
        return lib.nf_sample_percond(m._flow.ptr, y.data_ptr(), eps.data_ptr(), 0, 0, 1.0, n, rows_ptr, out.data_ptr(), st)

    for f in (nll_rc, smp_rc):
        assert f(rows.data_ptr()) == _lib.NF_OK
        assert f(None) == _lib.NF_EINVAL                           # rows = NULL with B > 0
        assert f(rows.data_ptr() + 4) == _lib.NF_EINVAL            # rows + 1 float: not 16-byte aligned
        host = np.zeros(B * 48 + 16, np.uint8)
        assert f((host.ctypes.data + 15) & ~15) == _lib.NF_EINVAL  # aligned, but not device memory
        assert f(None, 0) == _lib.NF_OK                            # B = 0
        assert f(rows.data_ptr(), 0) == _lib.NF_OK
    torch.cuda.synchronize()
    mt = NoiseFlow([32, 32, 4], True, default_hps(), variables=shipped_variables)
    xs, ys = x[:2], y[:2]
    with pytest.raises(ValueError, match="is_training"):
        mt._loss(xs, ys, [0.0], [0.0], [100.0, 400.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="is_training"):
        mt.sample(ys, 1.0, ys, [0.0], [0.0], [100.0, 400.0], [2.0])
    with pytest.raises(ValueError):                                # neither 1 nor B values
        m._loss(x, y, [0.0], [0.0], [100.0, 400.0, 800.0], [2.0])
    empty = m._loss(x[:0], y[:0], [0.0], [0.0], [100.0], [2.0])[0]
    assert tuple(empty.shape) == (0,)
