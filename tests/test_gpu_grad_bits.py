"""The four gradient kernels (csrc/nf_grad.hip: nf_grad_kernel whole-patch and TILED; csrc/nf_grad_wide.hip: nf_grad_wide_kernel;
csrc/nf_grad_gemm.hip: nf_grad_gemm_kernel; csrc/nf_sample_grad.hip: nf_sample_grad_kernel) share one frame and, the two scalar
ones, one coupling pass (csrc/nf_grad_common.h), and each file has one launcher behind one host dispatcher.  This fixture pins their
per-patch outputs bit for bit, so that code can move between the kernels and the shared header, or between launchers, without a
product, an addition order, a rounding point, a launch geometry, an LDS size or a gate-record size changing:
tests/golden/grad_family_bits.npz was recorded with tools/make_golden_grad_bits.py on an MI355X from the build of commit 7fa8201, the
last one with the frame written per kernel and two launchers per file, every case twice with the same bits.  array_equal on the
uint32 views; a differing bit is an expression that was reordered while moving, or a launch that changed, not a tolerance question.

Per-patch outputs only: nll, gx, gy of nf_nll_grad; x, gy, geps, gtemp of nf_sample_vjp.  Models: `sdn5|unc|unc|gain4|unc` with
sample_vjp_ref.sampling_variables (finite in both directions at every width); the two-segment and conditioning-row cases
`sdn5|unc|gain|unc|sdn3` (an sdn layer in each segment, so that g_in, the gradient ping-pong and NF_GT_GY_ACC run) with the
conditional layers moved off their initial values as in tests/test_gpu_nll_grad.py.  Fixed seeds, B = 2 unless the case says otherwise.

CASES are the smallest shapes that reach each instantiation and each shared piece: every (threads, pixels per lane) of dispatch_grad
and dispatch_sgrad per width, the tiled geometries, every (wavefronts, strip height) of dispatch_grad_wide, every padded width of the
GEMM kernel, a raw width that is zero-padded, and per kernel one case with per-patch conditioning rows and one with a batch that
sends some workgroup through the persistent loop twice (32 x CU count + 1 patches at 7x5 for the flow_launch kernels — occupancy is
clamped at 32 workgroups per CU —, CU count + 1 for the GEMM kernel, which launches at most one workgroup per CU; the first, a middle
and the last patch are kept).  test_every_case_reaches_what_it_names checks the table against the library's own host arithmetic
without a GPU.

What the fixture keeps (it has to stay under 512 KiB): scalars of every patch kept; tensors of up to FULL_UP_TO floats in full; of
every other tensor the first and the last row plus, per row, the sum of the row's uint32 bit patterns (so a changed bit anywhere in
the tensor still shows)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import make_inputs
from sample_vjp_ref import sampling_variables
from test_cond_rows_cpu import cond_variables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_family_bits.npz")
ARCH = "sdn5|unc|unc|gain4|unc"           # 3 couplings
VOCAB_ARCH = "sdn5|unc|gain|unc|sdn3"     # 2 couplings, an sdn layer on either side
SEED, BASE, TEMP = 20251021, 23, 0.6
OCC_MAX = 32                              # flow_launch's clamp on resident workgroups per CU
ISO_CAM = (800.0, 2.0)
PC_TABLE = ((100.0, 0.0), (1600.0, 3.0))  # per-patch conditioning: one (ISO, camera) per patch
FULL_UP_TO = 320                          # floats
NF_GRAD_TILE = 32

# (kernel, coupling width, (H, W), kind, geometry)
#   kernel  scalar: nf_grad_kernel   wide: nf_grad_wide_kernel   gemm: nf_grad_gemm_kernel   svjp: nf_sample_grad_kernel
#   kind    std | pc (conditioning rows) | big (persistent loop) | tiled | seg2 (tiled, NF_GRAD_TILE_SEGMENTS=2, VOCAB_ARCH)
#           svjp only: philox (eps from the key) | nox (x_out absent) | nogt (gtemp_out absent)
#   geometry  scalar / svjp: (threads, pixels per lane) — tiled: of the tile; wide: (wavefronts, rows per strip) — tiled: of the tile;
#             gemm: the padded width
CASES = [
    # nf_grad_kernel, whole patches
    ("scalar", 4, (7, 5), "std", (64, 1)), ("scalar", 4, (9, 17), "std", (256, 1)), ("scalar", 4, (17, 33), "std", (256, 4)),
    ("scalar", 4, (33, 33), "std", (1024, 4)),
    ("scalar", 8, (7, 5), "std", (64, 1)), ("scalar", 8, (9, 17), "std", (256, 1)), ("scalar", 8, (17, 33), "std", (256, 4)),
    ("scalar", 8, (33, 33), "std", (1024, 4)),
    ("scalar", 16, (7, 5), "std", (64, 1)), ("scalar", 16, (9, 17), "std", (256, 1)), ("scalar", 16, (17, 33), "std", (256, 4)),
    ("scalar", 32, (7, 5), "std", (64, 1)), ("scalar", 32, (9, 17), "std", (256, 1)), ("scalar", 32, (17, 33), "std", (1024, 1)),
    ("scalar", 6, (7, 5), "std", (64, 1)),                 # 6 -> 8, zero-padded
    ("scalar", 4, (7, 5), "pc", (64, 1)),
    ("scalar", 4, (7, 5), "big", (64, 1)),
    # nf_grad_kernel, TILED
    ("scalar", 4, (2, 80), "tiled", (64, 1)), ("scalar", 4, (8, 80), "tiled", (256, 1)), ("scalar", 4, (40, 72), "tiled", (256, 4)),
    ("scalar", 8, (2, 80), "tiled", (64, 1)), ("scalar", 8, (8, 80), "tiled", (256, 1)), ("scalar", 8, (40, 72), "tiled", (256, 4)),
    ("scalar", 16, (2, 80), "tiled", (64, 1)), ("scalar", 16, (8, 80), "tiled", (256, 1)), ("scalar", 16, (40, 72), "tiled", (256, 4)),
    ("scalar", 8, (8, 80), "seg2", (256, 1)),
    # nf_grad_wide_kernel
    ("wide", 32, (2, 5), "std", (1, 2)), ("wide", 32, (4, 5), "std", (2, 2)), ("wide", 32, (7, 5), "std", (4, 2)),
    ("wide", 32, (12, 9), "std", (4, 4)), ("wide", 32, (17, 31), "std", (4, 8)),
    ("wide", 32, (7, 5), "pc", (4, 2)),
    ("wide", 32, (7, 5), "big", (4, 2)),
    ("wide", 32, (40, 36), "tiled", (4, 8)), ("wide", 32, (8, 80), "tiled", (4, 2)), ("wide", 32, (40, 36), "seg2", (4, 8)),
    # nf_grad_gemm_kernel
    ("gemm", 64, (7, 5), "std", 64), ("gemm", 128, (7, 5), "std", 128), ("gemm", 256, (7, 5), "std", 256),
    ("gemm", 512, (7, 5), "std", 512), ("gemm", 64, (17, 31), "std", 64),
    ("gemm", 64, (7, 5), "pc", 64),
    ("gemm", 64, (7, 5), "big", 64),
    ("gemm", 64, (40, 36), "tiled", 64), ("gemm", 512, (40, 36), "tiled", 512), ("gemm", 64, (40, 36), "seg2", 64),
    # nf_sample_grad_kernel
    ("svjp", 4, (7, 5), "std", (64, 1)), ("svjp", 4, (9, 17), "std", (256, 1)), ("svjp", 4, (17, 33), "std", (256, 4)),
    ("svjp", 4, (33, 33), "std", (1024, 4)),
    ("svjp", 8, (7, 5), "std", (64, 1)), ("svjp", 8, (9, 17), "std", (256, 1)), ("svjp", 8, (17, 33), "std", (256, 4)),
    ("svjp", 8, (33, 33), "std", (768, 4)),
    ("svjp", 16, (7, 5), "std", (64, 1)), ("svjp", 16, (9, 17), "std", (256, 1)), ("svjp", 16, (17, 33), "std", (256, 4)),
    ("svjp", 32, (7, 5), "std", (64, 1)), ("svjp", 32, (9, 17), "std", (256, 1)), ("svjp", 32, (17, 33), "std", (1024, 1)),
    ("svjp", 4, (9, 17), "philox", (256, 1)), ("svjp", 8, (33, 33), "philox", (768, 4)),
    ("svjp", 4, (9, 17), "nox", (256, 1)), ("svjp", 4, (9, 17), "nogt", (256, 1)),
    ("svjp", 4, (7, 5), "pc", (64, 1)),
    ("svjp", 4, (7, 5), "big", (64, 1)),
]
CASE_IDS = ["%s-w%d-%dx%d-%s" % (c[0], c[1], c[2][0], c[2][1], c[3]) for c in CASES]
TILED_KINDS = ("tiled", "seg2")


def padded_width(width):
    return next(w for w in (4, 8, 16, 32, 64, 128, 256, 512) if width <= w)


def scalar_geometry(wp, pixels, svjp=False):
    """csrc/nf_grad.hip::dispatch_grad and csrc/nf_sample_grad.hip::dispatch_sgrad: (threads, pixels per lane)."""
    if pixels <= 64:
        return (64, 1)
    if pixels <= 256:
        return (256, 1)
    if wp >= 32:
        return (1024, 1)
    if pixels <= 1024:
        return (256, 4)
    return (768, 4) if (svjp and wp == 8) else (1024, 4)


def wide_geometry(H):
    """csrc/nf_grad_wide.hip::dispatch_grad_wide: (wavefronts, rows per strip)."""
    if H > 16:
        return (4, 8)
    if H > 8:
        return (4, 4)
    return (1 if H <= 2 else 2 if H <= 4 else 4, 2)


def _arch(kind):
    return VOCAB_ARCH if kind in ("seg2", "pc") else ARCH


_VARS = {}


def variables(kind, width):
    key = (_arch(kind), width)
    if key not in _VARS:
        if key[0] == ARCH:
            v = sampling_variables(ARCH, width, seed=width)
        else:   # tests/test_gpu_nll_grad.py::_vocab_variables with the width scaling of sampling_variables
            v = cond_variables(VOCAB_ARCH, width, seed=5)
            for k in v:
                if k == "model/g1":
                    v[k] = (v[k] - 6.0).astype(np.float32)
                elif "gain_param_" in k:
                    v[k] = (v[k] - 30.0).astype(np.float32)
                elif k.endswith("l_2/W") or k.endswith("l_last/W"):
                    v[k] = (v[k] * np.sqrt(4.0 / width)).astype(np.float32)
        _VARS[key] = v
    return _VARS[key]


def model_keywords(kernel, kind):
    """The NoiseFlow keywords that send a case to its kernel."""
    kw = {"grad_kernel": {"scalar": "scalar", "svjp": "scalar", "wide": "mfma", "gemm": "gemm"}[kernel]}
    if kind in TILED_KINDS:
        kw["grad_tiles"] = True
    return kw


class forced_segments:
    """NF_GRAD_TILE_SEGMENTS as the case wants it (the library reads it when it plans: nf_create, nf_grad_tile_segments)."""

    def __init__(self, kind):
        self.want = "2" if kind == "seg2" else None

    def __enter__(self):
        self.old = os.environ.pop("NF_GRAD_TILE_SEGMENTS", None)
        if self.want:
            os.environ["NF_GRAD_TILE_SEGMENTS"] = self.want

    def __exit__(self, *exc):
        os.environ.pop("NF_GRAD_TILE_SEGMENTS", None)
        if self.old is not None:
            os.environ["NF_GRAD_TILE_SEGMENTS"] = self.old


def expected_path(kernel, kind):
    from noise_flow_amd import _lib
    tiled = kind in TILED_KINDS
    return {"scalar": _lib.NF_GRAD_PATH_TILED if tiled else _lib.NF_GRAD_PATH_SCALAR,
            "svjp": _lib.NF_GRAD_PATH_SCALAR,
            "wide": _lib.NF_GRAD_PATH_TILED_WIDE32 if tiled else _lib.NF_GRAD_PATH_WIDE32,
            "gemm": _lib.NF_GRAD_PATH_TILED_GEMM if tiled else _lib.NF_GRAD_PATH_GEMM}[kernel]


def host_plan(case):
    """(path of nf_grad_fold, segments of nf_grad_tile_segments, return code of nf_sample_vjp_supported): host arithmetic, no device."""
    from noise_flow_amd import _lib, params
    kernel, width, (H, W), kind, _ = case
    lib = _lib.load()
    kw = model_keywords(kernel, kind)
    flags = {"scalar": 0, "mfma": _lib.NF_CFG_GRAD_MFMA, "gemm": _lib.NF_CFG_GRAD_GEMM}[kw["grad_kernel"]]
    if kw.get("grad_tiles"):
        flags |= _lib.NF_CFG_GRAD_TILED | {"scalar": 0, "mfma": _lib.NF_CFG_GRAD_TILED_WIDE, "gemm": _lib.NF_CFG_GRAD_TILED_GEMM}[kw["grad_kernel"]]
    layers, descs, flat = params.pack(_arch(kind), variables(kind, width), width, "loss_first")
    cfg = _lib.nf_config(H, W, 4, len(layers), -1, flags)
    fp = flat.ctypes.data_as(C.POINTER(C.c_float))
    with forced_segments(kind):
        ops = (C.c_int32 * 256)()
        n_ops, nf, path = C.c_int32(), C.c_size_t(), C.c_int32()
        rc = lib.nf_grad_fold(C.byref(cfg), descs, fp, flat.size, C.byref(path), ops, 128, C.byref(n_ops), None, 0, C.byref(nf))
        assert rc == 0, (case, lib.nf_last_error())
        out = (C.c_int32 * 80)()
        n = lib.nf_grad_tile_segments(C.byref(cfg), descs, fp, flat.size, out, 16)
        svjp = lib.nf_sample_vjp_supported(C.byref(cfg), descs, fp, flat.size)
    return path.value, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))], svjp


def test_every_case_reaches_what_it_names():
    """No GPU: the table's geometry column against the dispatchers' rules, the path and the segments against the library's own host
    arithmetic, and the facts the cases rely on."""
    for case in CASES:
        kernel, width, (H, W), kind, geo = case
        wp = padded_width(width)
        path, segs, svjp = host_plan(case)
        assert path == expected_path(kernel, kind), case
        tiled = kind in TILED_KINDS
        th, tw = (min(H, NF_GRAD_TILE), min(W, NF_GRAD_TILE)) if tiled else (H, W)
        assert (len(segs) > 0) == tiled and (kind != "seg2" or len(segs) == 2) and (not tiled or max(s[3] * s[4] for s in segs) > 1), (case, segs)
        if kernel in ("scalar", "svjp"):
            assert wp <= 32 and scalar_geometry(wp, th * tw, kernel == "svjp") == geo, case
            assert kernel != "svjp" or svjp == 0, case
        elif kernel == "wide":
            assert wp == 32 and wide_geometry(th) == geo, case
        else:
            assert wp == geo and wp >= 64, case
    geos = lambda k, tiled: {(padded_width(c[1]), c[4]) for c in CASES if c[0] == k and (c[3] in TILED_KINDS) == tiled}   # noqa: E731
    whole = {(w, g) for w in (4, 8, 16) for g in ((64, 1), (256, 1), (256, 4))} | {(32, (64, 1)), (32, (256, 1)), (32, (1024, 1))}
    assert geos("scalar", False) == whole | {(4, (1024, 4)), (8, (1024, 4))}
    assert geos("svjp", False) == whole | {(4, (1024, 4)), (8, (768, 4))}
    assert geos("scalar", True) == {(w, g) for w in (4, 8, 16) for g in ((64, 1), (256, 1), (256, 4))}
    assert {g for _, g in geos("wide", False)} == {(1, 2), (2, 2), (4, 2), (4, 4), (4, 8)}
    assert {w for w, _ in geos("gemm", False)} == {64, 128, 256, 512}
    assert ("scalar", 6, (7, 5), "std", (64, 1)) in CASES and padded_width(6) == 8
    for kernel in ("scalar", "wide", "gemm", "svjp"):
        kinds = [c[3] for c in CASES if c[0] == kernel]
        assert kinds.count("pc") == 1 and kinds.count("big") == 1 and (kernel == "svjp" or kinds.count("seg2") == 1), kernel
    kinds = [c[3] for c in CASES if c[0] == "svjp"]
    assert kinds.count("philox") == 2 and kinds.count("nox") == 1 and kinds.count("nogt") == 1


def _reduced(t):
    """First and last row of [B, H, W, 4], and per row the sum of its bit patterns."""
    bits = np.ascontiguousarray(t).view(np.uint32).astype(np.uint64)
    return {"rows": np.ascontiguousarray(t[:, [0, -1]]), "rowsum": bits.sum(axis=(2, 3))}


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def case_outputs(case):
    """What the fixture holds of one case, from the library that is loaded: {name: array}."""
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from noise_flow_amd.noise_flow_model import PatchCond
    kernel, width, (H, W), kind, _ = case
    with forced_segments(kind):
        m = NoiseFlow([H, W, 4], False, default_hps(arch=_arch(kind), width=width), variables=variables(kind, width), **model_keywords(kernel, kind))
    lib, st = m._flow.lib, m._dev.stream_ptr()
    assert lib.nf_grad_path(m._flow.ptr) == expected_path(kernel, kind), case
    B, keep = 2, None
    if kind == "big":
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        B = (n_cu if kernel == "gemm" else OCC_MAX * n_cu) + 1
        keep = [0, B // 2, B - 1]
    x, y = make_inputs(B, H, W, seed=H + W + width)
    rng = np.random.RandomState(SEED)
    eps, g = (rng.randn(B, H, W, 4).astype(np.float32) for _ in range(2))
    xd, yd, ed, gd = _dev(x), _dev(y), _dev(eps), _dev(g)
    cond, rows = _lib.nf_cond(ISO_CAM[0], ISO_CAM[1], 0.0, 0.0), None
    if kind == "pc":
        rows = m._rows_to_dev(PatchCond(np.array([(i, c, 0, 0) for i, c in PC_TABLE], np.float32)), 1 if kernel == "svjp" else 0)
    cp, rp = (C.byref(cond), None) if rows is None else (None, rows.data_ptr())
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    if kernel == "svjp":
        o_x = None if kind == "nox" else torch.empty_like(gd)
        o_gt = None if kind == "nogt" else torch.empty((B,), device="cuda")
        o_gy, o_ge = torch.empty_like(gd), torch.empty_like(gd)
        _lib.check(lib.nf_sample_vjp(m._flow.ptr, p(yd), None if kind == "philox" else p(ed), SEED, BASE, TEMP, B, cp, rp, p(gd), p(o_x), p(o_gy),
                                     p(o_ge), p(o_gt), st))
        res = {"x": o_x, "gy": o_gy, "geps": o_ge, "gtemp": o_gt}
    else:
        o_nll, o_gx, o_gy = torch.empty((B,), device="cuda"), torch.empty_like(xd), torch.empty_like(yd)
        _lib.check(lib.nf_nll_grad(m._flow.ptr, p(xd), p(yd), B, cp, rp, p(o_nll), p(o_gx), p(o_gy), st))
        res = {"nll": o_nll, "gx": o_gx, "gy": o_gy}
    torch.cuda.synchronize()
    out = {}
    for name, t in res.items():
        if t is None:
            continue
        a = t.cpu().numpy()
        assert np.isfinite(a).all(), (case, name)
        if keep is not None:
            a = a[keep]
        parts = {"": a} if a.size <= FULL_UP_TO else _reduced(a)
        for k, v in parts.items():
            v = np.ascontiguousarray(v)
            assert v.dtype in (np.float32, np.uint64), (case, name)
            out["%s__%s%s" % (CASE_IDS[CASES.index(case)], name, "_" + k if k else "")] = v
    return out


def compute_outputs():
    out = {}
    for case in CASES:
        out.update(case_outputs(case))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gradient_kernels_give_the_bits_of_the_stand_alone_kernels(case):
    golden = np.load(GOLDEN)
    got = case_outputs(case)
    prefix = CASE_IDS[CASES.index(case)] + "__"
    assert sorted(got) == sorted(k for k in golden.files if k.startswith(prefix))
    bad = []
    for key, g in got.items():
        want = golden[key]
        assert g.dtype == want.dtype and g.shape == want.shape, key
        view = np.uint32 if g.dtype == np.float32 else np.uint64
        diff = g.view(view) != want.view(view)
        print("%s: %d of %d values differ in some bit" % (key, int(diff.sum()), diff.size))
        if diff.any():
            bad.append(key)
    assert not bad, bad
