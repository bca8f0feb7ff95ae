"""The two matrix-core kernels between width 4 and the GEMM family (csrc/nf_wide.hip: nf_wide32*_kernel in fp32 and fp16, whole-patch
and tiled; csrc/nf_wide16.hip: nf_wide16_kernel) carry inline what csrc/nf_flow_common.h holds once for the GEMM kernels: input draw /
load, 1x1 mix, sdn and scale layers, the affine half behind l_last, the epilogue.  They share with every other kernel the tile record
(width 16) and the persistent-grid launcher (flow_launch).  This fixture pins their per-patch outputs bit for bit, so that code can
move between the inline copies and the shared helpers, or between launchers, without a product, an addition order or a rounding
point changing: tests/golden/wide_family_bits.npz was recorded with tools/make_golden_wide_bits.py on an MI355X from the build of
commit 98d9469, the last one with a launcher per file.  array_equal on the uint32 views; a differing bit is an expression that was
reordered while moving, not a tolerance question.  (nf_wide16_kernel takes sd_z through the hardware fp32 square root of the rounded
variance, every other kernel through sqrt in double: the fixture holds each kernel's own bits.)

Per-patch outputs only — NLL, sd_z, log-det, latents, samples from a supplied epsilon and from the in-kernel Philox draw; batch
sums and mean losses are added by device atomics in arrival order and are not recorded.  Model and inputs: `sdn5|unc|gain4|unc` and
`_variables` of tests/test_gpu_gemm.py, fixed seeds, B = 2 unless the case says otherwise.

CASES are the smallest shapes at which each shared piece or launch geometry can go wrong, per family: every thread count and strip
height the dispatchers pick (a ragged strip and tile, a strip boundary, the column seams), a width that is zero-padded onto the
kernel, and per family one case each of per-patch conditioning (the PC = true instantiation), an 80x100 image (the tile geometry and
the epilogue's tile share; for width 32 the nf_wide32_tiled* kernels) and a batch of 32 x CU count + 1 patches at 7x5 (occupancy is
clamped at 32 workgroups per CU, so some workgroup takes a second patch through the persistent loop whatever the occupancy is; the
NLL of the first, a middle and the last patch is kept).

What the fixture keeps (it has to stay under 512 KiB): the scalars of every patch; latents in full up to 33x33, samples in
full up to 512 pixels; of every other tensor the first and the last row plus, per row, the sum of the rows'
uint32 bit patterns (so a changed bit anywhere in the tensor still shows)."""
import os

import numpy as np
import pytest

from conftest import make_inputs
from test_gpu_gemm import ARCH, _variables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_family_bits.npz")
SEED, BASE = 20250412, 17
OCC_MAX = 32                                          # the launcher's clamp on resident workgroups per CU
ISO_CAM = (100.0, 2.0)
PC_TABLE = ((100.0, 2.0), (800.0, 0.0))               # per-patch conditioning: one (ISO, camera) per patch

# (family, cnn_dtype, width, (H, W), kind, geometry)   kind: std | pc | tiled | big
#   geometry: wide32 / wide32h (threads, tiles per image row), wide16 (threads, rows per strip); None: a tile of an image
CASES = [
    # nf_wide32, fp32
    ("wide32", "fp32", 32, (7, 5), "std", (256, 1)),       # one ragged strip, ragged tile
    ("wide32", "fp32", 32, (9, 31), "std", (256, 1)),      # strip boundary through `exch`
    ("wide32", "fp32", 32, (33, 9), "std", (512, 1)),      # one tile per row
    ("wide32", "fp32", 32, (9, 33), "std", (512, 2)),      # two tiles per row: column seam, ragged right tile
    ("wide32", "fp32", 32, (33, 33), "std", (1024, 2)),
    ("wide32", "fp32", 24, (7, 5), "std", (256, 1)),       # 24 -> 32, zero-padded
    ("wide32", "fp32", 32, (7, 5), "pc", (256, 1)),
    ("wide32", "fp32", 32, (80, 100), "tiled", None),
    ("wide32", "fp32", 32, (7, 5), "big", (256, 1)),
    # nf_wide32, fp16 CNN
    ("wide32h", "fp16", 32, (7, 5), "std", (256, 1)),
    ("wide32h", "fp16", 32, (9, 33), "std", (512, 2)),
    ("wide32h", "fp16", 32, (33, 33), "std", (1024, 2)),
    ("wide32h", "fp16", 32, (7, 5), "pc", (256, 1)),
    ("wide32h", "fp16", 32, (80, 100), "tiled", None),
    # nf_wide16
    ("wide16", "fp32", 16, (7, 5), "std", (256, 8)),
    ("wide16", "fp32", 16, (9, 33), "std", (512, 8)),      # three column blocks with seams
    ("wide16", "fp32", 16, (17, 33), "std", (1024, 8)),
    ("wide16", "fp32", 16, (33, 49), "std", (1024, 16)),
    ("wide16", "fp32", 12, (7, 5), "std", (256, 8)),       # 12 -> 16, zero-padded
    ("wide16", "fp32", 16, (7, 5), "pc", (256, 8)),
    ("wide16", "fp32", 16, (80, 100), "tiled", None),      # the run-time T.tiled route
    ("wide16", "fp32", 16, (7, 5), "big", (256, 8)),
]
CASE_IDS = ["%s-w%d-%dx%d-%s" % (c[0], c[2], c[3][0], c[3][1], c[4]) for c in CASES]


def wide32_geometry(H, W):
    """csrc/nf_wide.hip::dispatch_wide: (threads, tiles per image row); a wavefront owns a strip of 8 rows of one 32-pixel tile column."""
    if W <= 32:
        return (256, 1) if H <= 32 else (512, 1)
    return (512, 2) if H <= 32 else (1024, 2)


def wide16_geometry(H, W):
    """csrc/nf_wide16.hip::dispatch_wide16: (threads, rows per strip); a wavefront owns a strip of one 16-pixel column block."""
    s8 = ((H + 7) >> 3) * ((W + 15) >> 4)     # strips of 8 rows
    if s8 <= 4:
        return (256, 8)
    if s8 <= 8:
        return (512, 8)
    return (1024, 8) if s8 <= 16 else (1024, 16)


def test_every_case_reaches_the_geometry_it_names():
    """No GPU: the table's geometry column against the dispatchers' thread-count rule, and the facts the cases rely on."""
    for family, dtype, width, (H, W), kind, geo in CASES:
        assert (dtype == "fp16") == (family == "wide32h") and width <= (16 if family == "wide16" else 32), (family, dtype, width)
        if kind == "tiled":
            assert geo is None and (H > 64 or W > 64)
        else:
            assert (wide16_geometry if family == "wide16" else wide32_geometry)(H, W) == geo, (family, H, W)
    std = lambda fam: {c[5] for c in CASES if c[0] == fam and c[4] == "std"}
    assert std("wide32") == {(256, 1), (512, 1), (512, 2), (1024, 2)}
    assert std("wide32h") == {(256, 1), (512, 2), (1024, 2)}
    assert std("wide16") == {(256, 8), (512, 8), (1024, 8), (1024, 16)}
    assert ("wide32", "fp32", 32, (9, 31), "std", (256, 1)) in CASES and (9 + 7) // 8 == 2    # two strips in one tile column: `exch`
    assert ("wide16", "fp32", 16, (9, 33), "std", (512, 8)) in CASES and (33 + 15) >> 4 == 3   # three column blocks
    for family, has_big in (("wide32", True), ("wide32h", False), ("wide16", True)):
        kinds = [c[4] for c in CASES if c[0] == family]
        assert kinds.count("pc") == 1 and kinds.count("tiled") == 1 and kinds.count("big") == (1 if has_big else 0), family
    assert {c[2] for c in CASES if c[0] == "wide32"} == {24, 32} and {c[2] for c in CASES if c[0] == "wide16"} == {12, 16}


def _reduced(t):
    """First and last row of [B, H, W, 4], and per row the sum of its bit patterns."""
    bits = np.ascontiguousarray(t).view(np.uint32).astype(np.uint64)
    return {"rows": np.ascontiguousarray(t[:, [0, -1]]), "rowsum": bits.sum(axis=(2, 3))}


def case_outputs(case):
    """What the fixture holds of one case, from the library that is loaded: {name: array}."""
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from test_gpu_percond import _dev, _nll, _rows, _sample
    family, dtype, width, (H, W), kind, _ = case
    v = _variables(ARCH, width, seed=1000 * H + 10 * W + width)
    m = NoiseFlow([H, W, 4], False, default_hps(arch=ARCH, width=width), variables=v, cnn_dtype=dtype)
    want = {"wide32": _lib.NF_PATH_WIDE32, "wide32h": _lib.NF_PATH_WIDE32_FP16, "wide16": _lib.NF_PATH_WIDE16}[family]
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (case, direction)
    B = 2
    if kind == "big":
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        B = OCC_MAX * n_cu + 1
        assert n_cu * OCC_MAX < B
    x, y = make_inputs(B, H, W, seed=H + W)
    x, y = _dev(x), _dev(y)
    eps = _dev(np.random.RandomState(SEED).randn(B, H, W, 4).astype(np.float32))
    if kind == "pc":
        table = np.array([(i, c, 0, 0) for i, c in PC_TABLE], np.float32)
        kw0, kw1 = dict(rows=_rows(m, table, 0)), dict(rows=_rows(m, table, 1))
    else:
        kw0 = kw1 = dict(cond=_lib.nf_cond(ISO_CAM[0], ISO_CAM[1], 0.0, 0.0))
    nll, sd, ld, z = _nll(m, x, y, **kw0)
    if kind == "big":
        res = {"nll": nll[[0, B // 2, B - 1]]}
    else:
        res = {"nll": nll, "sd": sd, "logdet": ld}
        tensors = {"z": (z, 33 * 33), "x_eps": (_sample(m, y, eps, 0, **kw1), 512),
                   "x_philox": (_sample(m, y, None, BASE, seed=SEED, **kw1), 512)}
        for name, (t, full_up_to) in tensors.items():
            assert np.isfinite(t).all(), (case, name)
            if H * W <= full_up_to and max(H, W) <= 33:
                res[name] = t
            else:
                for k, a in _reduced(t).items():
                    res["%s_%s" % (name, k)] = a
    out = {}
    for name, a in res.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.uint64) and (a.dtype == np.uint64 or np.isfinite(a).all()), (case, name)
        out["%s__%s" % (CASE_IDS[CASES.index(case)], name)] = a
    return out


def compute_outputs():
    out = {}
    for case in CASES:
        out.update(case_outputs(case))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_wide_kernels_give_the_bits_of_the_stand_alone_kernels(case):
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
