"""The four GEMM coupling kernels (csrc/nf_gemm.hip: nf_gemm_kernel, nf_gemmb_kernel; csrc/nf_gemm16.hip: nf_gemm16_kernel,
nf_gemm16b_kernel) share code through csrc/nf_gemm_common.h: nf_gemmb_kernel and nf_gemm16_kernel their frame (patch loop, op
interpreter, epilogue), the 9-tap gather of the P records, the P-record store, the bias fill and the publication of the pass-through
half; all four the per-pixel helpers (since then in csrc/nf_flow_common.h, which the width-16 / 32 kernels use too:
tests/test_gpu_wide_bits.py) and the launcher.  Moving those from four copies into one
changed no product, no addition order and no rounding point, so every per-patch output is bit for bit what the four stand-alone
kernels gave: tests/golden/gemm_family_bits.npz was recorded with tools/make_golden_gemm_bits.py on an MI355X from the build of
commit 55960a5, the last one with the four copies.  array_equal on the uint32 views; a differing bit is an expression that was
reordered while moving, not a tolerance question.

Per-patch outputs only — NLL, sd_z, log-det, latents, samples from a supplied epsilon and from the in-kernel Philox draw; batch
sums and mean losses are added by device atomics in arrival order and are not recorded.  Model and inputs: `sdn5|unc|gain4|unc` and
`_variables` of tests/test_gpu_gemm.py, fixed seeds, B = 2 unless the case says otherwise.

CASES are the smallest shapes at which each shared helper can go wrong, per kernel: a partial round / ragged bands, each pixels-
per-thread count (OWN 2 / 4 / 8), the bordered and the bare pass-through tile of nf_gemm_kernel, both halves of nf_gemm16_kernel's
P stage (two bands of 128 pixels at width 512), the band kernels at width 64 under NF_GEMM=a / NF_GEMM16=a (nf_kernel_path does
not tell the variants apart, so these cases also run the model without the switch: in fp16 the latents agree but not bit for bit,
which shows that the switch was read; in fp32 at width 64 the two variants give the same bits), and per kernel one
case each of per-patch conditioning (the PC = true instantiation), an 80x100 image (NF_K_TILED through flow_tile and the epilogue's
tile share) and a batch larger than the CU count at 7x5 (the persistent loop takes a second patch through the frame; the NLL of
the first, a middle and the last patch is kept).

What the fixture keeps (it has to stay under 512 KiB): the scalars of every patch; latents in full up to 33x33, samples in
full up to 512 pixels; of every other tensor the first and the last row plus, per row, the sum of the rows'
uint32 bit patterns (so a changed bit anywhere in the tensor still shows)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import make_inputs
from test_gpu_gemm import ARCH, _variables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_family_bits.npz")
LDS_MAX = 160 * 1024
GT, GW, P_STRIDE, BAND_FLOATS = 512, 8, 44, 32768      # csrc/nf_gemm.hip, nf_device.h (NF7_P_STRIDE, NF7_BAND_FLOATS)
SEED, BASE = 20250412, 17
B_BIG = 300                                           # > the 256 CUs of an MI355X: one workgroup per CU, so some take a second patch
KEEP = (0, B_BIG // 2, B_BIG - 1)
ISO_CAM = (100.0, 2.0)
PC_TABLE = ((100.0, 2.0), (800.0, 0.0))               # per-patch conditioning: one (ISO, camera) per patch

# (kernel, cnn_dtype, width, (H, W), kind, env)   kind: std | pc | tiled | big;   env: the A/B switch set before nf_create
CASES = [
    # fp32 variant B (weights resident in LDS)
    ("gemmb", "fp32", 64, (7, 5), "std", None),          # one partial round
    ("gemmb", "fp32", 128, (17, 19), "std", None),       # two rounds, ragged
    ("gemmb", "fp32", 96, (33, 33), "std", None),        # 96 -> 128, OWN 4
    ("gemmb", "fp32", 64, (46, 47), "std", None),        # OWN 8
    # fp32 variant A (band, weights streamed from L2)
    ("gemm", "fp32", 512, (9, 13), "std", None),         # two bands of 64, ragged
    ("gemm", "fp32", 256, (33, 31), "std", None),
    ("gemm", "fp32", 200, (40, 30), "std", None),        # 200 -> 256, OWN 4
    ("gemm", "fp32", 512, (46, 47), "std", None),        # OWN 8, bordered tile
    ("gemm", "fp32", 128, (64, 64), "std", None),        # the slabs do not fit: variant A with the bare tile (BRD = false)
    ("gemm", "fp32", 64, (32, 32), "std", "NF_GEMM"),
    # fp16 variant A
    ("gemm16", "fp16", 512, (11, 13), "std", None),      # two bands of 128: both halves of the P stage, the record index map
    ("gemm16", "fp16", 256, (33, 31), "std", None),
    ("gemm16", "fp16", 512, (64, 64), "std", None),      # OWN 8
    ("gemm16", "fp16", 64, (32, 32), "std", "NF_GEMM16"),
    # fp16 variant B
    ("gemm16b", "fp16", 64, (7, 5), "std", None),        # one partial round
    ("gemm16b", "fp16", 128, (33, 33), "std", None),     # OWN 4
    ("gemm16b", "fp16", 96, (64, 40), "std", None),      # OWN 8
    # per kernel: per-patch conditioning, an image beyond 64x64, a batch beyond the CU count
    ("gemmb", "fp32", 64, (7, 5), "pc", None), ("gemm", "fp32", 256, (7, 5), "pc", None),
    ("gemm16", "fp16", 256, (7, 5), "pc", None), ("gemm16b", "fp16", 64, (7, 5), "pc", None),
    ("gemmb", "fp32", 64, (80, 100), "tiled", None), ("gemm", "fp32", 256, (80, 100), "tiled", None),
    ("gemm16", "fp16", 256, (80, 100), "tiled", None), ("gemm16b", "fp16", 64, (80, 100), "tiled", None),
    ("gemmb", "fp32", 64, (7, 5), "big", None), ("gemm", "fp32", 256, (7, 5), "big", None),
    ("gemm16", "fp16", 256, (7, 5), "big", None), ("gemm16b", "fp16", 64, (7, 5), "big", None),
]
CASE_IDS = ["%s-w%d-%dx%d-%s%s" % (c[0], c[2], c[3][0], c[3][1], c[4], "-a" if c[5] else "") for c in CASES]


def pad_width(width):
    return next(w for w in (64, 128, 256, 512) if width <= w)


def gemmb_lds_bytes(wp, H, W):
    """csrc/nf_gemm.hip::gemmb_lds_bytes: the slabs, the round's P records, the bordered two-plane tile, the reduction scratch."""
    plane = ((H + 2) * (W + 2) + 3) & ~3
    return ((wp // 32) * (32 * wp + 1024 + 128 + 32) + 32 * GW * P_STRIDE + 2 * plane + 3 * GW + 8) * 4


def gemm_lds_bytes(H, W, bordered):
    """csrc/nf_gemm.hip::gemm_lds_bytes: the band and the two-plane tile; the bare tile shares the band for its scratch."""
    plane = (((H + 2) * (W + 2) if bordered else H * W) + 3) & ~3
    return (BAND_FLOATS + 2 * plane + (3 * GW + 8 if bordered else 0)) * 4


def gemm16b_lds_bytes(wp, H, W):
    """csrc/nf_gemm16.hip::gemm16b_lds_bytes: the slabs (dwords of packed halves), the P records, the half2 tile, the scratch."""
    plane = ((H + 2) * (W + 2) + 3) & ~3
    return ((wp // 32) * ((wp // 16) * 256 + 512 + 64 + 32) + 32 * GW * P_STRIDE + plane + 3 * GW + 8) * 4


def kernel_of(dtype, width, hw, env):
    """The kernel nf_create picks (nf_host.hip): variant B at widths <= 128 (fp32: where its slabs fit), unless the switch says a."""
    wp = pad_width(width)
    H, W = min(hw[0], 64), min(hw[1], 64)      # images beyond 64x64 run as tiles of at most 64x64
    if dtype == "fp16":
        assert wp > 128 or gemm16b_lds_bytes(wp, H, W) <= LDS_MAX      # nf_host.hip picks it by width alone: it always fits
        return "gemm16b" if wp <= 128 and not env else "gemm16"
    return "gemmb" if wp <= 128 and gemmb_lds_bytes(wp, H, W) <= LDS_MAX and not env else "gemm"


def test_every_case_names_the_kernel_the_library_picks():
    """No GPU: the table's kernel column against the selection rule and the LDS formulas, and the facts the cases rely on."""
    for kernel, dtype, width, hw, kind, env in CASES:
        assert kernel_of(dtype, width, hw, env) == kernel, (kernel, dtype, width, hw, env)
    # width 128 at 64x64: the slabs do not fit beside the tile, and neither does the bordered tile beside the band
    assert gemmb_lds_bytes(128, 64, 64) > LDS_MAX
    assert gemm_lds_bytes(64, 64, True) > LDS_MAX >= gemm_lds_bytes(64, 64, False)
    assert gemm_lds_bytes(46, 47, True) <= LDS_MAX          # "OWN 8, bordered tile"
    for kernel in ("gemmb", "gemm", "gemm16", "gemm16b"):
        kinds = [c[4] for c in CASES if c[0] == kernel]
        assert all(kinds.count(k) == 1 for k in ("pc", "tiled", "big")), kernel


@contextlib.contextmanager
def _switch(env):
    """NF_GEMM=a / NF_GEMM16=a while the model is created (read at nf_create)."""
    old = {k: os.environ.get(k) for k in ("NF_GEMM", "NF_GEMM16")}
    for k in old:
        os.environ.pop(k, None)
    if env:
        os.environ[env] = "a"
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _reduced(t):
    """First and last row of [B, H, W, 4], and per row the sum of its bit patterns."""
    bits = np.ascontiguousarray(t).view(np.uint32).astype(np.uint64)
    return {"rows": np.ascontiguousarray(t[:, [0, -1]]), "rowsum": bits.sum(axis=(2, 3))}


def case_outputs(case):
    """What the fixture holds of one case, from the library that is loaded: {name: array}."""
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from test_gpu_percond import _dev, _nll, _rows, _sample
    kernel, dtype, width, (H, W), kind, env = case
    v = _variables(ARCH, width, seed=1000 * H + 10 * W + width)
    with _switch(env):
        m = NoiseFlow([H, W, 4], False, default_hps(arch=ARCH, width=width), variables=v, cnn_dtype=dtype)
    want = _lib.NF_PATH_GEMM_FP16 if dtype == "fp16" else _lib.NF_PATH_GEMM
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (case, direction)
    if (kernel, width, (H, W)) == ("gemm", 128, (64, 64)):     # the library's own predicate, not only its restatement above
        ok = getattr(m._flow.lib, "_Z17nf_gemmb_shape_okiii")
        ok.restype, ok.argtypes = C.c_bool, [C.c_int] * 3
        assert not ok(128, 64, 64) and ok(64, 64, 64)
    B = B_BIG if kind == "big" else 2
    if kind == "big":
        assert torch.cuda.get_device_properties(0).multi_processor_count < B
    x, y = make_inputs(B, H, W, seed=H + W)
    x, y = _dev(x), _dev(y)
    eps = _dev(np.random.RandomState(SEED).randn(B, H, W, 4).astype(np.float32))
    if kind == "pc":
        table = np.array([(i, c, 0, 0) for i, c in PC_TABLE], np.float32)
        kw0, kw1 = dict(rows=_rows(m, table, 0)), dict(rows=_rows(m, table, 1))
    else:
        kw0 = kw1 = dict(cond=_lib.nf_cond(ISO_CAM[0], ISO_CAM[1], 0.0, 0.0))
    nll, sd, ld, z = _nll(m, x, y, **kw0)
    if env:     # against the same model without the switch (variant B)
        mb = NoiseFlow([H, W, 4], False, default_hps(arch=ARCH, width=width), variables=v, cnn_dtype=dtype)
        zb = _nll(mb, x, y, **kw0)[3]
        if dtype == "fp16":     # the fp16 variants associate their sums differently: close, and not the same bits — the switch was read
            np.testing.assert_allclose(zb, z, rtol=0, atol=2e-3 * np.abs(z).max())
            assert not np.array_equal(zb.view(np.uint32), z.view(np.uint32)), (case, "NF_GEMM16=a did not change the kernel")
        else:                   # fp32 at width 64 (one wavefront along the channels): both variants add the same terms in the same
            #                     order, so the bits agree and cannot tell whether the switch was read
            assert np.array_equal(zb.view(np.uint32), z.view(np.uint32)), case
    if kind == "big":
        res = {"nll": nll[list(KEEP)]}
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
def test_gemm_kernels_give_the_bits_of_the_four_stand_alone_kernels(case):
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
