"""Probe models on every fp32 kernel family: the coupling CNN observed at fp32 resolution, the log-det per patch.

The probes, the yardstick A and the oracle are those of tests/test_gpu_split_bf16_probe.py (a one-coupling `unc` model whose
output IS the conv chain l_1 -> ReLU -> l_2 -> ReLU -> l_last: shift probe and raw probe, both directions); here they run at the
widths and patch shapes that reach the other kernels and their seams — CASES below: the width-4 matrix-core kernel off 32x32
(NF_PATH_MFMA4), the scalar-weight kernel (NF_PATH_SCALAR), nf_wide16_kernel (NF_PATH_WIDE16), nf_wide32_kernel (NF_PATH_WIDE32)
and both weight-delivery variants of the GEMM kernels (NF_PATH_GEMM).  Every GPU test asserts the kernel path in both directions.

Bound, shift probe, every element, both directions:   |kernel - oracle64| <= BOUND_UNITS[width] * 2^-24 * A.
The table is measured against the CPU oracles, never against a kernel: an entry is twice the worst distance from the fp64
chain of the two CPU fp32 evaluations of the same model — the numpy oracle's float32 flavour and the plain-C oracle, whose
sequential fp32 loops model an accumulation chain — over all of that width's shapes, input families and seeds, rounded up to two
significant digits and capped at the 4 units of the width-4 probe.  test_bound_table_against_the_cpu_oracles recomputes both
flavours and asserts that they stay within half the entry, so the constants are a checked condition.  A shrinks the units with the
width because it grows like the number of terms while round-off grows like its square root (numpy: pairwise / blocked sums) or, for
the sequential C loops, like a small multiple of it.

Teeth, widths <= 32 (where a split-bf16 kernel would land next): the same CPU test evaluates numpy mutants of the chain that run ONE
layer as "bf16 x 3" (hh, hm, mh; tests/test_gpu_split_bf16_probe.py::chain_emulated) — l_1 only, l_2 only, l_last only — and asserts
that on every input family the worst element over the seeds and that width's shapes is at least 2 x the bound.  Dropped
mutant / family pairs (at most one per width, never l_2 on lognormal) would be listed in DROPPED with their measured ratio; none
is.  Measured, the weakest pair per width in units of its bound: width 4 l_1 on bf16_exact 5.7, width 8 l_2 on impulse 4.7, width 16
l_1 on bf16_exact 3.1, width 32 l_1 on bf16_exact 2.05 (1.54 units against 2 x 0.75); l_2 on lognormal: 10.3 / 6.1 / 3.5 / 3.3.

Widths >= 64: the CPU test prints the ratio "l_2 as bf16 x 3 / bound" and asserts only that it is at least 1.  At these widths the
probe resolves per-element geometry (a wrong tap, a missed border, a seam), the log-det, and anything coarser than a three-product
split (measured: l_2 as bf16 x 3 is at 2.6 / 2.7 / 1.7 / 2.3 / 1.4 x the bound at widths 64 / 96 / 200 / 256 / 512).  It can NOT resolve a three-product split with margin: sequential fp32 accumulation over 9 x width terms (error ~ n) is
itself that close to one (error ~ sqrt n).  Nothing more is claimed.

Raw probe: log(out) within raw_bound (the conv bound mapped through tanh, plus RAW_T 2^-24 (1 + |ls|)); RAW_T = 9 holds at every
width by the rule of the width-4 module (4 x the worst fp32 flavour <= RAW_T; test_raw_t_against_the_cpu_oracles).  Per-patch
log-det within the sum of its elements' conv allowances plus GRAD_NOISE_C 2^-24 sum |ls| — at EVERY shape, the ragged ones above all:
a log-det that loses or double-counts one pixel's log-scales at a partial strip, a ragged column block or a band boundary moves by
|ls| of that pixel, 1e3 .. 1e5 times this allowance.

Impulse positions (one patch each): the four corners, the four edge midpoints, and one pixel either side of every seam the kernel
under test has at that shape — CASES names them, read from the kernels:
  * nf_flow_kernel, not 2x2-blocked (scalar weights at any shape, matrix cores off 32x32 / 64x64): pixel p belongs to thread
    p % THREADS, slot p / THREADS; THREADS = 64 up to 64 pixels, 256 up to 1024 (4 slots), 1024 beyond — "lin" seams at the
    wavefront boundary p = 64 and at every slot boundary p = k THREADS;
  * nf_flow_kernel, 2x2-blocked (matrix cores at 64x64): a lane owns a 2x2 block, a wavefront two block rows — row seams 2 and 4,
    column seam 2;
  * nf_wide16_kernel: column blocks of 16 pixels (seams 16, 32, 48), strips of 8 rows (16 once (H / 8) x (W / 16) > 16), lane
    group g owning rows row0 + 4 q + g (seam 4), the last partial strip;
  * nf_wide32_kernel: tiles of 32 pixels (column seam 32), strips of 8 rows, the last partial strip;
  * nf_gemmb_kernel (widths <= 128): linear tiles of 32 pixels, rounds of 256, thread stride 512, 8 pixels per thread beyond 2048;
  * nf_gemm_kernel (widths > 128): bands of 32768 / padded width linear pixels (128 at 256, 64 at 512), tiles of 32.

Measured on an MI355X: see the docstrings of the two GPU tests and DESIGN.md 2.
"""
import numpy as np
import pytest

from conftest import GRAD_NOISE_C
from test_gpu_split_bf16_probe import (RAW_T, THREE, U24, _params64, _units, abs_terms, chain_emulated, probe_input,
                                       probe_variables, raw_bound)
from test_split_bf16 import family

SEEDS = (11, 12)
B_FAMILY = 2

# units of 2^-24 A; the rule is in the module docstring, the measurement in test_bound_table_against_the_cpu_oracles
# measured (numpy float32 flavour / plain-C oracle, worst over the width's CASES x families x SEEDS): 4: 1.08 / 1.41, 8: 0.89 / 0.53,
# 16: 0.35 / 0.61, 32: 0.29 / 0.37, 64: 0.14 / 0.26, 96: 0.06 / 0.13, 200: 0.04 / 0.06, 256: 0.04 / 0.07, 512: 0.02 / 0.07
BOUND_UNITS = {4: 2.9, 8: 1.8, 16: 1.3, 32: 0.75, 64: 0.53, 96: 0.27, 200: 0.12, 256: 0.15, 512: 0.14}
DROPPED = {}      # width -> (mutant, family, measured ratio to 2 x bound)

# (path, width, (H, W), row seams, column seams, linear-pixel seams)
CASES = [
    ("MFMA4", 4, (64, 64), (2, 4), (2,), ()),
    ("MFMA4", 4, (20, 28), (), (), (64, 256, 512)),
    ("MFMA4", 4, (33, 31), (), (), (64, 256, 512, 768)),
    ("MFMA4", 4, (1, 1), (), (), ()),
    ("SCALAR", 8, (32, 32), (), (), (64, 256, 512, 768)),
    ("SCALAR", 8, (20, 28), (), (), (64, 256, 512)),
    ("SCALAR", 8, (7, 5), (), (), ()),
    ("WIDE16", 16, (17, 16), (4, 8, 16), (), ()),
    ("WIDE16", 16, (9, 33), (4, 8), (16, 32), ()),
    ("WIDE16", 16, (33, 64), (4, 16, 32), (16, 32, 48), ()),
    ("WIDE16", 16, (1, 1), (), (), ()),
    ("WIDE32", 32, (9, 33), (8,), (32,), ()),
    ("WIDE32", 32, (33, 64), (8, 32), (32,), ()),
    ("WIDE32", 32, (64, 33), (8, 56), (32,), ()),
    ("WIDE32", 32, (1, 1), (), (), ()),
    ("WIDE32", 8, (60, 64), (8, 56), (32,), ()),
    ("GEMM", 64, (9, 33), (), (), (32, 256)),
    ("GEMM", 64, (33, 31), (), (), (32, 256, 512, 992)),
    ("GEMM", 64, (64, 64), (), (), (32, 256, 512, 2048, 4064)),
    ("GEMM", 96, (9, 33), (), (), (32, 256)),
    ("GEMM", 96, (33, 31), (), (), (32, 256, 512, 992)),
    ("GEMM", 256, (9, 33), (), (), (32, 128, 256)),
    ("GEMM", 256, (1, 1), (), (), ()),
    ("GEMM", 512, (9, 33), (), (), (32, 64, 256)),
    ("GEMM", 512, (1, 1), (), (), ()),
    ("GEMM", 200, (7, 5), (), (), (32,)),
]
CASE_IDS = ["%s-w%d-%dx%d" % (c[0].lower(), c[1], c[2][0], c[2][1]) for c in CASES]
WIDTHS = sorted({c[1] for c in CASES})


def families_of(width):
    """lognormal, wide_range, impulse everywhere; the bf16 families where a future split kernel would land."""
    return ("lognormal", "bf16_ties", "bf16_exact", "impulse", "wide_range") if width <= 32 else ("lognormal", "impulse", "wide_range")


def impulse_positions(hw, rows=(), cols=(), lin=()):
    """Corners, edge midpoints, and the pixel either side of every row seam (at the middle column), column seam (at the middle
    row) and linear-pixel seam of the case; duplicates (small shapes) removed, order kept."""
    H, W = hw
    rm, cm = H // 2, W // 2
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, cm), (H - 1, cm), (rm, 0), (rm, W - 1)]
    for r in rows:
        assert 0 < r < H, (hw, r)
        pos += [(r - 1, cm), (r, cm)]
    for c in cols:
        assert 0 < c < W, (hw, c)
        pos += [(rm, c - 1), (rm, c)]
    for p in lin:
        assert 0 < p < H * W, (hw, p)
        pos += [((p - 1) // W, (p - 1) % W), (p // W, p % W)]
    return list(dict.fromkeys(pos))


def case_input(case, name, seed):
    _, width, hw, rows, cols, lin = case
    return family(name, seed, B=B_FAMILY, hw=hw, impulses=impulse_positions(hw, rows, cols, lin))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_family_and_probe_variables_defaults_are_unchanged():
    """family() and probe_variables() grew a shape / impulse / width parameter; with the defaults they must return, byte for
    byte, what they returned before (the committed fixture tests/golden/split_bf16_bits.npz and every 32x32 test depend on it).
    `old_family` is the previous function, verbatim."""
    from conftest import trained_like_variables
    from oracle.nf_oracle import conv1x1_variable_names
    from test_split_bf16 import FAMILIES, IMPULSES, _bf16

    def old_family(name, seed, B=8, channels=2):
        rng = np.random.RandomState(100 * seed + FAMILIES.index(name))
        shape = (B, 32, 32, channels)
        if name == "lognormal":
            return (rng.randn(*shape) * np.exp(rng.randn(*shape))).astype(np.float32)
        if name == "bf16_ties":
            hi = (rng.randn(*shape) * np.exp(rng.randn(*shape))).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
            low = np.asarray([0x8000, 0x7FFF, 0x8001, 0x0080, 0x007F, 0x0081, 0x8080, 0x807F, 0x7F80, 0xFF80], np.uint32)
            return (hi | low[rng.randint(len(low), size=shape)]).view(np.float32)
        if name == "bf16_exact":
            z = _bf16((rng.randn(*shape) * np.exp(rng.randn(*shape))).astype(np.float32)).copy()
            k = rng.randint(5, size=shape)
            z[k == 0] = 0.0
            z[k == 1] = -0.0
            return z
        if name == "impulse":
            z = np.zeros((len(IMPULSES), 32, 32, channels), np.float32)
            for b, (r, c) in enumerate(IMPULSES):
                z[b, r, c] = (rng.randn(channels) * 3.0).astype(np.float32)
            return z
        return (np.sign(rng.randn(*shape)) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)).astype(np.float32)

    for name in FAMILIES:
        for seed, kw in ((3, {}), (11, {}), (4, {"channels": 4}), (12, {"B": 3})):
            a, b = family(name, seed, **kw), old_family(name, seed, **kw)
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, seed, kw)
    for half in ("shift", "raw"):
        v = probe_variables(7, half)
        old = trained_like_variables("unc", 4, seed=7)
        n = conv1x1_variable_names(0, "LU")
        old[n["P"]] = np.eye(4, dtype=np.float32)
        old[n["sign_S"]] = np.ones(4, np.float32)
        old[n["log_S"]] = np.zeros(4, np.float32)
        old[n["L_vec"]] = np.zeros_like(old[n["L_vec"]])
        old[n["U_vec"]] = np.zeros_like(old[n["U_vec"]])
        dead = slice(2, 4) if half == "shift" else slice(0, 2)
        for k in ("l_last/W", "l_last/b"):
            a = old["model/real_nvp_conv_template/" + k].copy()
            a[..., dead] = 0.0
            old["model/real_nvp_conv_template/" + k] = a
        assert sorted(v) == sorted(old)
        for k in v:
            assert np.asarray(v[k]).tobytes() == np.asarray(old[k]).tobytes(), (half, k)


def test_impulse_positions_cover_corners_midpoints_and_both_sides_of_every_seam():
    for case in CASES:
        _, _, (H, W), rows, cols, lin = case
        pos = impulse_positions((H, W), rows, cols, lin)
        assert len(set(pos)) == len(pos) and all(0 <= r < H and 0 <= c < W for r, c in pos)
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)} <= set(pos)
        for p in lin:
            assert divmod(p - 1, W) in pos and divmod(p, W) in pos
        z = case_input(case, "impulse", 11)
        assert z.shape == (len(pos), H, W, 2)
        assert all(np.count_nonzero(np.abs(z[b]).sum(-1)) == 1 and np.abs(z[b, r, c]).sum() > 0 for b, (r, c) in enumerate(pos))


def _round_up_2_digits(x):
    from math import ceil, floor, log10
    e = floor(log10(x)) - 1
    return ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


@pytest.mark.parametrize("width", WIDTHS)
def test_bound_table_against_the_cpu_oracles(width):
    """Per width, over its shapes x families x seeds, in units of 2^-24 A from the fp64 chain: the oracle's float32 flavour and
    the plain-C oracle (both must stay within BOUND_UNITS / 2, and the entry must be what the rule of the module docstring gives),
    and the three-product mutants (widths <= 32: each >= 2 x bound on every family; beyond: l_2's >= the bound)."""
    from oracle.nf_oracle import coupling_cnn
    from oracle.nf_oracle_c import COracle
    bound = BOUND_UNITS[width]
    w_np = w_c = 0.0
    muts = {}       # (mutant, family) -> worst over seeds and shapes
    for case in [c for c in CASES if c[1] == width]:
        for name in families_of(width):
            for seed in SEEDS:
                v = probe_variables(seed, "shift", width)
                p = _params64(v)
                p32 = {k: np.asarray(a, np.float32) for k, a in p.items()}
                z0 = case_input(case, name, seed)
                A = abs_terms(p, z0)[..., :2]
                ref = coupling_cnn(z0.astype(np.float64), p)[0]
                u_np = _units(coupling_cnn(z0, p32)[0].astype(np.float64) - ref, A)
                zc = COracle("unc", v).nll(probe_input(z0, "shift"), want_z=True)[2]
                u_c = _units(zc[..., 2:].astype(np.float64) - ref, A)
                w_np, w_c = max(w_np, u_np), max(w_c, u_c)
                which = (("l_1", (THREE, None, None)), ("l_2", (None, THREE, None)), ("l_last", (None, None, THREE)))
                for tag, (p1, p2, p3) in which if width <= 32 else which[1:2]:
                    u = _units(chain_emulated(p, z0, p1, p3, p2)[0] - ref, A)
                    muts[tag, name] = max(muts.get((tag, name), 0.0), u)
    rule = min(4.0, _round_up_2_digits(2.0 * max(w_np, w_c)))
    print("\nwidth %d, units of 2^-24 A: fp32 flavour (numpy) %.3f, plain-C oracle %.3f -> rule gives %.2g, table %.2g"
          % (width, w_np, w_c, rule, bound))
    for (tag, name), u in sorted(muts.items()):
        print("  width %d: %s as bf16 x 3 on %s: %.2f units = %.2f x bound" % (width, tag, name, u, u / bound))
    assert max(w_np, w_c) <= bound / 2, (w_np, w_c)
    assert bound <= rule * (1 + 1e-9), (bound, rule)       # the table is never wider than its rule gives
    for (tag, name), u in muts.items():
        if DROPPED.get(width, ("", ""))[:2] == (tag, name):
            continue
        assert u >= (2.0 if width <= 32 else 1.0) * bound, (width, tag, name, u)
    assert DROPPED.get(width, ("", ""))[:2] != ("l_2", "lognormal")


@pytest.mark.parametrize("width", WIDTHS)
def test_raw_t_against_the_cpu_oracles(width):
    """RAW_T per width, by the rule of tests/test_gpu_split_bf16_probe.py: tanh / exp of the two fp32 flavours in units of
    2^-24 (1 + |ls|), the conv allowance (this width's bound) taken off, x 4 for hardware exp2 / rcp, must not exceed it."""
    from oracle.nf_oracle import NoiseFlowOracle, coupling_cnn
    from oracle.nf_oracle_c import COracle
    t_np = t_c = 0.0
    for case in [c for c in CASES if c[1] == width]:
        for name in families_of(width):
            for seed in SEEDS:
                v = probe_variables(seed, "raw", width)
                p = _params64(v)
                z0 = case_input(case, name, seed)
                x = probe_input(z0, "raw")
                raw64 = coupling_cnn(z0.astype(np.float64), p)[1]
                conv, _, ls = raw_bound(p, abs_terms(p, z0)[..., 2:], raw64, BOUND_UNITS[width])
                o32 = NoiseFlowOracle("unc", v, dtype=np.float32)
                oc = COracle("unc", v)
                for k, (inv, fwd) in (("np", (o32.inverse(x)[0], o32.forward(x))), ("c", (oc.nll(x, want_z=True)[2], oc.sample(x, 1.0)))):
                    e = np.maximum(np.abs(np.log(inv[..., 2:].astype(np.float64)) - ls), np.abs(np.log(fwd[..., 2:].astype(np.float64)) + ls))
                    t = float((np.maximum(e - conv, 0) / (U24 * (1 + np.abs(ls)))).max())
                    if k == "np":
                        t_np = max(t_np, t)
                    else:
                        t_c = max(t_c, t)
    print("\nwidth %d raw probe: tanh / exp of the fp32 flavour %.2f, of the plain-C oracle %.2f units of 2^-24 (1 + |ls|); RAW_T = %g"
          % (width, t_np, t_c, RAW_T))
    assert 4.0 * max(t_np, t_c) <= RAW_T, (t_np, t_c)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

_ARGS = ([0.0], [0.0], [100], [0])


def _model(case, v):
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    path, width, (H, W) = case[:3]
    m = NoiseFlow([H, W, 4], False, default_hps(arch="unc", width=width), variables=v)
    want = getattr(_lib, "NF_PATH_" + path)
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (case[:3], direction)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_shift_probe_kernel_within_the_widths_bound_of_the_fp64_chain(case, seed):
    """Every shift element within BOUND_UNITS[width] 2^-24 A in both directions, the pass-through half bit-identical, the
    log-det exactly zero.

    Measured on an MI355X, worst element per path over its shapes x families x 2 seeds, units of 2^-24 A (bound), the same in both
    directions: MFMA4 width 4 1.22 (2.9) — the 12th impulse of seed 12 (pixel 256 of 20x28, (8, 8) of 33x31, (4, 32) of 64x64: an impulse's
    figure goes with the drawn value, the same at every interior position); SCALAR width 8 0.46 (1.8) — impulse in the corner
    (0, W-1), every shape; WIDE16 0.27 (1.3) — impulse at the left edge midpoint (H / 2, 0), every shape;
    WIDE32 width 32 0.16 (0.75) — bf16_exact at 33x64, width 8 padded onto it 0.36 (1.8) — wide_range at 60x64; GEMM with
    LDS-resident weights 0.10 at width 64 (0.53), 0.08 at 96 (0.27) — impulses; with streamed weights 0.04 at 256 (0.15) — impulse at
    (8, 32) of 9x33, 0.03 at 512 (0.14), 0.02 at 200 (0.12).  No kernel came beyond 42 % of its bound."""
    from oracle.nf_oracle import coupling_cnn
    width = case[1]
    v = probe_variables(seed, "shift", width)
    p = _params64(v)
    m = _model(case, v)
    lines, bad = [], []
    for name in families_of(width):
        z0 = case_input(case, name, seed)
        x = probe_input(z0, "shift")
        A = abs_terms(p, z0)[..., :2]
        ref = coupling_cnn(z0.astype(np.float64), p)[0]
        z, obj = m.inverse(x, None, None, *_ARGS)
        xs = m.forward(x, None, None, *_ARGS)
        for tag, out, want in (("inverse", z, ref), ("forward", xs, -ref)):
            out = np.asarray(out)
            assert np.array_equal(out[..., :2], z0), (name, tag, "the pass-through half changed")
            u = np.abs(out[..., 2:].astype(np.float64) - want) / (U24 * A)
            at = np.unravel_index(np.argmax(u), u.shape)
            lines.append("PROBE shift %s %s %s seed %d: worst %.3f units of 2^-24 A (bound %g) at (patch, row, col, ch) = %s"
                         % (CASE_IDS[CASES.index(case)], name, tag, seed, u.max(), BOUND_UNITS[width], tuple(int(i) for i in at)))
            if not u.max() <= BOUND_UNITS[width]:
                bad.append(lines[-1])
        assert np.all(np.asarray(obj) == 0.0), (name, "ls = 0 exactly: the log-det must be zero")
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_raw_probe_kernel_log_scale_and_log_det(case, seed):
    """log(out) = +-ls per element within raw_bound at this width's conv bound; the per-patch log-det within the sum of its
    elements' conv allowances plus GRAD_NOISE_C 2^-24 sum |ls|.

    Measured on an MI355X: per element at most 0.20 of the bound on every path (MFMA4 at 64x64 and WIDE32 at 64x33, lognormal); the
    log-det at most 0.14 of its allowance at every shape with more than one pixel (WIDE32 at 64x33, impulse) and 0.32 at 1x1 (two
    terms: WIDE16 and GEMM width 256, lognormal)."""
    from oracle.nf_oracle import coupling_cnn
    width = case[1]
    v = probe_variables(seed, "raw", width)
    p = _params64(v)
    m = _model(case, v)
    lines, bad = [], []
    for name in families_of(width):
        z0 = case_input(case, name, seed)
        x = probe_input(z0, "raw")
        raw64 = coupling_cnn(z0.astype(np.float64), p)[1]
        conv, bound, ls = raw_bound(p, abs_terms(p, z0)[..., 2:], raw64, BOUND_UNITS[width])
        z, obj = m.inverse(x, None, None, *_ARGS)
        xs = m.forward(x, None, None, *_ARGS)
        for tag, out, want in (("inverse", z, ls), ("forward", xs, -ls)):
            out = np.asarray(out)
            assert np.array_equal(out[..., :2], z0), (name, tag, "the pass-through half changed")
            r = np.abs(np.log(out[..., 2:].astype(np.float64)) - want) / bound
            at = np.unravel_index(np.argmax(r), r.shape)
            lines.append("PROBE raw %s %s %s seed %d: worst %.3f of the bound at %s"
                         % (CASE_IDS[CASES.index(case)], name, tag, seed, r.max(), tuple(int(i) for i in at)))
            if not r.max() <= 1.0:
                bad.append(lines[-1])
        ld_ref = ls.sum(axis=(1, 2, 3))
        ld_tol = conv.sum(axis=(1, 2, 3)) + GRAD_NOISE_C * U24 * np.abs(ls).sum(axis=(1, 2, 3))
        ld_err = np.abs(np.asarray(obj, np.float64) - ld_ref)
        lines.append("PROBE log-det %s %s seed %d: worst %.3f of its allowance"
                     % (CASE_IDS[CASES.index(case)], name, seed, (ld_err / ld_tol).max()))
        if not np.all(ld_err <= ld_tol):
            bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
