"""CPU tier of the dyadic fp16-CNN probes (tests/fp16_probe.py): the conditions that make the GPU assertions of
tests/test_gpu_fp16_exact_probe.py meaningful.  No GPU is touched.

Per case x family x seed:
  * conditions — every addend of l_1, l_2 (and of l_last where bit equality is claimed) is a multiple of one unit u with
    sum |addends| <= 2^22 u per output element (exact in fp32 in any order, two spare bits for how a matrix instruction aligns
    its addends); no half operand is subnormal or overflows; `exact`: z0, relu(h1), relu(h2) are representable in half; `rounding`:
    >= 10 % of z0 are exact ties, relu(h1) and relu(h2) have ties and >= 25 % inexact roundings; 30 % .. 80 % of the hidden
    activations are alive after each ReLU; the distinct values of a family patch's shift are >= half its element count.  The
    population conditions are asserted on the two family patches and not at 1x1 (two pixels are no population).
  * l_last — `exact`: exact everywhere.  `rounding`: relu(h2) spans 2^-14 .. 2^13, one unit for a whole 3x3 window does not
    exist in general; the per-element condition (fp16_probe.l_last_exact_mask) holds on the impulse patches' background and on
    width 4, and bit equality is claimed exactly there.  Everywhere else — most of the `rounding` family patches of EVERY case —
    the shift is held to BOUND_U[width] * 2^-24 * A, A = test_gpu_split_bf16_probe.abs_terms: twice the worst distance from the
    fp64 chain of the oracle's float32 flavour of coupling_cnn_fp16 and of a sequential fp32 accumulation
    (fp16_probe.sequential_f32_l_last), capped at 4, two digits, recomputed here.
  * the library's fold (nf_fold_params, host only) of the probe variables lands on the design: weights rounded to half with
    numpy are the designed half values, biases and border table the designed fp32 values bit for bit (fl32(1 - BN_EPS) as the
    BN variance does it, as it does in the oracle); the oracle's fp64 and float32 flavours give identical bits wherever bit
    equality is claimed.
  * teeth — numpy mutants of the chain, each changing at least one element of EVERY patch of every case it applies to (a
    bit on a bit-exact element, or >= 2 x the bound on a bounded one): round-toward-zero and round-half-away at z0, relu(h1),
    relu(h2) (`rounding`), l_2 accumulated in half (`rounding`), one 3x3 tap of l_1 / of l_last dropped at every patch's own
    pixel (the impulse position = every listed seam, corner and edge midpoint; four pixels of each family patch, where a
    pixel whose hidden channels are all dead hides an l_1 tap from any test),
    two input channels of l_2 swapped inside the first block of 16 (`exact`), l_last's raw weights rounded before the
    2 log2(e) fold (raw probe; DROPPED on the two 1x1 cases, where only the centre tap's handful of weights act and
    their 2^-12 relative change is not 2 x the raw bound on every patch).  DROPPED: "a padded channel given a non-zero bias",
    on the five cases whose width pads (24, 48, 96, 200) — every
    layout writes zero OUTGOING weights for a padded channel (nf_host.hip: `cin < w ? ... : 0`), so its activation cannot reach
    the output whatever its bias; the fold test asserts instead that every padded slot of the exported block is zero.
  * raw probe — RAW_T = 9 by the rule of test_raw_probe_fp32_flavours_and_the_mutant_on_the_cpu (4 x the worst fp32 flavour in
    units of 2^-24 (1 + |ls|), the conv allowance taken off), the conv allowance ONE unit of 2^-24 A for the fp32 rounding of
    bias * 2 log2(e) (1 + BOUND_U where l_last is not exact); |ls| >= 0.05 on at least half of the elements.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fp16_probe as P
from test_gpu_split_bf16_probe import RAW_T, U24, abs_terms, raw_bound

# units of 2^-24 A on the elements of the `rounding` family where l_last is not exact; measured (float32 flavour / sequential):
# see test_bound_table_against_the_cpu_flavours
BOUND_U = {4: 0.06, 8: 0.053, 16: 0.039, 24: 0.034, 32: 0.061, 48: 0.018, 64: 0.061, 96: 0.092, 200: 0.079, 256: 0.074, 512: 0.087}
PRE_ROUNDED = "l_last's raw weights rounded before the 2 log2(e) fold"
DROPPED = {c[0]: ("padded channel given a non-zero bias", "its outgoing weights are zero in every layout: it cannot reach the output")
           for c in P.CASES if P.pads(c[2])}
DROPPED.update({c[0]: (PRE_ROUNDED, "one pixel: only the centre tap's handful of weights act, and their 2^-12 relative change is within twice "
                                    "the raw bound on some patches") for c in P.CASES if c[3] == (1, 1)})
WIDTHS = sorted({c[2] for c in P.CASES})


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=2)
def _data(case_id, name, seed):
    """Everything the tests of one case x family x seed share: inputs, the fp64 chain with its intermediates, the mask of
    bit-exact shift elements, A."""
    case = P.CASES[P.CASE_IDS.index(case_id)]
    width, hw = case[2], case[3]
    D = P.design(width, seed)
    pos = P.case_positions(case)
    z0 = P.probe_z0(D, name, hw, pos)
    I = {}
    shift = P.chain(D, z0, "shift", want=I)
    mask = P.l_last_exact_mask(I["a2"], I["abs3"], I["E"])
    v = P.variables(D, "shift")
    A = abs_terms(P.params64(v), z0)[..., :2]
    return {"case": case, "D": D, "pos": pos, "z0": z0, "I": I, "shift": shift, "mask": mask, "A": A, "v": v}


def bounded_ok(err, A, width):
    return np.abs(err) <= BOUND_U[width] * U24 * A


def _every_patch_moved(d, mutant, what):
    """The mutant's shift differs from the chain's on every patch: a bit-exact element changed, or a bounded one by 2 x bound."""
    moved = np.where(d["mask"], mutant != d["shift"], np.abs(mutant - d["shift"]) >= 2.0 * BOUND_U[d["case"][2]] * U24 * d["A"])
    per_patch = moved.reshape(moved.shape[0], -1).any(axis=1)
    assert per_patch.all(), (d["case"][0], what, "patches not moved:", np.flatnonzero(~per_patch).tolist())


def _own_pixels(d):
    H, W = d["case"][3]
    fam = [(b, r, c) for b in range(P.B_FAMILY) for r, c in dict.fromkeys([(0, 0), (H // 2, W // 2), (H - 1, W // 3), (H // 3, W - 1)])]
    return fam + [(P.B_FAMILY + b, r, c) for b, (r, c) in enumerate(d["pos"])]


# ---- conditions ------------------------------------------------------------------------------------------------------------------

def check_conditions(d, name):
    I, (H, W), width = d["I"], d["case"][3], d["case"][2]
    for k in ("z", "a1", "a2"):
        P.assert_half_normal(I[k], k)
    for k, pre in (("z", d["z0"].astype(np.float64)), ("a1", np.maximum(I["h1"], 0)), ("a2", np.maximum(I["h2"], 0))):
        P.assert_half_normal(pre, "unrounded " + k)
    W1, b1, W2, b2, W3, b3 = P.weights(d["D"], "shift")
    for k, a in (("W1", W1), ("W2", W2), ("W3", W3[:, :, :width]), ("W3 raw", P.weights(d["D"], "raw")[4][:, :, :width])):
        P.assert_half_normal(a, k)
        assert np.array_equal(a.astype(np.float16).astype(np.float64), a), k
    # one unit, 2^22 of it, per layer and element
    u1 = 2.0 ** (P.SZ[name] + P.S1) if name == "exact" else min(P.lowbit(I["z"]).min() * 2.0 ** P.S1, 2.0 ** P.SB1)
    assert min(P.lowbit(I["z"]).min() * 2.0 ** P.S1, 2.0 ** P.SB1) >= u1 and I["abs1"].max() <= 2.0 ** 22 * u1
    u2 = min(P.lowbit(I["a1"]).min() * 2.0 ** P.S2, 2.0 ** P.SB2)
    assert I["abs2"].max() <= 2.0 ** 22 * u2, (I["abs2"].max() / u2 / 2.0 ** 22)
    fam = slice(0, P.B_FAMILY)
    if name == "exact":
        assert u1 == 2.0 ** (P.SZ[name] + P.S1) and u2 == u1 * 2.0 ** P.S2
        for k, pre in (("z", d["z0"].astype(np.float64)), ("a1", np.maximum(I["h1"], 0)), ("a2", np.maximum(I["h2"], 0))):
            assert np.array_equal(I[k], pre), (k, "not representable in half")
        u3 = u2 * 2.0 ** P.S3
        assert min(P.lowbit(I["a2"]).min() * 2.0 ** P.S3, P.lowbit(I["E"]).min()) >= u3 and I["abs3"].max() <= 2.0 ** 22 * u3
        assert d["mask"].all()
        z1 = P.probe_z1(d["D"], name, "shift", d["z0"]).astype(np.float64)
        assert P.lowbit(z1).min() >= u3 and (np.abs(z1) + np.abs(d["shift"])).max() <= 2.0 ** 22 * u3 and np.all(z1 != 0)
    else:
        assert d["mask"][P.B_FAMILY:].mean() >= 0.5 or H * W < 64, "impulse backgrounds are bit-exact"
    if H * W == 1:
        return
    if name == "rounding":
        z64 = d["z0"][fam].astype(np.float64)
        ties = np.abs(P.round_half(z64, "rtz") - z64) == np.abs(P.round_half(z64, "rha") - z64)
        assert (ties & (I["z"][fam] != z64)).mean() >= 0.10
        for k, h in (("h1", I["h1"][fam]), ("h2", I["h2"][fam])):
            h = h[h > 0]
            lo, hi = P.round_half(h, "rtz"), P.round_half(h, "rha")
            assert np.any((h - lo == hi - h) & (lo != hi)), (k, "no ties")
            assert (P.round_half(h) != h).mean() >= 0.25, (k, (P.round_half(h) != h).mean())
    for k in ("h1", "h2"):
        alive = (I[k][fam] > 0).mean()
        assert 0.30 <= alive <= 0.80, (k, alive)
    for b in range(P.B_FAMILY):
        inner = d["shift"][b, 1:-1, 1:-1] if min(H, W) > 2 else d["shift"][b]
        assert len(np.unique(inner)) >= inner.size / 2, (b, len(np.unique(inner)), inner.size)


# ---- the library's fold, the oracle's flavours -------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", ["shift", "raw"])
@pytest.mark.parametrize("width", WIDTHS)
def test_fold_lands_on_the_design(width, half):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    for seed in P.SEEDS:
        D = P.design(width, seed)
        v = P.variables(D, half)
        W1, b1, W2, b2, W3, b3 = P.weights(D, half)
        layers, descs, flat = params.pack("unc", v, width, "loss_first", 1, "LU")
        for direction in (0, 1):
            cfg = _lib.nf_config(9, 33, 4, len(layers), -1, _lib.NF_CFG_FP16_CNN)
            ops = (C.c_int32 * 16)()
            n_ops, nf, ld = C.c_int32(), C.c_size_t(), C.c_double()
            blk = np.zeros(1 << 20, np.float32)
            _lib.check(lib.nf_fold_params(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, direction, ops, 8,
                                          C.byref(n_ops), blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(nf), C.byref(ld)))
            assert n_ops.value == 2 and ld.value == 0.0
            (mix,) = [ops[2 * i + 1] for i in range(2) if ops[2 * i] == _lib.NF_OP_MIX]
            (cpl,) = [ops[2 * i + 1] for i in range(2) if ops[2 * i] != _lib.NF_OP_MIX]
            assert np.array_equal(_bits(blk[mix:mix + 16]), _bits(np.eye(4).reshape(-1)))
            wk = P.layout_width(width)
            b = blk[cpl:]
            E = b[:64].reshape(16, 4)
            gW3 = b[64:64 + 36 * wk].reshape(9, wk, 4)
            o = 64 + 36 * wk
            gW1, gb1 = b[o:o + 18 * wk].reshape(9, 2, wk), b[o + 18 * wk:o + 19 * wk]
            o += 19 * wk
            gW2, gb2 = b[o:o + wk * wk].reshape(wk, wk), b[o + wk * wk:o + wk * wk + wk]
            assert b[o + wk * wk + wk] == np.float32(P.RESCALE)

            def padded(a, shape):
                out = np.zeros(shape)
                out[tuple(slice(0, n) for n in a.shape)] = a
                return out
            h16 = lambda a: np.asarray(a, np.float16).view(np.uint16)   # noqa: E731
            assert np.array_equal(h16(gW1), h16(padded(W1.reshape(9, 2, width), (9, 2, wk))))
            assert np.array_equal(h16(gW2), h16(padded(W2, (wk, wk))))
            want3 = padded(W3[:, :, :width].reshape(9, width, 4), (9, wk, 4))
            got3 = gW3.astype(np.float64)
            got3[..., 2:] *= P.K2                                       # nf_host.hip::to_half_w3: folded before the rounding
            assert np.array_equal(h16(got3), h16(want3))
            # every padded slot is zero, bit for bit: what "a padded channel that is not zero" would break
            assert not gW1[..., width:].any() and not gW2[width:].any() and not gW2[:, width:].any() and not gW3[:, width:].any()
            assert np.array_equal(_bits(gb1), _bits(padded(b1, (wk,)))) and np.array_equal(_bits(gb2), _bits(padded(b2, (wk,))))
            edge = W3[:, :, width, :]
            for m in range(16):
                out = [(di, dj) for di in range(3) for dj in range(3)
                       if (di == 0 and m & 1) or (di == 2 and m & 2) or (dj == 0 and m & 4) or (dj == 2 and m & 8)]
                want = b3 + sum(edge[di, dj] for di, dj in out)
                assert np.array_equal(_bits(E[m]), _bits(want)), (m, E[m], want)
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)


def check_oracle_flavours_agree_to_the_bit_where_bit_equality_is_claimed(d):
    from oracle.nf_oracle import coupling_cnn_fp16
    p = P.params64(d["v"])
    p32 = {k: np.asarray(a, np.float32) for k, a in p.items()}
    o64 = coupling_cnn_fp16(d["z0"].astype(np.float64), p)
    o32 = coupling_cnn_fp16(d["z0"], p32)
    assert not o64[1].any() and not o32[1].any()
    m = d["mask"]
    assert np.array_equal(o64[0][m], d["shift"][m]), "the oracle's fp64 flavour is not the unrounded chain"
    assert np.array_equal(_bits(o32[0])[m], _bits(d["shift"])[m])
    assert np.array_equal(_bits(P.sequential_f32_l_last(d["D"], d["I"]["a2"], d["I"]["E"]))[m], _bits(d["shift"])[m])
    assert bounded_ok(o32[0].astype(np.float64) - d["shift"], d["A"], d["case"][2])[~m].all()


@pytest.mark.parametrize("width", WIDTHS)
def test_bound_table_against_the_cpu_flavours(width):
    """BOUND_U[width] is what the rule gives: twice the worst distance, in units of 2^-24 A, of the two CPU fp32 flavours from
    the fp64 chain over the width's cases x seeds on the `rounding` family, two digits, capped at 4."""
    from oracle.nf_oracle import coupling_cnn_fp16
    from test_gpu_probe_families import _round_up_2_digits
    w_np = w_seq = 0.0
    for case in [c for c in P.CASES if c[2] == width]:
        for seed in P.SEEDS:
            d = _data(case[0], "rounding", seed)
            p32 = {k: np.asarray(a, np.float32) for k, a in P.params64(d["v"]).items()}
            o32 = coupling_cnn_fp16(d["z0"], p32)[0].astype(np.float64)
            seq = P.sequential_f32_l_last(d["D"], d["I"]["a2"], d["I"]["E"]).astype(np.float64)
            w_np = max(w_np, float((np.abs(o32 - d["shift"]) / (U24 * d["A"])).max()))
            w_seq = max(w_seq, float((np.abs(seq - d["shift"]) / (U24 * d["A"])).max()))
    rule = min(4.0, _round_up_2_digits(2.0 * max(w_np, w_seq)))
    print("\nwidth %d, units of 2^-24 A: float32 flavour %.3f, sequential fp32 %.3f -> rule gives %.2g, table %.2g"
          % (width, w_np, w_seq, rule, BOUND_U[width]))
    assert max(w_np, w_seq) <= BOUND_U[width] / 2 and BOUND_U[width] <= rule * (1 + 1e-9), (w_np, w_seq, rule)


# ---- teeth -----------------------------------------------------------------------------------------------------------------------

def check_rounding_mode_and_half_accumulation_mutants_move_every_patch(d):
    for k, where in enumerate(("z0", "relu h1", "relu h2")):
        for mode in ("rtz", "rha"):
            modes = tuple(mode if i == k else "rne" for i in range(3))
            _every_patch_moved(d, P.chain(d["D"], d["z0"], "shift", modes=modes), "%s at %s" % (mode, where))
    _every_patch_moved(d, P.chain(d["D"], d["z0"], "shift", l2_half=True), "l_2 accumulated in half")


def check_dropped_tap_mutants_move_every_patch(d):
    for layer in ("l_1", "l_last"):
        _every_patch_moved(d, P.chain(d["D"], d["z0"], "shift", drop=(layer, _own_pixels(d))), "a tap of %s dropped" % layer)


def check_swapped_k_lanes_of_l_2_move_every_patch(d):
    """Two input channels of l_2 exchanged inside the first block of 16: the first pair whose designed biases already differ
    after the ReLU (an impulse patch is mostly background) and whose columns of l_2 differ."""
    W1, b1, W2, b2, _, _ = P.weights(d["D"], "shift")
    n = min(16, d["case"][2])
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)
             if max(b1[i], 0) != max(b1[j], 0) and np.any(W2[i] != W2[j]) and np.any((W2[i] != 0) | (W2[j] != 0))]
    assert pairs
    last = None
    for pair in pairs[:8]:
        try:
            _every_patch_moved(d, P.chain(d["D"], d["z0"], "shift", swap=pair), "l_2 input channels %d, %d swapped" % pair)
            return
        except AssertionError as e:
            last = e
    raise last


# ---- raw probe -------------------------------------------------------------------------------------------------------------------

def raw_reference(d):
    """(ls, per-element bound, conv allowance) of the raw probe of _data's case in fp64."""
    D, z0 = d["D"], d["z0"]
    raw = P.chain(D, z0, "raw")
    p = P.params64(P.variables(D, "raw"))
    units = np.where(d["mask"], 1.0, 1.0 + BOUND_U[d["case"][2]])
    conv, bound, ls = raw_bound(p, abs_terms(p, z0)[..., 2:], raw, units)
    return ls, bound, conv


def check_raw_probe_tail_constant_and_the_pre_rounded_weights_mutant(d, name):
    from oracle.nf_oracle import NoiseFlowOracle, coupling_cnn_fp16
    D, z0 = d["D"], d["z0"]
    v = P.variables(D, "raw")
    ls, bound, conv = raw_reference(d)
    assert (np.abs(ls) >= 0.05).mean() >= 0.5, (np.abs(ls) >= 0.05).mean()
    o64 = coupling_cnn_fp16(z0.astype(np.float64), P.params64(v))
    assert not o64[0].any() and np.abs(P.RESCALE * np.tanh(o64[1]) - ls).max() <= 1e-13
    x = P.probe_x(D, name, "raw", z0)
    o32 = NoiseFlowOracle("unc", v, dtype=np.float32, cnn_dtype="fp16")
    inv, fwd = o32.inverse(x)[0], o32.forward(x)
    e = np.maximum(np.abs(np.log(inv[..., 2:].astype(np.float64)) - ls), np.abs(np.log(fwd[..., 2:].astype(np.float64)) + ls))
    t = float((np.maximum(e - conv, 0) / (U24 * (1 + np.abs(ls)))).max())
    print("raw probe: tanh / exp of the oracle's float32 flavour %.2f units of 2^-24 (1 + |ls|); RAW_T = %g" % (t, RAW_T))
    assert 4.0 * t <= RAW_T, t
    if name == "exact" and DROPPED.get(d["case"][0], ("",))[0] != PRE_ROUNDED:
        m_ls = P.RESCALE * np.tanh(P.chain(D, z0, "raw", w3_pre_round=True))
        moved = (np.abs(m_ls - ls) >= 2.0 * bound).reshape(ls.shape[0], -1).any(axis=1)
        assert moved.all(), np.flatnonzero(~moved).tolist()


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("name", P.FAMILIES)
@pytest.mark.parametrize("case_id", P.CASE_IDS)
def test_conditions_flavours_teeth_and_raw_tail(case_id, name, seed):
    """Everything the module docstring lists for one case x family x seed (one test: the checks share the chain's intermediates,
    hundreds of MB at the widest cases)."""
    d = _data(case_id, name, seed)
    check_conditions(d, name)
    check_oracle_flavours_agree_to_the_bit_where_bit_equality_is_claimed(d)
    check_dropped_tap_mutants_move_every_patch(d)
    if name == "rounding":
        check_rounding_mode_and_half_accumulation_mutants_move_every_patch(d)
    else:
        check_swapped_k_lanes_of_l_2_move_every_patch(d)
    check_raw_probe_tail_constant_and_the_pre_rounded_weights_mutant(d, name)


def test_dropped_table():
    """At most one mutant per case, never a rounding-mode one; the cases whose width pads and the two of one pixel."""
    assert sorted(DROPPED) == sorted(c[0] for c in P.CASES if c[2] in (24, 48, 96, 200) or c[3] == (1, 1))
    assert {m for m, _ in DROPPED.values()} <= {PRE_ROUNDED, "padded channel given a non-zero bias"}     # no rounding-mode mutant
