"""What gives the bound of tests/test_gpu_train_mm.py its meaning — on the CPU, no kernel involved.

That file launches the trainer's matrix-core GEMMs (csrc/nf_train_mm.h: `k_mm_pix` as exact fp32 and as "bf16 x 6" on 8 and on 4
wavefronts, `k_mm_kpix` / `k_mm_kpix6`) directly and holds every output element to

    |kernel - ref64| <= U_B * 2^-24 * T,      T = the fp64 sum of the magnitudes of every term that reaches the element.

This module owns the cases, the inputs, the fp64 references and the yardstick T, and derives U_B and U_S:

* U_B = twice the worst distance, in units of 2^-24 T, of a PLAIN numpy float32 evaluation of the same product (prologue, product,
  epilogue all in float32) from the fp64 one, over every case, family and seed with K <= 132, rounded up to an integer.  The factor 2
  covers another summation order.  Measured (test_plain_fp32_and_six_products_within_half_the_bound prints the table): per family,
  worst over the cases, lognormal 11.2, bf16_ties 12.2, bf16_exact 7.5, impulse 6.0, wide_range 15.36 — hence U_B = 31.  On normal
  operands a float32 product of this length stays near 4 units; the heavy-tailed families put one large term at the head of a sum
  and every later addition then rounds at ITS ulp, which is what a yardstick of sum |terms| has to allow for.  The emulated
  six-product scheme is at most 9.7 on the same inputs; every single omission is beyond 73 on some family of every case.
  No kernel entered these numbers.
* U_S[P] = the same for the batch sums: twice the worst distance of a float32 SEQUENTIAL sum of the P summands from their fp64 sum,
  in units of 2^-24 sum |summand|, over every batch sum of this file with that many pixels, rounded up.

and asserts what makes U_B discriminate: a numpy emulation of the six-product scheme (operands split with
tests/test_split_bf16._split3, the products 11, 12 + 21, 13 + 22 + 31 per K = 16 step exact, float32 accumulation in the kernel's
order) stays within U_B / 2, while for every case with K <= 132 there is at least one input family on which EACH of the five
single-product omissions and the three-product scheme (11, 12, 21) is at least 2 U_B away on some element the kernel stores.

Where no family separates, it is said here and not hidden by a wider bound:
* pix<0,4,4> stores nothing; its only outputs are batch sums, in which the sign-random error of a dropped 2^-16-class product
  averages out.  A dropped product there is caught by pix<0,3,4>, the second pass over the same product, which is separated.
* K = 260 and the pixel-K products (K = the pixel count, 389 .. 4 133) are coverage of loops, tiles and chunks: held to the bound,
  not claimed to be discriminating for the three smallest products (the two 2^-8-class products are thousands of units away at
  every K).
"""
import numpy as np
import pytest

from test_split_bf16 import FAMILIES, _split3, family

U24 = 2.0 ** -24
SEEDS = (11, 12, 13)

# measured by this file (see the docstring); the tests below assert that the constants ARE what the measurement gives
MEASURED_FP32 = 15.362                          # pix<0,2,4> P = 1 263, N = K = 132, wide_range
U_B = 31
U_S = {130: 21, 259: 38, 1263: 93, 2309: 17}    # from 10.35, 18.59, 46.50 (a sum of squares led by one large term), 8.47

# (APRO, EPI, AV, P, N, K, nslot): the instantiations csrc/nf_train_gemm.h launches with more than 64 output channels, at the
# smallest shapes that reach each branch of k_mm_pix.  P: 130 = one ragged tile at 256 and at 128 pixels; 259; 1 263 = five
# 256-pixel tiles (on two slots: each workgroup walks two or three and reuses its LDS; on seven: more slots than the 8-wavefront
# launch uses, the stale ones must be cleared); 2 309 = ten / nineteen tiles on twelve slots, so that the slot index
# (q / n_tiles) * 8 + xcd takes both of its terms.  N: 68 = one ragged channel tile, 128, 132 = a second tile of 4 channels, 70 on
# the unaligned instantiations.  K: 20 = l_1 forward on rows of 20 whose last two columns are NON-zero in A and zero in Bt, 36,
# 68, 70, 128, 132, 260 = several K tiles with a ragged last one.
PIX_CASES = [
    (0, 1, 4, 130, 68, 20, 1),
    (0, 1, 4, 1263, 132, 20, 2),
    (1, 1, 4, 259, 128, 128, 3),
    (1, 1, 4, 1263, 132, 132, 7),
    (1, 1, 4, 1263, 68, 260, 2),
    (1, 1, 1, 259, 70, 70, 2),
    (0, 2, 4, 130, 128, 128, 1),
    (0, 2, 4, 1263, 132, 132, 2),
    (0, 2, 4, 2309, 68, 68, 12),
    (0, 2, 1, 259, 70, 70, 7),
    (0, 4, 4, 130, 68, 36, 2),
    (0, 4, 4, 1263, 132, 36, 7),
    (0, 3, 4, 259, 68, 36, 1),
    (0, 3, 4, 1263, 132, 36, 7),
]
PIX_IDS = ["pix%d%d%d-P%d-N%d-K%d-s%d" % c for c in PIX_CASES]
# (npix, M, N) of d l_2/W = relu(bn(h1))^T . g_h2, the one pixel-K launch with a bf16 x 6 twin: ragged chunks, S > 1
KPIX_CASES = [(npix, w, w) for w in (68, 128, 132) for npix in (389, 1000, 4133)]
KPIX_IDS = ["kpix-npix%d-M%d-N%d" % c for c in KPIX_CASES]
# floats the partial products may take: 5 products of 132 x 132 — this, not the CU count, limits S (18 at 68 x 68, 5 at 128 and 132)
KPIX_PART_CAP = 5 * 132 * 132


def _draw(name, seed, rows, cols):
    """[rows, cols] float32 of one family of tests/test_split_bf16.family."""
    return np.ascontiguousarray(family(name, seed, B=1, channels=cols, hw=(rows, 1)).reshape(rows, cols))


def _weight_scale(K):
    """0.3 sqrt(4 / K) rounded to a power of two, so that bf16-exact weights and rounding ties stay what they are."""
    return np.float32(2.0 ** np.round(np.log2(0.3 * np.sqrt(4.0 / K))))


def _impulse(rows, cols):
    """One non-zero per row, at column (7 row + 3) % cols, holding 1 + row 2^-11 + column 2^-20 (bits in all three bf16 planes): a
    product that took a wrong k, row or column is an identifiable number, not just an error size."""
    a = np.zeros((rows, cols), np.float32)
    r = np.arange(rows)
    k = (7 * r + 3) % cols
    a[r, k] = (1.0 + r * 2.0 ** -11 + k * 2.0 ** -20).astype(np.float32)
    return a


def _bn(rng, n):
    """(bias [n], (mean [n], rstd [n]) as one vector of 2 n) of a batch normalisation, as mm_probe.hip draws them."""
    bias = (0.2 * rng.uniform(-1, 1, n)).astype(np.float32)
    mean = (0.2 * rng.uniform(-1, 1, n)).astype(np.float32)
    rstd = (0.5 + np.abs(rng.uniform(-1, 1, n))).astype(np.float32)
    return bias, np.concatenate([mean, rstd])


def _xhat64(h, bias, bn):
    n = bias.size
    rs = bn[n:].astype(np.float64)
    return h.astype(np.float64) * rs + (bias.astype(np.float64) - bn[:n].astype(np.float64)) * rs


def _off_the_kink(h, bias, bn):
    """Masks are discontinuous: every element of the pre-BN activation whose fp64 xhat is within 2^-16 (1 + |xhat|) of zero is
    replaced by one with xhat = 0.5 — a condition on the inputs, met by the reference alone (there is no kink rule in these files)."""
    n = bias.size
    xh = _xhat64(h, bias, bn)
    near = np.abs(xh) <= 2.0 ** -16 * (1.0 + np.abs(xh))
    sub = (0.5 / bn[n:].astype(np.float64) - (bias.astype(np.float64) - bn[:n].astype(np.float64))).astype(np.float32)
    h = np.where(near, np.broadcast_to(sub, h.shape), h).astype(np.float32)
    xh = _xhat64(h, bias, bn)
    assert not (np.abs(xh) <= 2.0 ** -16 * (1.0 + np.abs(xh))).any()
    return h


def pix_operands(case, name, seed):
    """float32 operands of one k_mm_pix launch: A [P][K], W [N][K] (Bt = W padded to a multiple of 4 columns), and whatever the
    prologue / epilogue of the instantiation reads."""
    apro, epi, av, P, N, K, nslot = case
    rng = np.random.RandomState(1000 * seed + 17 * PIX_CASES.index(case) + FAMILIES.index(name))
    o = {}
    o["A"] = _impulse(P, K) if name == "impulse" else _draw(name, seed, P, K)
    dense = "lognormal" if name == "impulse" else name
    W = _draw(dense, seed + 40, N, K) * _weight_scale(K)
    if K == 20:
        W[:, 18:] = 0.0                                    # the spare columns of the packed W1^T; A keeps its two
        assert np.all(o["A"][:, 18:] != 0) or name in ("impulse", "bf16_exact")
    o["W"] = W.astype(np.float32)
    if apro == 1:
        o["abias"], o["abn"] = _bn(rng, K)
    if epi:
        o["ebias"], o["ebn"] = _bn(rng, N)
    if epi >= 2:
        o["eh"] = _off_the_kink(_draw(dense, seed + 80, P, N), o["ebias"], o["ebn"])
    if epi == 3:
        o["ebb"] = (0.1 * rng.uniform(-1, 1, 2 * N)).astype(np.float32)
    return o


def _prologue64(apro, o):
    """(pro(A), its magnitude) in fp64 from the fp32 inputs: APRO 1 = relu(h r + (b - m) r) with magnitude |h r| + |(b - m) r|."""
    A = o["A"].astype(np.float64)
    if apro != 1:
        return A, np.abs(A)
    K = o["abias"].size
    rs = o["abn"][K:].astype(np.float64)
    c = (o["abias"].astype(np.float64) - o["abn"][:K].astype(np.float64)) * rs
    return np.maximum(A * rs + c, 0.0), np.abs(A * rs) + np.abs(c)


def _epilogue64(epi, o, acc, Tacc):
    """What the kernel leaves, from the fp64 product `acc` (and its term magnitudes): dict with C / T_C (None: nothing stored) and
    the batch sums as (name, summand [P][N]) pairs."""
    if epi == 0:
        return dict(C=acc, T=Tacc, sums=[])
    N = o["ebias"].size
    if epi == 1:
        x = acc + o["ebias"].astype(np.float64)
        return dict(C=acc, T=Tacc, sums=[("sum", x), ("sumsq", x * x)])
    xh = _xhat64(o["eh"], o["ebias"], o["ebn"])
    gx = np.where(xh > 0, acc, 0.0)
    if epi in (2, 4):
        return dict(C=acc if epi == 2 else None, T=Tacc, sums=[("sum gx", gx), ("sum gx xhat", gx * xh)])
    rs = o["ebn"][N:].astype(np.float64)
    ba, bq = o["ebb"][:N].astype(np.float64), o["ebb"][N:].astype(np.float64)
    out = rs * (gx - ba - xh * bq)
    return dict(C=out, T=rs * (Tacc + np.abs(ba) + np.abs(xh * bq)), sums=[("sum", out)])


def pix_reference(case, o):
    apro, epi = case[0], case[1]
    Ap, Am = _prologue64(apro, o)
    W = o["W"].astype(np.float64)
    return _epilogue64(epi, o, Ap @ W.T, Am @ np.abs(W).T)


def matmul32(A, W):
    """A [P][K] . W [N][K]^T in plain float32, one k after the other: every product and every sum rounded to float32 (elementwise
    numpy only, so the figure does not depend on the BLAS behind numpy.matmul)."""
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    Wt = np.ascontiguousarray(W.T)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * Wt[k]
    return acc


def pix_plain_fp32(case, o):
    """The same launch as a plain numpy float32 evaluation: prologue, product and epilogue in float32."""
    apro, epi, av, P, N, K, nslot = case
    f = np.float32
    A = o["A"]
    if apro == 1:
        rs = o["abn"][K:]
        A = np.maximum(A * rs + (o["abias"] - o["abn"][:K]) * rs, f(0))
    acc = matmul32(A, o["W"])
    if epi != 3:
        return acc.astype(np.float64)
    rs = o["ebn"][N:]
    xh = o["eh"] * rs + (o["ebias"] - o["ebn"][:N]) * rs
    out = rs * (np.where(xh > 0, acc, f(0)) - o["ebb"][:N] - xh * o["ebb"][N:])
    assert out.dtype == np.float32
    return out.astype(np.float64)


def kpix_operands(case, name, seed):
    """A [npix][M] = the pre-BN activation (APRO 1: the kernel forms relu(xhat(A + bias))), B [npix][N], bias and (mean, rstd) [M]."""
    npix, M, N = case
    rng = np.random.RandomState(2000 * seed + 17 * KPIX_CASES.index(case) + FAMILIES.index(name))
    o = {}
    o["A"] = _impulse(npix, M) if name == "impulse" else _draw(name, seed, npix, M)
    o["B"] = _draw("lognormal" if name == "impulse" else name, seed + 40, npix, N)
    o["abias"], o["abn"] = _bn(rng, M)
    return o


def kpix_reference(o):
    Ap, Am = _prologue64(1, o)
    B = o["B"].astype(np.float64)
    return Ap.T @ B, Am.T @ np.abs(B)


def units(err, T):
    """max |err| / (2^-24 T) over the elements whose T is not zero; an error where T is zero is infinite."""
    err, T = np.abs(np.asarray(err, np.float64)), np.asarray(T, np.float64)
    if np.any((T == 0) & (err != 0)):
        return float("inf")
    nz = T > 0
    return float((err[nz] / (U24 * T[nz])).max()) if nz.any() else 0.0


def seq_sum_units(summand):
    """Distance of the float32 sequential column sums of `summand` [P][N] from the fp64 ones, in units of 2^-24 sum |summand|."""
    s32 = np.cumsum(summand.astype(np.float32), axis=0, dtype=np.float32)[-1].astype(np.float64)
    return units(s32 - summand.sum(axis=0), np.abs(summand).sum(axis=0))


# ---- the six-product scheme and its mutants, emulated ---------------------------------------------------------------------------

# (piece of A, piece of B) in the order k_mm_pix / k_mm_kpix6 issue them per K = 16 step: smallest products first
ORDER = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
MUTANTS = {"six": ORDER, "no 13": [p for p in ORDER if p != (0, 2)], "no 31": [p for p in ORDER if p != (2, 0)],
           "no 22": [p for p in ORDER if p != (1, 1)], "no 12": [p for p in ORDER if p != (0, 1)],
           "no 21": [p for p in ORDER if p != (1, 0)], "three": [(0, 1), (1, 0), (0, 0)]}


def emulate(A32, W32):
    """{variant: C [P][N]} of pro(A) . W^T as the bf16 x 6 kernels take it: both float32 operands in three bf16 pieces, per K = 16
    step the listed piece products exact (fp64 dots of 16 bf16 x bf16 terms) and added to a float32 accumulator in ORDER."""
    P, K = A32.shape
    Ap, Wp = _split3(A32), _split3(W32)
    acc = {v: np.zeros((P, W32.shape[0]), np.float32) for v in MUTANTS}
    for k0 in range(0, K, 16):
        part = {(i, j): Ap[i][:, k0:k0 + 16] @ Wp[j][:, k0:k0 + 16].T for i, j in ORDER}
        for v, prods in MUTANTS.items():
            for ij in prods:
                acc[v] = (acc[v] + part[ij]).astype(np.float32)
    return {v: a.astype(np.float64) for v, a in acc.items()}


def _pro32(case, o):
    """pro(A) as the kernel stages it (float32; one fma per element)."""
    if case[0] != 1:
        return o["A"]
    K = case[5]
    rs = o["abn"][K:]
    c = ((o["abias"] - o["abn"][:K]) * rs).astype(np.float32)
    x = (o["A"].astype(np.float64) * rs.astype(np.float64) + c.astype(np.float64)).astype(np.float32)   # fmaf: one rounding
    return np.maximum(x, np.float32(0))


_cache = {}


def _measured(case):
    """Per family: worst units over the seeds of the plain float32 evaluation, and of every emulated variant pushed through the
    epilogue in fp64; and the sequential-sum units of every batch sum.  Computed once per case."""
    if case in _cache:
        return _cache[case]
    epi = case[1]
    res = {"fp32": {}, "seq": 0.0}
    for v in MUTANTS:
        res[v] = {}
    for name in FAMILIES:
        w32 = 0.0
        wv = {v: 0.0 for v in MUTANTS}
        for seed in SEEDS:
            o = pix_operands(case, name, seed)
            ref = pix_reference(case, o)
            for _, summand in ref["sums"]:
                res["seq"] = max(res["seq"], seq_sum_units(summand))
            if ref["C"] is None:
                continue
            w32 = max(w32, units(pix_plain_fp32(case, o) - ref["C"], ref["T"]))
            Tacc = _prologue64(case[0], o)[1] @ np.abs(o["W"].astype(np.float64)).T
            for v, acc in emulate(_pro32(case, o), o["W"]).items():
                wv[v] = max(wv[v], units(_epilogue64(epi if epi != 1 else 0, o, acc, Tacc)["C"] - ref["C"], ref["T"]))
        res["fp32"][name] = w32
        for v in MUTANTS:
            res[v][name] = wv[v]
    _cache[case] = res
    return res


def test_the_constants_are_what_the_cpu_measurement_gives():
    """U_B and U_S as derived: twice the worst plain-float32 distance over every case with K <= 132, rounded up."""
    worst = max(max(_measured(c)["fp32"].values()) for c in PIX_CASES if c[5] <= 132)
    seq = {}
    for c in PIX_CASES:
        if c[1]:
            seq[c[3]] = max(seq.get(c[3], 0.0), _measured(c)["seq"])
    print("\nworst plain float32 distance from fp64, K <= 132, units of 2^-24 T: %.3f -> U_B = %d" % (worst, int(np.ceil(2 * worst))))
    print("worst float32 sequential-sum distance by pixel count, units of 2^-24 sum |summand|: %s -> U_S = %s"
          % ({p: round(s, 3) for p, s in sorted(seq.items())}, {p: int(np.ceil(2 * s)) for p, s in sorted(seq.items())}))
    assert abs(worst - MEASURED_FP32) <= 5e-3, worst
    assert U_B == int(np.ceil(2 * worst))
    assert U_S == {p: int(np.ceil(2 * s)) for p, s in seq.items()}


@pytest.mark.parametrize("case", PIX_CASES, ids=PIX_IDS)
def test_plain_fp32_and_six_products_within_half_the_bound(case):
    """... on EVERY family and seed, also at K = 260; and the table of every variant is printed."""
    m = _measured(case)
    print("\n%s, worst over the seeds in units of 2^-24 T" % PIX_IDS[PIX_CASES.index(case)])
    print("%-11s" % "family" + "".join("%10s" % v for v in ["fp32"] + list(MUTANTS)))
    for name in FAMILIES:
        print("%-11s" % name + "".join("%10.3g" % m[v][name] for v in ["fp32"] + list(MUTANTS)))
    if case[1] == 4:
        return      # nothing stored: only batch sums (module docstring)
    for name in FAMILIES:
        assert m["fp32"][name] <= U_B / 2, (name, m["fp32"][name])
        assert m["six"][name] <= U_B / 2, (name, m["six"][name])


@pytest.mark.parametrize("case", [c for c in PIX_CASES if c[5] <= 132 and c[1] != 4],
                         ids=[i for c, i in zip(PIX_CASES, PIX_IDS) if c[5] <= 132 and c[1] != 4])
def test_every_omission_is_twice_the_bound_away_on_some_family(case):
    m = _measured(case)
    for v in MUTANTS:
        if v == "six":
            continue
        best = max(m[v].values())
        assert best >= 2 * U_B, (v, m[v])
