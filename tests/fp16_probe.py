"""Dyadic probe models for the fp16-CNN kernel families (helper, not a test).

The probe model is that of tests/test_gpu_split_bf16_probe.py::probe_variables — one `unc` coupling, the 1x1 mix the LU form of
the identity, a "shift" probe (the raw channels of l_last zero) and a "raw" probe (the shift channels zero, the input's second
half one) — but its weights are DESIGNED: every weight, bias and input is a small integer times a power of two, so that every
accumulation in front of a rounding point is exact in fp32 in any order, and the half rounding is a function of an exactly known
number.  design() draws the integers, variables() turns them into checkpoint variables, probe_z0() / probe_x() give the two input
families, chain() is the fp64 evaluation (exact wherever the conditions hold) with the mutants the CPU test needs.

Integers and scales (value = integer * 2^scale):
  l_1     c1 [3,3,2,w]: every output channel holds +-1 .. +-9 once each over its 18 (tap, channel) slots; scale S1 = -2;
          b1 = m1 * 2^-1, m1 in +-1 .. +-6
  l_2     d [w,w] (cin, cout), 1x1: min(8, w) non-zeros per output channel, the values +-1 .. +-4 once each, every input channel
          used at least once (width 4: +-(1, -2, -3, 4), signs that sum to zero); scale S2 = -2;  b2 = m2 * 2^-3, m2 in +-1 .. +-32
  l_last  e [3,3,w,2] for the two live output channels: n3 = min(9 w, max(144, w / 2)) non-zeros per output channel holding
          +-1 .. +-n3/2 once each, every hidden channel used by at least one of the two; scale S3 = -6 (shift probe) or
          raw_scale(width) (raw probe, where e * 2^scale is the HALF value q the kernel shall hold and the variable is
          fl32(q / (2 log2 e))); edge-channel weights r * 2^-2 (r in +-1 .. +-20, distinct over the taps), b3 = m3 * 2^-2 (2^-7 both in the
          raw probe)
  z0      `exact`:    a * 2^1,   a in -3 .. 3             -> h1 is a multiple of 2^-1, h2 of 2^-3, the shift of 2^-9
          `rounding`: +-a * 2^-10, a in 2048 .. 5119        (12- and 13-bit significands: ties and inexact values)
BN means are 0, BN variances fl32(1 - BN_EPS): the fold's scale 1 / sqrt(var + eps) is within 2^-25 of 1 and every designed value
rounds back to itself (asserted against nf_fold_params and the oracle in tests/test_fp16_exact_probe_cpu.py).  rescaling_scale = 1.
"""
import numpy as np

T = "model/real_nvp_conv_template/"
K2 = 2.0 * 1.4426950408889634
BN_VAR = np.float32(1.0 - 1e-4)
S1, S2, S3 = -2, -2, -6
SB1, SB2, SB3 = -1, -3, -2
SB3_RAW = -7            # border table and bias of the raw probe: small against tanh's linear range
SZ = {"exact": 1, "rounding": -10}
FAMILIES = ("exact", "rounding")
RESCALE = 1.0
B_FAMILY = 2
HALF_MIN, HALF_MAX = 2.0 ** -14, 65504.0


def _signed(n):
    return np.concatenate([np.arange(1, n + 1), -np.arange(1, n + 1)])


def raw_scale(width):
    """Scale of the raw probe's l_last half values: the raw log-scale of the designed inputs has a spread of a few tenths (neither
    lost in tanh's linear part nor saturated), as far as e * 2^scale stays a normal half (scale >= -14)."""
    w = width
    n3 = min(9 * w, max(144, (w + 1) // 2))
    n2 = (min(8, w) * 7.5 * 48.0 ** 2 / 2) ** 0.5            # spread of h2 in units of 2^-3 on the `exact` family
    spread = (n3 * ((n3 / 2) ** 2 / 3.0) * n2 ** 2 / 2) ** 0.5 * 2.0 ** -3
    return max(-14, -int(round(np.log2(spread))))


def design(width, seed):
    """The integers of one probe model (module docstring)."""
    rng = np.random.RandomState(7919 * seed + width)
    w = width
    c1 = np.stack([rng.permutation(_signed(9)) for _ in range(w)], -1).reshape(3, 3, 2, w)
    m1 = rng.choice(_signed(6), w)
    k = min(8, w)
    d = np.zeros((w, w), np.int64)
    first = rng.permutation(w)
    for j in range(w):
        rest = np.delete(np.arange(w), first[j])
        cin = np.concatenate([[first[j]], rng.choice(rest, k - 1, replace=False)])
        # all eight values at widths >= 8; at width 4 the four magnitudes with signs that sum to zero: with four hidden channels
        # one row of like signs would leave the second ReLU nearly all alive or all dead
        vals = rng.permutation(_signed(4)) if k == 8 else rng.permutation(np.asarray([1, -2, -3, 4])[:k] * rng.choice([-1, 1]))
        d[cin, j] = vals
    m2 = rng.choice(_signed(32), w)
    n3 = min(9 * w, max(144, (w + 1) // 2))
    e = np.zeros((9 * w, 2), np.int64)
    owner = rng.permutation(w) % 2                           # the output channel that is sure to use hidden channel c
    for j in range(2):
        must = np.flatnonzero(owner == j) if n3 < 9 * w else np.arange(0)
        pos = rng.randint(9, size=must.size) * w + must
        free = np.setdiff1d(np.arange(9 * w), pos)
        pos = np.concatenate([pos, rng.choice(free, n3 - pos.size, replace=False)])
        e[pos, j] = rng.permutation(_signed((n3 + 1) // 2))[:n3]
    e = e.reshape(3, 3, w, 2)
    r = np.stack([rng.permutation(_signed(20))[:9] for _ in range(2)], -1).reshape(3, 3, 2)
    m3 = rng.choice(_signed(40), 2)
    return {"width": w, "seed": seed, "c1": c1, "m1": m1, "d": d, "m2": m2, "e": e, "r": r, "m3": m3}


def weights(D, half):
    """The designed values in fp64: W1, b1, W2 [w,w], b2, W3 [3,3,w+1,4] (the half values the kernel holds: the raw columns carry
    2 log2(e), i.e. they multiply to 2 log2(e) raw), b3 [4] (natural units)."""
    w = D["width"]
    W3 = np.zeros((3, 3, w + 1, 4))
    b3 = np.zeros(4)
    live = slice(0, 2) if half == "shift" else slice(2, 4)
    W3[:, :, :w, live] = np.ldexp(D["e"].astype(np.float64), S3 if half == "shift" else raw_scale(w))
    sb3 = SB3 if half == "shift" else SB3_RAW
    W3[:, :, w, live] = np.ldexp(D["r"].astype(np.float64), sb3)
    b3[live] = np.ldexp(D["m3"].astype(np.float64), sb3)
    return (np.ldexp(D["c1"].astype(np.float64), S1), np.ldexp(D["m1"].astype(np.float64), SB1),
            np.ldexp(D["d"].astype(np.float64), S2), np.ldexp(D["m2"].astype(np.float64), SB2), W3, b3)


def variables(D, half):
    """Checkpoint variables of the probe model: `unc`, identity mix, BN mean 0 / var fl32(1 - BN_EPS), logs = 0."""
    from oracle.nf_oracle import conv1x1_variable_names, fresh_variables
    w = D["width"]
    W1, b1, W2, b2, W3, b3 = weights(D, half)
    v = fresh_variables("unc", w, seed=D["seed"])
    n = conv1x1_variable_names(0, "LU")
    v[n["P"]] = np.eye(4, dtype=np.float32)
    v[n["sign_S"]] = np.ones(4, np.float32)
    v[n["log_S"]] = np.zeros(4, np.float32)
    v[n["L_vec"]] = np.zeros_like(v[n["L_vec"]])
    v[n["U_vec"]] = np.zeros_like(v[n["U_vec"]])
    f32 = lambda a: np.asarray(a, np.float32)   # noqa: E731
    v[T + "l_1/W"] = f32(W1)
    v[T + "l_1/b"] = f32(b1).reshape(1, 1, 1, w)
    v[T + "l_2/W"] = f32(W2).reshape(1, 1, w, w)
    v[T + "l_2/b"] = f32(b2).reshape(1, 1, 1, w)
    W3v = W3.copy()
    if half == "raw":       # designed backwards: half(fl32(q / k2) * k2) = q under an fp32 or an fp64 fold alike
        W3v[:, :, :w, 2:] = f32(W3[:, :, :w, 2:] / K2)
    v[T + "l_last/W"] = f32(W3v)
    v[T + "l_last/b"] = f32(b3).reshape(1, 1, 1, 4)
    v[T + "l_last/logs"] = np.zeros((1, 4), np.float32)
    for b in ("bn_nvp_conv_1", "bn_nvp_conv_2"):
        v[T + b + "/mean"] = np.zeros((w,), np.float32)
        v[T + b + "/var"] = np.full((w,), BN_VAR, np.float32)
    v["level0/bijector0/rescaling_scale0"] = np.float32(RESCALE)
    for k in (T + "l_1/W", T + "l_1/b", T + "l_2/W", T + "l_2/b", T + "l_last/b"):
        assert np.array_equal(v[k].astype(np.float64).reshape(-1), {"l_1/W": W1, "l_1/b": b1, "l_2/W": W2, "l_2/b": b2,
                                                                      "l_last/b": b3}[k[len(T):]].reshape(-1))
    return v


# ---- rounding to half, on fp64 ---------------------------------------------------------------------------------------------------

def round_half(x, mode="rne"):
    """x (fp64) rounded to 11 significant bits: "rne" = IEEE round-to-nearest-even (what the kernels and numpy do), "rtz" =
    toward zero, "rha" = nearest, ties away from zero.  Normal range only (assert_half_normal)."""
    x = np.asarray(x, np.float64)
    m, ex = np.frexp(x)
    s = m * 2048.0
    if mode == "rne":
        s = np.rint(s)
    elif mode == "rtz":
        s = np.trunc(s)
    else:
        assert mode == "rha", mode
        s = np.sign(s) * np.floor(np.abs(s) + 0.5)
    return np.ldexp(s, ex - 11)


def assert_half_normal(x, what):
    a = np.abs(np.asarray(x, np.float64))
    nz = a[a != 0]
    assert nz.size == 0 or (nz.min() >= HALF_MIN and nz.max() <= HALF_MAX), (what, float(nz.min()), float(nz.max()))


def lowbit(x):
    """The value of the lowest set bit of every element (inf for 0)."""
    x = np.asarray(x, np.float64)
    m, ex = np.frexp(x)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)
    return np.where(x != 0, np.ldexp((M & -M).astype(np.float64), ex - 53), np.inf)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def l_2(a1, W2, b2, in_half=False):
    """relu(h1) -> h2 (1x1 conv); in_half: accumulated in half, input channel by input channel (ascending), from the bias."""
    if not in_half:
        return a1 @ W2 + b2
    w = W2.shape[0]
    idx = np.stack([np.flatnonzero(W2[:, j]) for j in range(w)])          # [cout, non-zeros], ascending input channel
    h2 = np.broadcast_to(b2, a1.shape).copy()
    for i in range(idx.shape[1]):
        h2 = round_half(h2 + a1[..., idx[:, i]] * W2[idx[:, i], np.arange(w)])
    return h2


def _local_shift(D, zpix, modes, valid, l2_half=False):
    """The shift on the 3x3 neighbourhood of a lone impulse `zpix` [2] of a zero image, as far as the neighbourhood's own
    relu(h2) feeds it (the background's share is the same for every `modes`); valid [3,3] = the neighbours inside the image."""
    W1, b1, W2, b2, W3, _ = weights(D, "shift")
    z = round_half(zpix, modes[0])
    h1 = np.maximum(np.einsum("c,ijcw->ijw", z, W1[::-1, ::-1]) + b1, 0)
    h2 = np.maximum(l_2(round_half(h1, modes[1]), W2, b2, l2_half), 0)
    a2 = round_half(h2, modes[2]) * valid[..., None]
    out = np.zeros((3, 3, 2))
    for oy in range(3):
        for ox in range(3):
            for ny in range(max(0, oy - 1), min(3, oy + 2)):
                for nx in range(max(0, ox - 1), min(3, ox + 2)):
                    out[oy, ox] += a2[ny, nx] @ W3[ny - oy + 1, nx - ox + 1, :D["width"], :2]
    return out * valid[..., None]


def _rounding_impulse(D, rng, hw, pos):
    """An impulse of the `rounding` family at `pos`: channel 0 a 12-bit tie that round-to-nearest-even rounds up (toward zero
    differs), channel 1 one it rounds down (ties-away differs), drawn until each of the six rounding-mode mutants, and l_2 accumulated in half, moves
    the shift next to the impulse — a patch with one live pixel has few roundings, and every mutant must show on every patch."""
    valid = np.asarray([[0 <= pos[0] + i < hw[0] and 0 <= pos[1] + j < hw[1] for j in (-1, 0, 1)] for i in (-1, 0, 1)], np.float64)
    for _ in range(1024):
        a = np.asarray([2048 + 4 * rng.randint(512) + 3, 2048 + 4 * rng.randint(512) + 1], np.float64)
        z = np.ldexp(a * rng.choice([-1.0, 1.0], 2), SZ["rounding"])
        ref = _local_shift(D, z, ("rne", "rne", "rne"), valid)
        if all(not np.array_equal(ref, _local_shift(D, z, tuple(m if i == k else "rne" for i in range(3)), valid))
               for k in range(3) for m in ("rtz", "rha")) and not np.array_equal(ref, _local_shift(D, z, ("rne",) * 3, valid, True)):
            return z
    raise AssertionError("no impulse separates the six rounding mutants at width %d, %s of %s" % (D["width"], pos, hw))


def probe_z0(D, name, hw, positions):
    """[B_FAMILY + len(positions), H, W, 2] fp32: B_FAMILY patches of the family, then one impulse patch per position."""
    H, W = hw
    rng = np.random.RandomState(1000 * D["seed"] + 10 * FAMILIES.index(name) + 3)
    n = B_FAMILY + len(positions)
    z = np.zeros((n, H, W, 2))
    shape = (B_FAMILY, H, W, 2)
    if name == "exact":
        z[:B_FAMILY] = np.ldexp(rng.randint(-3, 4, size=shape).astype(np.float64), SZ[name])
        if H * W == 1:
            z[:B_FAMILY] = np.ldexp(rng.choice(_signed(3), size=shape).astype(np.float64), SZ[name])
        for b, (r, c) in enumerate(positions):
            z[B_FAMILY + b, r, c] = np.ldexp(rng.choice(_signed(3), 2).astype(np.float64), SZ[name])
    else:
        a = rng.randint(2048, 5120, size=shape) * rng.choice([-1.0, 1.0], size=shape)
        z[:B_FAMILY] = np.ldexp(a, SZ[name])
        for b, (r, c) in enumerate(positions):
            z[B_FAMILY + b, r, c] = _rounding_impulse(D, rng, hw, (r, c))
        if H * W == 1:      # one pixel is no population: the family patches are such impulses too
            for b in range(B_FAMILY):
                z[b, 0, 0] = _rounding_impulse(D, rng, hw, (0, 0))
    out = z.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), z)
    return out


def probe_z1(D, name, half, z0):
    """The input's second half: one in the raw probe; in the shift probe of the `exact` family a grid of non-zero multiples of
    2^-3 (a wrong pass-through pixel shows, and z1 + shift stays exact); zero in the shift probe of the `rounding` family, whose
    shift is not everywhere exact in fp32."""
    if half == "raw":
        return np.ones_like(z0)
    if name != "exact":
        return np.zeros_like(z0)
    rng = np.random.RandomState(1000 * D["seed"] + 77)
    return np.ldexp(rng.choice(_signed(40), z0.shape).astype(np.float64), -3).astype(np.float32)


def probe_x(D, name, half, z0):
    return np.concatenate([z0, probe_z1(D, name, half, z0)], -1)


# ---- the chain -------------------------------------------------------------------------------------------------------------------

def _conv3(x, Wt, pad):
    from oracle.nf_oracle import conv2d_nhwc
    return conv2d_nhwc(x, Wt, pad)


def edge_table(D, half):
    """E [H, W, 4] builder: b3 plus the edge-channel weights of the taps that fall outside the image."""
    _, _, _, _, W3, b3 = weights(D, half)
    w = D["width"]

    def table(H, W):
        from oracle.nf_oracle import add_edge_padding
        ring = add_edge_padding(np.zeros((1, H, W, 0)))
        return (_conv3(ring, W3[:, :, w:, :], False) + b3)[0]
    return table


def chain(D, z0, half, modes=("rne", "rne", "rne"), drop=None, swap=None, l2_half=False, w3_pre_round=False, want=None):
    """The coupling CNN on the designed values in fp64 -> [N, H, W, 2], the live half of l_last's output in natural units (the
    shift, or the raw log-scale).  Exact wherever the conditions of the CPU test hold.  Mutants: `modes` = rounding of (z0, relu
    h1, relu h2); drop = (layer, [(patch, row, col)]) leaves one 3x3 tap of l_1 / l_last out at those output pixels (per pixel
    the first tap, centre first, whose contribution is not zero); swap = (i, j) exchanges two input channels of l_2; l2_half
    accumulates l_2 in half, input channel by input channel; w3_pre_round rounds l_last's raw weights before the 2 log2(e) fold.
    `want` (a dict) receives the intermediates."""
    W1, b1, W2, b2, W3, b3 = weights(D, half)
    w = D["width"]
    live = slice(0, 2) if half == "shift" else slice(2, 4)
    z = round_half(np.asarray(z0, np.float64), modes[0])
    N, H, W, _ = z.shape
    taps = [(1, 1), (0, 1), (1, 0), (1, 2), (2, 1), (0, 0), (0, 2), (2, 0), (2, 2)]
    h1 = _conv3(z, W1, True) + b1
    if drop is not None and drop[0] == "l_1":
        zp = np.pad(z, [(0, 0), (1, 1), (1, 1), (0, 0)])
        for b, r, c in drop[1]:
            for di, dj in taps:
                t = zp[b, r + di, c + dj] @ W1[di, dj]
                if np.any(t != 0):
                    h1[b, r, c] -= t
                    break
            else:
                raise AssertionError(("no live tap of l_1", b, r, c))
    a1 = round_half(np.maximum(h1, 0), modes[1])
    if swap is not None:
        a1 = a1.copy()
        a1[..., list(swap)] = a1[..., list(swap[::-1])]
    h2 = l_2(a1, W2, b2, l2_half)
    a2 = round_half(np.maximum(h2, 0), modes[2])
    W3l = W3[:, :, :w, live]
    if w3_pre_round:
        assert half == "raw"
        W3l = round_half(np.asarray(W3l / K2, np.float32).astype(np.float64)) * K2
    a2p = np.pad(a2, [(0, 0), (1, 1), (1, 1), (0, 0)])
    E = edge_table(D, half)(H, W)[..., live]
    o = _conv3(a2p, W3l, False)
    if drop is not None and drop[0] == "l_last":
        for b, r, c in drop[1]:
            for di, dj in taps:
                t = a2p[b, r + di, c + dj] @ W3l[di, dj]
                if np.any(t != 0):
                    o[b, r, c] -= t
                    break
            else:
                raise AssertionError(("no live tap of l_last", b, r, c))
    nat = 1.0 / K2 if half == "raw" else 1.0       # the raw columns' products are in units of 2 log2(e) raw
    if want is not None:
        want.update(z=z, h1=h1, a1=a1, h2=h2, a2=a2, conv3=o.copy(), E=E,
                    abs1=_conv3(np.abs(z), np.abs(W1), True) + np.abs(b1), abs2=a1 @ np.abs(W2) + np.abs(b2),
                    abs3=_conv3(a2p, np.abs(W3l), False) * nat + np.abs(E))
    return o * nat + E


def l_last_exact_mask(a2, abs3, E):
    """Per output element: every addend of l_last (the products of the 3x3 window, the border-table entry) is a multiple of one
    unit u and sum |addends| <= 2^22 u.  u = the lowest set bit over the window's live activations times that of the weights
    (2^S3: the integers e are odd or even), and over E."""
    lb = lowbit(a2).min(axis=-1)
    lbp = np.pad(lb, [(0, 0), (1, 1), (1, 1)], constant_values=np.inf)
    H, W = lb.shape[1:]
    u = np.full(lb.shape, np.inf)
    for di in range(3):
        for dj in range(3):
            u = np.minimum(u, lbp[:, di:di + H, dj:dj + W])
    u = np.minimum(u * 2.0 ** S3, lowbit(E).min(axis=-1))
    return abs3 <= 2.0 ** 22 * u[..., None]


def sequential_f32_l_last(D, a2, E):
    """The shift half of l_last as a sequential fp32 accumulation: border-table entry first, then tap by tap, channel by
    channel, one rounding per addition (the products are exact in fp32: 8 x 11 bits)."""
    W3 = weights(D, "shift")[4]
    w = D["width"]
    a2p = np.pad(a2, [(0, 0), (1, 1), (1, 1), (0, 0)]).astype(np.float32)
    N, H, W = a2.shape[:3]
    out = np.empty((N, H, W, 2), np.float32)
    for j in range(2):
        acc = np.broadcast_to(E[..., j].astype(np.float32), (N, H, W)).copy()
        for di in range(3):
            for dj in range(3):
                for ch in np.flatnonzero(W3[di, dj, :w, j]):
                    acc += a2p[:, di:di + H, dj:dj + W, ch] * np.float32(W3[di, dj, ch, j])
        out[..., j] = acc
    return out


def params64(v):
    from oracle.nf_oracle import bind_variables
    return [L for L in bind_variables("unc", v) if L["type"] == "coupling"][0]["p"]


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, kernel path, width, (H, W), environment switch read at nf_create, row seams, column seams, linear-pixel seams)
# Seams, read from the kernels:
#  * NF_PATH_FP16 (nf_kernels.hip, the frame of the fp32 width-4 matrix-core kernel): 32x32 = 4 linear slots of 256 threads (pixel
#    seams 64 — the wavefront — 256, 512, 768); 64x64 = a lane owns a 2x2 block, a wavefront two block rows (row seams 2 and 4,
#    column seam 2), plus the middle of the patch and the linear seams 64 / 1024 for the pixel-per-lane formulation NF_H16=4x4;
#  * NF_PATH_WIDE32_FP16 (nf_wide.hip): tiles of 32 pixels along a row (column seam 32), strips of 8 rows, the last partial strip;
#  * NF_PATH_GEMM_FP16 variant b (nf_gemm16.hip::nf_gemm16b_kernel): a wavefront's tile is 32 linear pixels (`p0 + 32 * wv + n`,
#    line 289), a round RND = 32 * GW = 256 pixels (line 216), a thread owns p = t + GT m, GT = 512 (line 241), OWN = 8 pixels per
#    thread beyond 2048 (line 43), the last partial tile;
#  * NF_PATH_GEMM_FP16 variant a (nf_gemm16.hip::nf_gemm16_kernel): bands of NB = 65536 / padded width pixels (line 50: 1024 at
#    64, 256 at 256, 128 at 512), tiles of 32 (line 89), a wavefront column = 4 tiles = 128 pixels (lines 53, 116), whose P stage
#    runs in two halves of 2 tiles = 64 pixels (lines 151, 186 - 188).
# Tiled images (beyond 64x64): the seams are the tile cores' first rows / columns, asked of nf_tile_plan (halo of one coupling = 2).
CASES = [
    ("fp16-w4-32x32", "FP16", 4, (32, 32), None, (), (), (64, 256, 512, 768)),
    ("fp16-w4-32x32-4x4", "FP16", 4, (32, 32), ("NF_H16", "4x4"), (), (), (64, 256, 512, 768)),
    ("fp16-w4-64x64", "FP16", 4, (64, 64), None, (2, 4, 32), (2, 32), (64, 1024)),
    ("fp16-w4-64x64-4x4", "FP16", 4, (64, 64), ("NF_H16", "4x4"), (2, 4, 32), (2, 32), (64, 1024)),
    ("wide32h-w32-9x33", "WIDE32_FP16", 32, (9, 33), None, (8,), (32,), ()),
    ("wide32h-w32-33x64", "WIDE32_FP16", 32, (33, 64), None, (8, 32), (32,), ()),
    ("wide32h-w32-64x33", "WIDE32_FP16", 32, (64, 33), None, (8, 56), (32,), ()),
    ("wide32h-w32-1x1", "WIDE32_FP16", 32, (1, 1), None, (), (), ()),
    ("wide32h-w16-17x16", "WIDE32_FP16", 16, (17, 16), None, (8, 16), (), ()),
    ("wide32h-w8-24x24", "WIDE32_FP16", 8, (24, 24), None, (8, 16), (), ()),
    ("wide32h-w4-20x28", "WIDE32_FP16", 4, (20, 28), None, (8, 16), (), ()),
    ("wide32h-w24-9x33", "WIDE32_FP16", 24, (9, 33), None, (8,), (32,), ()),
    ("gemm16b-w64-9x33", "GEMM_FP16", 64, (9, 33), None, (), (), (32, 256)),
    ("gemm16b-w64-33x31", "GEMM_FP16", 64, (33, 31), None, (), (), (32, 256, 512, 768, 992)),
    ("gemm16b-w96-9x33", "GEMM_FP16", 96, (9, 33), None, (), (), (32, 256)),
    ("gemm16b-w96-33x31", "GEMM_FP16", 96, (33, 31), None, (), (), (32, 256, 512, 768, 992)),
    ("gemm16b-w64-64x64", "GEMM_FP16", 64, (64, 64), None, (), (), (32, 256, 512, 2048, 4064)),
    ("gemm16b-w48-7x5", "GEMM_FP16", 48, (7, 5), None, (), (), (32,)),
    ("gemm16a-w256-9x33", "GEMM_FP16", 256, (9, 33), None, (), (), (32, 64, 128, 256)),
    ("gemm16a-w256-1x1", "GEMM_FP16", 256, (1, 1), None, (), (), ()),
    ("gemm16a-w512-9x33", "GEMM_FP16", 512, (9, 33), None, (), (), (32, 64, 128, 256)),
    ("gemm16a-w200-7x5", "GEMM_FP16", 200, (7, 5), None, (), (), (32,)),
    ("gemm16a-w64-9x33-forced", "GEMM_FP16", 64, (9, 33), ("NF_GEMM16", "a"), (), (), (32, 64, 128, 256)),
    ("tiled-fp16-w4-70x66", "FP16", 4, (70, 66), None, "tiles", "tiles", ()),
    ("tiled-wide32h-w32-66x40", "WIDE32_FP16", 32, (66, 40), None, "tiles", "tiles", ()),
]
CASE_IDS = [c[0] for c in CASES]
SEEDS = (11, 12)


def layout_width(width):
    """The width the kernels run (nf_host.hip::build_program): 4 / 8 / 16 / 32 up to 32, the model's own beyond (zero-padded to
    64 / 128 / 256 / 512 inside the GEMM layouts)."""
    return width if width > 32 else 4 if width <= 4 else 8 if width <= 8 else 16 if width <= 16 else 32


def pads(width):
    return width not in (4, 8, 16, 32, 64, 128, 256, 512)


def tile_seams(size):
    """First core row / column of every tile but the first, from the library's own plan (64-pixel tiles, halo 2)."""
    import ctypes as C
    from noise_flow_amd import _lib
    if size <= 64:
        return ()
    core0 = (C.c_int32 * 16)()
    n = _lib.load().nf_tile_plan(size, 64, 2, None, core0, None, 16)
    assert 2 <= n <= 16, n
    return tuple(int(core0[i]) for i in range(1, n))


def case_positions(case):
    from test_gpu_probe_families import impulse_positions
    _, _, _, hw, _, rows, cols, lin = case
    rows = tile_seams(hw[0]) if rows == "tiles" else rows
    cols = tile_seams(hw[1]) if cols == "tiles" else cols
    return impulse_positions(hw, rows, cols, lin)
