"""Probe models: the coupling CNN of the width-4 kernels at 32x32, observed at fp32 resolution.

A one-coupling model (`unc`, 1x1 mix = the identity) whose OUTPUT is the conv chain l_1 -> ReLU -> l_2 -> ReLU -> l_last and
nothing else:

* shift probe: the two raw-log-scale output channels of l_last are zero (ls = 0 exactly) and the input's second half is zero, so
  `inverse` returns  x1 = shift  and `forward`  -shift  in channels 2, 3;
* raw probe: the two shift channels are zero and the input's second half is one, so the output is  exp(+-ls),
  ls = rescaling_scale * tanh(raw); log(out) is compared in fp64, and the per-patch log-det against  sum ls.

Yardstick (fp64 oracle alone): per output element  A = |W3| * (|W2| . a1 + |b2'|) + |E|,  a1 = |W1| * |z0| + |b1'|,  BN-eval
folded as oracle.coupling_cnn applies it — to first order the sum of the magnitudes of every term that reaches the element.

Bound, shift probe, both directions, both kernels (split-bf16 = the default, exact fp32 = cnn_dtype "fp32_exact"), every element:
    |kernel - oracle64| <= BOUND_UNITS * 2^-24 * A,     BOUND_UNITS = 4
(the 2^-22 * mag of tests/test_split_bf16.py's lane-by-lane emulation, applied to the kernel).  What makes the bound meaningful is
asserted on the CPU, on every input family: the oracle's fp32 flavour stays within 2 units, and a numpy model of the chain that
runs l_1 only, or l_last only, as "bf16 x 3" (hh, hm, mh) is at least 2 x BOUND_UNITS away.

Bound, raw probe: the same allowance on raw mapped through  d ls / d raw = rescaling_scale (1 - tanh^2 raw),  plus what tanh / exp
and the fp32 output add,  RAW_T * 2^-24 * (1 + |ls|).  The "1 +" is there because the probe observes  out = exp(+-ls):  a RELATIVE
error of exp, and the rounding of `out` to fp32 itself (half an ulp = 2^-24 relative), is an ABSOLUTE error of log(out), however
small ls is (in units of 2^-24 |ls| alone the oracle's fp32 flavour reaches 32 on elements with |ls| < 0.05, so a T of that form
would have to be ~130 and would hide the conv term).  Measured on the CPU in units of 2^-24 (1 + |ls|), on all five families x 3
seeds x both directions, with the conv allowance taken off: the oracle's fp32 flavour is at most 2.16 and the plain-C oracle at most
0.94 from the fp64 oracle (printed and asserted by test_raw_probe_fp32_flavours_and_the_mutant_on_the_cpu); x 4 because the kernels
use hardware exp2 / rcp instead of libm, rounded up: RAW_T = 9.  Neither GPU kernel entered that number.  The same CPU test holds
the l_last three-product mutant to >= 2 x the resulting bound on every family (it is at 3.8 .. 5.5 x).
"""
import numpy as np
import pytest

from conftest import trained_like_variables
from test_split_bf16 import FAMILIES, _fold_layout, _split3, family

BOUND_UNITS = 4.0
RAW_T = 9.0
U24 = 2.0 ** -24
SEEDS = (11, 12, 13)
T = "model/real_nvp_conv_template/"


# ---- the probe model ----------------------------------------------------------------------------------------------------------

def probe_variables(seed, half, width=4):
    """`unc`, trained-like coupling weights and BN statistics, the 1x1 mix the LU form of the identity; `half` =
    "shift": the raw channels of l_last are zero, "raw": the shift channels are.  Beyond width 4 the weights of l_2 and l_last are
    scaled by sqrt(4 / width), as tests/test_gpu_gemm.py::_variables does: activations of O(1) at every width."""
    from oracle.nf_oracle import conv1x1_variable_names
    v = trained_like_variables("unc", width, seed=seed)
    if width > 4:
        for k in v:
            if k.endswith("l_2/W") or k.endswith("l_last/W"):
                v[k] = (v[k] * np.float32((4.0 / width) ** 0.5)).astype(np.float32)
    n = conv1x1_variable_names(0, "LU")
    v[n["P"]] = np.eye(4, dtype=np.float32)
    v[n["sign_S"]] = np.ones(4, np.float32)
    v[n["log_S"]] = np.zeros(4, np.float32)
    v[n["L_vec"]] = np.zeros_like(v[n["L_vec"]])
    v[n["U_vec"]] = np.zeros_like(v[n["U_vec"]])
    W, b = v[T + "l_last/W"].copy(), v[T + "l_last/b"].copy()
    dead = slice(2, 4) if half == "shift" else slice(0, 2)
    W[..., dead] = 0.0
    b[..., dead] = 0.0
    v[T + "l_last/W"], v[T + "l_last/b"] = W, b
    return v


def probe_input(z0, half):
    x = np.zeros(z0.shape[:3] + (4,), np.float32)
    x[..., :2] = z0
    if half == "raw":
        x[..., 2:] = 1.0
    return x


def _folded(p):
    """BN-eval and exp(3 logs) folded into weights and biases (fp64), as oracle.coupling_cnn applies them."""
    from oracle.nf_oracle import BN_EPS, LOGSCALE_FACTOR
    s1 = 1.0 / np.sqrt(p["bn1/var"] + BN_EPS)
    s2 = 1.0 / np.sqrt(p["bn2/var"] + BN_EPS)
    es = np.exp(p["l_last/logs"] * LOGSCALE_FACTOR)
    return (p["l_1/W"] * s1, (p["l_1/b"] - p["bn1/mean"]) * s1, p["l_2/W"] * s2, (p["l_2/b"] - p["bn2/mean"]) * s2,
            p["l_last/W"] * es, p["l_last/b"] * es)


def abs_terms(p, z0):
    """A [B, H, W, 4] (shift channels, raw channels): the fp64 sum of absolute terms carried through l_1 -> l_2 -> l_last."""
    from oracle.nf_oracle import add_edge_padding, conv2d_nhwc
    W1, b1, W2, b2, W3, b3 = (np.abs(a) for a in _folded(p))
    a1 = conv2d_nhwc(np.abs(np.asarray(z0, np.float64)), W1, True) + b1
    a2 = conv2d_nhwc(a1, W2, True) + b2
    return conv2d_nhwc(add_edge_padding(a2), W3, False) + b3


def _params64(v):
    from oracle.nf_oracle import bind_variables
    return [L for L in bind_variables("unc", v) if L["type"] == "coupling"][0]["p"]


def chain_emulated(p, z0, prods1, prods3, prods2=None):
    """(shift, raw) of the chain as a split-bf16 kernel evaluates it: folded fp32 weights and fp32 activations in three bf16
    pieces, the listed piece products (weight piece, activation piece) exact and summed in fp64, one fp32 rounding per layer;
    l_2 in fp32 unless it has a product list of its own.  prods = SIX for the kernel of DESIGN 4.1, THREE for the mutant, None for
    the layer as an ideal fp32 evaluation (the fp32 operands' exact products, one rounding).  Any width, any patch shape."""
    from oracle.nf_oracle import add_edge_padding, conv2d_nhwc
    W1, b1, W2, b2, W3, b3 = (np.asarray(a, np.float32) for a in _folded(p))
    f32 = lambda a: np.asarray(a, np.float32)   # noqa: E731
    w = W2.shape[-1]
    pad1 = [(0, 0), (1, 1), (1, 1), (0, 0)]
    if prods1 is None:
        h = conv2d_nhwc(np.asarray(z0, np.float64), W1.astype(np.float64), True)
    else:
        zp, wp = _split3(z0), _split3(W1)
        h = sum(conv2d_nhwc(zp[b], wp[a], True) for a, b in prods1)
    h = np.maximum(f32(h + b1.astype(np.float64)), 0)
    if prods2 is None:
        h2 = conv2d_nhwc(h.astype(np.float64), W2.astype(np.float64), True)
    else:
        hp, wp = _split3(h), _split3(W2)
        h2 = sum(conv2d_nhwc(hp[b], wp[a], True) for a, b in prods2)
    h = np.maximum(f32(h2 + b2.astype(np.float64)), 0)
    edge = conv2d_nhwc(add_edge_padding(np.zeros(h.shape))[..., w:], W3[:, :, w:, :].astype(np.float64), False)
    if prods3 is None:
        o = conv2d_nhwc(np.pad(h.astype(np.float64), pad1), W3[:, :, :w, :].astype(np.float64), False)
    else:
        hp, wp = _split3(h), _split3(W3[:, :, :w, :])
        o = sum(conv2d_nhwc(np.pad(hp[b], pad1), wp[a], False) for a, b in prods3)
    o = f32(o + edge + b3.astype(np.float64)).astype(np.float64)
    return o[..., :2], o[..., 2:]


SIX = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]
THREE = [(0, 0), (0, 1), (1, 0)]


def _units(err, A):
    return float((np.abs(err) / (U24 * A)).max())


def raw_bound(p, A_raw, raw64, units=BOUND_UNITS, raw_t=RAW_T):
    """Per-element allowance on ls = rescaling_scale * tanh(raw) as log(out) shows it (module docstring); `units` = the conv
    bound in units of 2^-24 A (BOUND_UNITS here, the per-width table of tests/test_gpu_probe_families.py there)."""
    rs = float(p["rescaling_scale"])
    t = np.tanh(raw64)
    ls = rs * t
    conv = units * U24 * A_raw * rs * (1.0 - t * t)
    return conv, conv + raw_t * U24 * (1.0 + np.abs(ls)), ls


# ---- CPU: the two conditions that give the bound its meaning ------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_probe_mix_folds_to_the_exact_identity(seed):
    from noise_flow_amd import _lib
    for half in ("shift", "raw"):
        v = probe_variables(seed, half)
        for path in (_lib.NF_PATH_SPLIT_BF16, _lib.NF_PATH_MFMA4):
            for direction in (0, 1):
                flags = _lib.NF_CFG_EXACT_FP32 if path == _lib.NF_PATH_MFMA4 else 0
                ops, blk = _fold_layout("unc", v, path, flags=flags, direction=direction)
                mixes = [o for t, o in ops if t == _lib.NF_OP_MIX]
                assert len(mixes) == 1 and sorted(t for t, _ in ops) == [_lib.NF_OP_MIX, 2 + direction]
                got = blk[mixes[0]:mixes[0] + 16].view(np.uint32)
                np.testing.assert_array_equal(got, np.eye(4, dtype=np.float32).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("name", FAMILIES)
def test_shift_probe_fp32_flavour_within_half_the_bound_and_three_product_mutants_beyond_twice_it(name):
    from oracle.nf_oracle import coupling_cnn
    worst32 = worst6 = 0.0
    mut1 = mut3 = 0.0
    for seed in SEEDS:
        v = probe_variables(seed, "shift")
        p = _params64(v)
        p32 = {k: np.asarray(a, np.float32) for k, a in p.items()}
        z0 = family(name, seed)
        A = abs_terms(p, z0)[..., :2]
        ref = coupling_cnn(z0.astype(np.float64), p)[0]
        worst32 = max(worst32, _units(coupling_cnn(z0, p32)[0].astype(np.float64) - ref, A))
        worst6 = max(worst6, _units(chain_emulated(p, z0, SIX, SIX)[0] - ref, A))
        # a mutant must be caught on some seed's input of EVERY family; the worst element over the seeds is what the GPU test sees
        mut1 = max(mut1, _units(chain_emulated(p, z0, THREE, SIX)[0] - ref, A))
        mut3 = max(mut3, _units(chain_emulated(p, z0, SIX, THREE)[0] - ref, A))
    print("\nshift probe, %s, units of 2^-24 A: fp32 flavour %.2f, six products %.2f, three products in l_1 only %.1f, in l_last "
          "only %.1f" % (name, worst32, worst6, mut1, mut3))
    assert worst32 <= BOUND_UNITS / 2, worst32
    assert worst6 <= BOUND_UNITS / 2, worst6
    assert mut1 >= 2 * BOUND_UNITS, mut1
    assert mut3 >= 2 * BOUND_UNITS, mut3


def test_raw_probe_fp32_flavours_and_the_mutant_on_the_cpu():
    """RAW_T: how far the fp32 evaluations of tanh / exp sit from fp64, in units of 2^-24 (1 + |ls|), once the conv allowance
    is taken off; RAW_T / 4 must cover them (the factor 4 is for hardware exp2 / rcp), and the l_last three-product mutant must
    exceed the whole bound 2x on every family."""
    from oracle.nf_oracle import NoiseFlowOracle, coupling_cnn
    from oracle.nf_oracle_c import COracle
    t_np = t_c = 0.0
    for name in FAMILIES:
        mut = 0.0
        for seed in SEEDS:
            v = probe_variables(seed, "raw")
            p = _params64(v)
            z0 = family(name, seed)
            x = probe_input(z0, "raw")
            raw64 = coupling_cnn(z0.astype(np.float64), p)[1]
            conv, bound, ls = raw_bound(p, abs_terms(p, z0)[..., 2:], raw64)
            o32 = NoiseFlowOracle("unc", v, dtype=np.float32)
            oc = COracle("unc", v)
            outs = {"np": (o32.inverse(x)[0], o32.forward(x)), "c": (oc.nll(x, want_z=True)[2], oc.sample(x, 1.0))}
            for k, (inv, fwd) in outs.items():
                e = np.maximum(np.abs(np.log(inv[..., 2:].astype(np.float64)) - ls), np.abs(np.log(fwd[..., 2:].astype(np.float64)) + ls))
                t = float((np.maximum(e - conv, 0) / (U24 * (1 + np.abs(ls)))).max())
                if k == "np":
                    t_np = max(t_np, t)
                else:
                    t_c = max(t_c, t)
            rs = float(p["rescaling_scale"])
            m_ls = rs * np.tanh(chain_emulated(p, z0, SIX, THREE)[1])
            mut = max(mut, float((np.abs(m_ls - ls) / bound).max()))
        print("\nraw probe, %s: three products in l_last only at %.1f x the bound" % (name, mut))
        assert mut >= 2.0, (name, mut)
    print("raw probe: tanh / exp of the fp32 flavour %.2f, of the plain-C oracle %.2f units of 2^-24 (1 + |ls|); RAW_T = %g"
          % (t_np, t_c, RAW_T))
    assert 4.0 * max(t_np, t_c) <= RAW_T, (t_np, t_c)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def _model(v, cnn_dtype):
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    m = NoiseFlow([32, 32, 4], False, default_hps(arch="unc", width=4), variables=v, cnn_dtype=cnn_dtype)
    want = _lib.NF_PATH_SPLIT_BF16 if cnn_dtype == "fp32" else _lib.NF_PATH_MFMA4
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (cnn_dtype, direction)
    return m


_ARGS = ([0.0], [0.0], [100], [0])


@pytest.mark.gpu
@pytest.mark.parametrize("cnn_dtype", ["fp32", "fp32_exact"])
@pytest.mark.parametrize("seed", SEEDS)
def test_shift_probe_kernel_within_four_units_of_the_fp64_chain(seed, cnn_dtype):
    """Measured on an MI355X, worst element over the 3 seeds x 5 families in units of 2^-24 A: split kernel 1.25 (impulse in a
    corner), exact kernel 1.71 (wide_range), the same in both directions."""
    from oracle.nf_oracle import coupling_cnn
    v = probe_variables(seed, "shift")
    p = _params64(v)
    m = _model(v, cnn_dtype)
    lines, bad = [], []
    for name in FAMILIES:
        z0 = family(name, seed)
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
            lines.append("%s %s %s seed %d: worst %.3f units of 2^-24 A at (patch, row, col, ch) = %s"
                         % (cnn_dtype, name, tag, seed, u.max(), tuple(int(i) for i in at)))
            if not u.max() <= BOUND_UNITS:
                bad.append(lines[-1])
        assert np.all(np.asarray(obj) == 0.0), (name, "ls = 0 exactly: the log-det must be zero")
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("cnn_dtype", ["fp32", "fp32_exact"])
@pytest.mark.parametrize("seed", SEEDS)
def test_raw_probe_kernel_log_scale_and_log_det(seed, cnn_dtype):
    """log(out) = +-ls per element within the conv allowance mapped through tanh plus RAW_T 2^-24 (1 + |ls|); per-patch log-det
    within the sum of the elements' allowances plus 16 x 2^-24 sum |ls| for the fp32 summation of 2 048 terms (the constant of
    conftest.GRAD_NOISE_C)."""
    from oracle.nf_oracle import coupling_cnn
    v = probe_variables(seed, "raw")
    p = _params64(v)
    m = _model(v, cnn_dtype)
    lines, bad = [], []
    for name in FAMILIES:
        z0 = family(name, seed)
        x = probe_input(z0, "raw")
        raw64 = coupling_cnn(z0.astype(np.float64), p)[1]
        conv, bound, ls = raw_bound(p, abs_terms(p, z0)[..., 2:], raw64)
        z, obj = m.inverse(x, None, None, *_ARGS)
        xs = m.forward(x, None, None, *_ARGS)
        for tag, out, want in (("inverse", z, ls), ("forward", xs, -ls)):
            out = np.asarray(out)
            assert np.array_equal(out[..., :2], z0), (name, tag, "the pass-through half changed")
            r = np.abs(np.log(out[..., 2:].astype(np.float64)) - want) / bound
            at = np.unravel_index(np.argmax(r), r.shape)
            lines.append("%s %s %s seed %d: worst %.3f of the bound at %s" % (cnn_dtype, name, tag, seed, r.max(), tuple(int(i) for i in at)))
            if not r.max() <= 1.0:
                bad.append(lines[-1])
        ld_ref = ls.sum(axis=(1, 2, 3))
        ld_tol = conv.sum(axis=(1, 2, 3)) + 16.0 * U24 * np.abs(ls).sum(axis=(1, 2, 3))
        ld_err = np.abs(np.asarray(obj, np.float64) - ld_ref)
        lines.append("%s %s log-det seed %d: worst %.3f of its allowance" % (cnn_dtype, name, seed, (ld_err / ld_tol).max()))
        if not np.all(ld_err <= ld_tol):
            bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
