"""CPU tier of the rule the nf_nll_grad kernels are held to (tests/nll_grad_ref.py): what the two norms can and cannot see, shown
on the reference alone for EVERY accuracy case of tests/test_gpu_nll_grad.py, test_gpu_nll_grad_wide.py and
test_gpu_nll_grad_tiled.py (the case lists are those modules' own constants).  No device is touched.

Per case:
  * the preconditions the GPU test asserts (pinned e32 <= E32_MAX in both norms, the kink count, the dynamic range where asked);
  * the hand-written backward sweep in fp64, stored and reversible, against torch.autograd at 1e-12 of max|grad|;
  * the two float32 flavours of the sweep (stored activations; the reversible arithmetic of csrc/nf_grad.hip) within HALF the
    bound in both norms — or named in HALF_BOUND_MISSES with the figure;
  * the mutants, each in fp64: beyond TWICE the combined bound on at least one element, or listed in DROPPED with the ratio.
The table printed with -s says for every mutant and case whether the raw norm alone (the rule before the whitened norm) saw it.
"""
import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables
import nll_grad_ref as R
import test_gpu_nll_grad as S
import test_gpu_nll_grad_tiled as T
import test_gpu_nll_grad_wide as Wd
from test_grad_tiles_cpu import _tiled_gradients
from test_grad_wide_supported_cpu import NO_SDN_ARCH, paper_like_variables

ISO, CAM = S.ISO, S.CAM
ROWS5 = np.array([(i, c, 0, 0) for i, c in S.TUPLES5], np.float32)


def _specs():
    """(label, model key, arch, width, (H, W), inputs key, iso, cam, hps, min_gy_range) of every accuracy case of the GPU files."""
    out = []
    add = lambda *a, hps=(), rng=None: out.append(a + (dict(hps), rng))   # noqa: E731
    for hw, seed in S.SHIPPED_CASES:
        add("scalar shipped %dx%d" % hw, "shipped", FULL_ARCH, 4, hw, ("std", 3, seed), ISO, CAM, rng=S.GY_RANGE if hw in S.GY_RANGE_CASES else None)
    for w, hw, seed in S.TRAINED_CASES:
        add("scalar trained w%d %dx%d" % ((w,) + hw), "trained", S.WIDE_ARCH, w, hw, ("std", 3, seed), ISO, CAM)
    add("scalar vocab per-call", "vocab", S.VOCAB_ARCH, 4, (12, 12), ("std", 3, 0), 1600.0, 3.0)
    add("scalar vocab rows", "vocab", S.VOCAB_ARCH, 4, (12, 12), ("std", 5, 1), ROWS5[:, 0], ROWS5[:, 1])
    add("scalar vocab perm0", "vocab", S.VOCAB_ARCH, 4, (12, 12), ("std", 3, 2), 400.0, 1.0, hps={"flow_permutation": 0})
    add("scalar vocab NONE", "vocab", S.VOCAB_ARCH, 4, (12, 12), ("std", 3, 2), 400.0, 1.0, hps={"decomp": "NONE"})
    add("scalar no-sdn 8x8", "nosdn", "unc|gain4|unc", 4, (8, 8), ("randn", 3, 0), None, None)
    for hw in T.SHIPPED_CASES:
        add("tiled shipped %dx%d" % hw, "shipped", FULL_ARCH, 4, hw, ("std", 2, 0), ISO, CAM, rng=S.GY_RANGE if hw in T.GY_RANGE_CASES else None)
    add("tiled shipped 80x72", "shipped", FULL_ARCH, 4, (80, 72), ("std", 2, 0), ISO, CAM)
    for w, hw, seed in T.TRAINED_CASES:
        add("tiled trained w%d %dx%d" % ((w,) + hw), "trained", S.WIDE_ARCH, w, hw, ("std", 2, seed), ISO, CAM)
    add("tiled vocab per-call", "vocab", S.VOCAB_ARCH, 4, (70, 36), ("std", 3, 0), 1600.0, 3.0)
    add("tiled vocab rows", "vocab", S.VOCAB_ARCH, 4, (70, 36), ("std", 3, 0), ROWS5[:3, 0], ROWS5[:3, 1])
    add("tiled no-sdn 66x12", "nosdn", T.NO_SDN_ARCH, 4, (66, 12), ("randn", 2, 0), None, None)
    for w, hw, B, seed in Wd.FULL_DEPTH_CASES:
        add("wide full w%d %dx%d" % ((w,) + hw), "paper", FULL_ARCH, w, hw, ("named",) if B == 0 else ("std", B, seed), ISO, CAM)
    add("wide full w32 32x32 shipped sdn", "paper sdn", FULL_ARCH, 32, (32, 32), ("named sdn",), ISO, CAM, rng=S.GY_RANGE)
    add("wide full w32 24x24", "paper", FULL_ARCH, 32, (24, 24), ("std", 2, 0), ISO, CAM)
    for arch, w, hw in Wd.SCALED_CASES:
        if arch == NO_SDN_ARCH:
            add("wide no-sdn w%d %dx%d" % ((w,) + hw), "paper", arch, w, hw, ("x only", 3, 0), None, None)
        else:
            add("wide scaled w%d %dx%d" % ((w,) + hw), "paper", arch, w, hw, ("std", 3, 0), ISO, CAM)
    add("wide vocab per-call", "vocab", S.VOCAB_ARCH, Wd.VW, (12, 12), ("std", 3, 0), 1600.0, 3.0)
    add("wide vocab rows", "vocab", S.VOCAB_ARCH, Wd.VW, (12, 12), ("std", 5, 1), ROWS5[:, 0], ROWS5[:, 1])
    add("wide vocab perm0", "vocab", S.VOCAB_ARCH, Wd.VW, (12, 12), ("std", 3, 2), 400.0, 1.0, hps={"flow_permutation": 0})
    add("wide vocab NONE", "vocab", S.VOCAB_ARCH, Wd.VW, (12, 12), ("std", 3, 2), 400.0, 1.0, hps={"decomp": "NONE"})
    return out


SPECS = _specs()
LABELS = [s[0] for s in SPECS]
_REFS, _INPUTS = {}, {}


def _case(spec, shipped_variables):
    """(reference, width, x, y, iso, cam, min_gy_range) of a spec; references per model and inputs per (shape, key) are built once."""
    label, model, arch, width, hw, ikey, iso, cam, hps, rng = spec
    rkey = (model, arch, width, tuple(sorted(hps.items())))
    if rkey not in _REFS:
        if model == "shipped":
            v = shipped_variables
        elif model == "trained":
            v = trained_like_variables(arch, width)
        elif model == "nosdn":
            v = trained_like_variables(arch, width, seed=3)
        elif model == "paper":
            v = paper_like_variables(arch, width)
        elif model == "paper sdn":
            v = Wd.shipped_sdn_variables(shipped_variables, width)
        else:
            v = (S._vocab_variables if width == 4 else Wd._vocab_variables)(hps.get("decomp", "LU"))
        _REFS[rkey] = R.PinnedRef(arch, v, **{k: hps[k] for k in ("flow_permutation", "decomp") if k in hps})
    if (hw, ikey) not in _INPUTS:
        if ikey[0] == "named":
            x, y = Wd._inputs_32x32_w32()
        elif ikey[0] == "named sdn":
            x, y = Wd.inputs_32x32_shipped_sdn()
        elif ikey[0] == "randn":
            x, y = np.random.RandomState(ikey[2]).randn(ikey[1], hw[0], hw[1], 4).astype(np.float32), None
        else:
            x, y = make_inputs(ikey[1], hw[0], hw[1], seed=ikey[2])
            if ikey[0] == "x only":
                y = None
        _INPUTS[(hw, ikey)] = (x, y)
    x, y = _INPUTS[(hw, ikey)]
    return _REFS[rkey], width, x, y, iso, cam, rng


# ---- the sweep is autograd; the float32 flavours sit within half the bound ---------------------------------------------------------
# label -> {(flavour, tensor and norm): measured distance / bound}: the float32 flavours that are NOT within half the bound; they
# are held to the bound itself.  The yardstick a kernel finding on that case is judged against.
#   tiled shipped 65x64: the reversible flavour's gx of image 0 is 7.2e-6 of max|gx| (bound 1e-5, e32 1.6e-6; stored 1.4e-6) and
#   1.7e-6 whitened: the pixel that carries max|gx| has the largest 1 / s and a quarter of max|gx s|, so the sweep's uniform
#   absolute round-off in gx s is four times as large relative to it.  (The tiled kernel stores the tensors between its
#   segments, so this whole-image figure is an upper mark for it, not its arithmetic.)
HALF_BOUND_MISSES = {"tiled shipped 65x64": {("reversible", "gx"): 0.72}}


@pytest.mark.parametrize("label", LABELS)
def test_sweep_and_flavours(shipped_variables, label):
    ref, width, x, y, iso, cam, rng = _case(SPECS[LABELS.index(label)], shipped_variables)
    e32 = R.reference_conditions(ref, width, x, y, iso, cam, min_gy_range=rng)
    _, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam)
    wx, wy = R.rule_weights(ref, y, iso, cam, x.shape)
    tensors = [("gx", gx64, wx)] + ([("gy", gy64, wy)] if gy64 is not None else [])
    for reversible in (False, True):
        got = R.backward_sweep(ref, x, y, iso, cam, np.float64, reversible)
        for (name, r64, _), g in zip(tensors, got):
            d = float(R.patch_rel_err(g, r64).max())
            assert d <= 1e-12, (name, reversible, d)
    assert (gy64 is None) == (got[1] is None)
    misses = {}
    for flavour, reversible in (("stored", False), ("reversible", True)):
        got = R.backward_sweep(ref, x, y, iso, cam, np.float32, reversible)
        for (name, r64, w), g in zip(tensors, got):
            for tag, wt in (("", None), ("/w", w)):
                d = R.patch_rel_err(g, r64, wt)
                tol = np.maximum(R.REL_TOL, R.E32_FACTOR * e32[name + tag])
                print("%-28s %-10s %-5s %.2e (e32 %.2e)" % (label, flavour, name + tag, d.max(), e32[name + tag].max()))
                listed = (flavour, name + tag) in HALF_BOUND_MISSES.get(label, {})
                if not np.all(d <= (1.0 if listed else 0.5) * tol):
                    misses[(flavour, name + tag)] = float((d / tol).max())
    assert not misses, misses


def test_leading_layers_take_their_values_forward():
    """Why the kernel recomputes the layers in front of the first coupling from x: rebuilt through the whole stack in float32, x
    comes back ~1e-4 off, and gy of the leading sdn layer — (a / 2 s^2) (1 - g z), a difference of O(1) terms — inherits it.
    ``sdn5|unc|unc|gain4|unc`` at width 16 on 16x16: rebuilt, gy misses the rule; forward, it is at the stored flavour's distance."""
    spec = SPECS[LABELS.index("scalar trained w16 16x16")]
    ref, width, x, y, iso, cam, _ = _case(spec, None)
    _, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam)
    bound = R.combined_bound(ref, x, y, iso, cam)
    rebuilt = R.backward_sweep(ref, x, y, iso, cam, np.float32, True, leading_forward=False)
    forward = R.backward_sweep(ref, x, y, iso, cam, np.float32, True)
    r_gy, f_gy = float(R.patch_rel_err(rebuilt[1], gy64).max()), float(R.patch_rel_err(forward[1], gy64).max())
    print("gy, leading layers rebuilt %.2e, taken forward %.2e of max|gy|" % (r_gy, f_gy))
    assert _ratios(bound, rebuilt, (gx64, gy64))[0] > 1.0 and _ratios(bound, forward, (gx64, gy64))[0] <= 0.5


# ---- the mutants -----------------------------------------------------------------------------------------------------------------------
# (label, mutant) -> measured worst-element ratio to the combined bound: mutants the rule cannot resolve on that case
# (gx_element: the perturbed element is one whose |gx| / w_x is below 2 % of the patch's largest on every patch of the case)
# (tiled shipped 64x65: 2.5 with this host's e32 of 2.7e-6 in the bound; another host CPU's 3.6e-6 takes it to 2 — not relied on)
DROPPED = {("tiled shipped 80x72", "gx_element"): 0.58, ("tiled vocab rows", "gx_element"): 1.81, ("tiled shipped 64x65", "gx_element"): 2.5}
DROPPED_LEAVES_AT = 4.0      # a dropped mutant that reaches this ratio is resolved after all and leaves the table
NEVER_DROPPED_ON_SHIPPED = ("l1_tap", "no_logdet", "gy_element")
SEAM_PIXEL = 256


def _mutants(ref, x, y, iso, cam, gx64, gy64, wy):
    """{name: (gx, gy)} of every mutant that applies to the case."""
    layers = ref.layers
    cpl = [i for i, L in enumerate(layers) if L["type"] == "coupling"]
    sdn = [i for i, L in enumerate(layers) if L["type"].startswith("sdn")]
    B, H, W, _ = x.shape
    out = {}
    mid = cpl[len(cpl) // 2]
    if H >= 2 and W >= 2:
        out["l1_tap"] = R.backward_sweep(ref, x, y, iso, cam, mutant=("l1_tap", mid))
    out["no_logdet"] = R.backward_sweep(ref, x, y, iso, cam, mutant=("no_logdet", None))
    if len(sdn) >= 2:
        out["gy_not_added"] = R.backward_sweep(ref, x, y, iso, cam, mutant=("gy_not_added", sdn[-1]))
    if H * W > SEAM_PIXEL:
        g = gx64.copy().reshape(B, H * W, 4)
        g[:, SEAM_PIXEL, 0] *= 1.0 + 1e-3
        out["gx_element"] = (g.reshape(gx64.shape), gy64)
    if gy64 is not None:
        g = gy64.copy().reshape(B, -1)
        for b in range(B):
            order = np.argsort(wy[b].reshape(-1), kind="stable")
            g[b, order[order.size // 2]] *= 1.0 + 1e-3
        out["gy_element"] = (gx64, g.reshape(gy64.shape))
    return out


def _ratios(bound, got, ref64):
    """(worst element over the combined bound, over the raw bound alone) of a mutant, the weakest patch of each left aside: the
    worst element of the case."""
    worst, worst_raw = 0.0, 0.0
    for name, g, r in zip(("gx", "gy"), got, ref64):
        if r is None:
            continue
        d = np.abs(g - r)
        worst = max(worst, float((d / bound[name][0]).max()))
        worst_raw = max(worst_raw, float((d / bound[name][1]).max()))
    return worst, worst_raw


@pytest.mark.parametrize("label", LABELS)
def test_mutants_exceed_twice_the_bound(shipped_variables, label):
    spec = SPECS[LABELS.index(label)]
    ref, width, x, y, iso, cam, _ = _case(spec, shipped_variables)
    _, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam)
    _, wy = R.rule_weights(ref, y, iso, cam, x.shape)
    bound = R.combined_bound(ref, x, y, iso, cam)
    failures = []
    for name, got in _mutants(ref, x, y, iso, cam, gx64, gy64, wy).items():
        ratio, raw = _ratios(bound, got, (gx64, gy64))
        dropped = (label, name) in DROPPED
        print("%-28s %-13s %9.3g x the combined bound;  the raw norm alone: %9.3g x  (%s)%s"
              % (label, name, ratio, raw, "seen" if raw > 1.0 else "MISSED by the raw norm", "  DROPPED" if dropped else ""))
        if dropped:
            assert ratio < DROPPED_LEAVES_AT, (label, name, ratio)
        elif not ratio >= 2.0:
            failures.append((name, ratio))
    assert not failures, failures


# the tile plan with a halo one pixel short: segments of 1 and of 2 couplings of the shipped model's leading layers, 90x70 image
# segments of 2 couplings: 2.9e-4 of the combined bound — no fp32 rule resolves it; tests/test_grad_tiles_cpu.py pins it in fp64
HALO_DROPPED = {2: 2.9e-4}


@pytest.mark.parametrize("arch,c", [("sdn5|unc", 1), ("sdn5|unc|unc", 2)])
def test_short_halo_mutant(shipped_variables, arch, c):
    ref = R.PinnedRef(arch, shipped_variables)
    x, y = make_inputs(1, 90, 70, seed=0)
    _, gx64, gy64 = ref.nll_and_grads(x, y, ISO, CAM)
    bound = R.combined_bound(ref, x, y, ISO, CAM)
    exact = _tiled_gradients(ref, x, y, 4 * c, 32)
    assert _ratios(bound, exact, (gx64, gy64))[0] <= 1e-6                  # the full halo is the whole image's gradient
    ratio, raw = _ratios(bound, _tiled_gradients(ref, x, y, 4 * c - 1, 32), (gx64, gy64))
    print("halo %d of %d, %d coupling(s): %9.3g x the combined bound;  the raw norm alone: %9.3g x  (%s)"
          % (4 * c - 1, 4 * c, c, ratio, raw, "seen" if raw > 1.0 else "MISSED by the raw norm"))
    if c in HALO_DROPPED:
        assert ratio < 2.0, ratio
    else:
        assert ratio >= 2.0, ratio


def test_dropped_table():
    """Dropping is capped: never one of the two structural coupling mutants or the single-element gy mutant on the shipped model
    (there a miss says the weights are wrong, not the mutant); every entry names a case and a mutant that exist."""
    for (label, name), ratio in DROPPED.items():
        assert label in LABELS and ratio < DROPPED_LEAVES_AT
        assert not ("shipped" in label and name in NEVER_DROPPED_ON_SHIPPED), (label, name)
    assert set(HALO_DROPPED) <= {2}
