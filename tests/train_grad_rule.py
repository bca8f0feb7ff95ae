"""The rule the training step's gradients are held to: fp32 resolution, measured by the oracle alone.

For every trainable tensor T of a step except l_1/b and l_2/b (analytically zero: they keep their absolute rule), per entry

    |g_kernel - g64|  <=  max( max(1e-5, 4 e32_T) * s_T ,  grad_noise_allowance(oracle, T)[entry] )
    s_T   = max(max|g64_T|, 1e-6 * gmax)
    e32_T = max|g32_T - g64_T| / s_T

g64 is ``GradOracle`` (fp64 autograd).  g32 is the same op sequence in torch.float32 with every ReLU gate pinned to the gate the
fp64 evaluation took on the same input (``RuleOracle``), so e32 is round-off alone: a gate a plain fp32 run flips is the kink
rule's business (conftest.py::grads_match_up_to_kinks), not a reason for a wider tolerance.  1e-5 is the project's tensor
tolerance; 4 is the factor tests/test_gpu_nll_grad.py uses for another summation order.  Nothing a kernel computes enters the bound.

Preconditions, asserted from the reference alone before a kernel's output is looked at (``Case.assert_admissible``):
  * every e32_T <= E32_MAX = 2.5e-5, so the relative part never exceeds 1e-4;
  * at most MAX_CANDIDATES = 64 activations on their ReLU kink (``Case.candidates``); at most MAX_EXCUSED = 2 may be excused.
A case that misses one gets another seed or input; the caps do not move.

Every evaluation (fp64, pinned fp32, each flipped subset) is memoised per (model, input): ``case(...)`` returns the same ``Case``
for the same model and input, and its oracle answers a repeated ``loss_and_grads`` from the memo.

For one release ``check_grads`` also asserts, entry by entry, that the bound is not above the one it replaces (``old_tol`` of
the tensor's scale, with the allowance where the replaced comparison had it; a comparison that had none gets the allowance capped
by its old tolerance), so no edited test can have got weaker.

Open.  Every kernel path of the trainer meets the rule on every admissible case but four tensors, each just outside the floor of
1e-5 on a case of a hundred to a few hundred pixels, and one whole case; they keep the 1e-3 they had (``exclude=`` at the call, named
there) until shown to be a slip or modelled:
  * matrix-core stages (NF_TRAIN_WIDE_MFMA=4095), ``unc`` at width 32 on three 5x7 patches: l_1/W 1.1e-5, l_2/W 1.43e-5 of the
    tensor's scale (e32 5e-7); the layer kernels are at 1.6e-6 on the same case;
  * GEMM route, ``unc`` at width 200 on one 16x24 patch: l_1/W 1.44e-5 (e32 4e-7);
  * GEMM route, ``sdn5|unc|gain4`` at width 132 on three 7x5 patches: l_2/W 1.08e-5 (e32 6e-7), fp32 and bf16 x 6 products alike;
  * GEMM route, 17 couplings of width 12 on three 6x6 patches (every tensor kept at 1e-3): l_1/W 2.4e-5 (e32 2.2e-6), a mixing L_vec
    2.6e-5 (e32 4.7e-6), l_2/W 1.4e-5.  (On another input of that case, noise of b1 = 0.03, the kernels met the rule with 1.8e-5 on a
    rescaling_scale0 at most — but its e32 was 1.2e-5 on one host CPU and 2.2e-5 on another, too near the cap to rely on.)
What reading the kernels gives for the first two and the last: the finalisers form the batch variance as E[h^2] - E[h]^2 from fp32 partial sums
(csrc/nf_train.hip::bn_from_slots, k_bn_fin), torch in two passes.  Those two models have no sdn layer in front, their l_1
activations are a bias plus a small signal (mean^2 / variance up to 167), and the same float32 evaluation with the one-pass variance
(``RuleOracle(one_pass_variance=True)``) moves e32 of exactly these tensors from 5.9e-7 / 5.3e-7 / 3.9e-7 to 6.1e-6 / 7.4e-6 /
3.4e-6, and e32 of the seventeen l_1/W of the last case from 2e-6 .. 9e-6 to 2e-5 .. 9e-5 (tests/test_train_grad_rule_cpu.py).  It is not the yardstick: with it the 5x7 case would pass (bound 2.4e-5 / 3.0e-5), the
width-200 case would not (1.38e-5 against 1.44e-5), and the 17-coupling case at width 12 would leave the precondition (e32 above
1e-4 on every input tried), so what the kernels' own summation adds is not yet modelled.  The width-132 item is not explained.

Not admissible.  Three cases of the GPU tests have more than MAX_CANDIDATES activations on their kink at any input of their size (1100
patches of 8x8 at width 32: 373; ``unc|unc`` at width 96 on six 32x32 patches: 215; eight patches on the patch-resident persistent
loop: 66).  They stay, at the 1e-3 they had, for the kernel paths only their size reaches (``hold_to_rule(admissible=False)``), each
next to a smaller twin that is held to the rule.
"""
import hashlib

import numpy as np
import torch

from conftest import GRAD_NOISE_C, MAX_EXCUSED_KINKS, grad_noise_allowance, grads_match_up_to_kinks  # noqa: F401
from oracle.nf_grad_oracle import BN_EPS, GradOracle, is_trainable

REL_TOL = 1e-5          # the project's tensor tolerance
E32_FACTOR = 4.0        # another summation order of the same fp32 arithmetic (tests/test_gpu_nll_grad.py)
E32_MAX = 2.5e-5        # precondition on every tensor's pinned e32
MAX_CANDIDATES = 64     # precondition on the on-kink activations of a case
MAX_EXCUSED = 2

FAMILIES = ("l_1/W", "l_2/W", "l_last/W", "logs", "mixing", "sdn/gain", "other")


def family(name):
    for sfx in ("l_1/W", "l_2/W", "l_last/W"):
        if name.endswith(sfx):
            return sfx
    if name.endswith("l_last/logs"):
        return "logs"
    if "onv2d_1x1" in name:
        return "mixing"
    if name.startswith("model/"):
        return "sdn/gain"
    return "other"            # rescaling_scale0, l_last/b


def is_zero_bias(name):
    return name.endswith("l_1/b") or name.endswith("l_2/b")


class RuleOracle(GradOracle):
    """GradOracle that (i) answers a repeated evaluation from a memo, restoring ``kinks`` / ``grad_abs_terms`` with it, (ii) records
    the ReLU gates of its evaluation without flips (``gates``) and (iii), given ``gates=`` of another evaluation, applies those
    instead of its own signs.  ``bn`` (optional) replaces ``_bn_train``: the CPU tier's mutants."""

    def __init__(self, *a, gates=None, bn=None, one_pass_variance=False, **k):
        super().__init__(*a, **k)
        self._pin, self._bn, self.gates, self._memo, self.one_pass_variance = gates, bn, {}, {}, one_pass_variance
        self._input = None

    def _bn_train(self, h, scope, which, new_running):
        out = super()._bn_train(h, scope, which, new_running)
        if self._bn is not None:
            return self._bn(h, out)
        if self.one_pass_variance:     # the batch variance as the kernels form it: E[h^2] - E[h]^2 (see "Open" in the module docstring)
            m = h.mean(dim=(0, 2, 3), keepdim=True)
            v = torch.clamp((h * h).mean(dim=(0, 2, 3), keepdim=True) - m * m, min=0.0)
            return (h - m) / torch.sqrt(v + BN_EPS)
        return out

    def _relu(self, hn, h, amp, site, err_in=None):
        out, err = super()._relu(hn, h, amp, site, err_in)
        if not self.relu_flips:
            self.gates[site] = hn.detach() > 0
        if self._pin is not None:
            out = hn * self._pin[site].to(hn.dtype)
        return out, err

    def loss_and_grads(self, x, y, iso, cam, relu_flips=()):
        inp = (id(x), id(y), float(iso), float(cam))      # one oracle, one input: the memo is keyed on the flips alone
        assert self._input in (None, inp), "a RuleOracle memoises the evaluations of ONE input"
        self._input = inp
        key = tuple(sorted((tuple(s), int(k)) for s, k in relu_flips))
        if key not in self._memo:
            out = super().loss_and_grads(x, y, iso, cam, relu_flips)
            self._memo[key] = (out, list(self.kinks), self.grad_abs_terms, self.grad_terms)
        out, kinks, self.grad_abs_terms, self.grad_terms = self._memo[key]
        self.kinks = list(kinks)
        return out


class Case:
    """One (model, input): the fp64 evaluation, the pinned fp32 one, e32 per tensor, the on-kink candidate count."""

    def __init__(self, arch, variables, x, y, iso, cam, **oracle_kw):
        self.arch, self.variables, self.x, self.y, self.iso, self.cam, self.kw = arch, variables, x, y, iso, cam, oracle_kw
        self.oracle = RuleOracle(arch, variables, **oracle_kw)
        self.ref = self.oracle.loss_and_grads(x, y, iso, cam)           # (loss, sd_z, grads, new running statistics)
        self.candidates = len(self.oracle.kinks)
        self.abs_terms = self.oracle.grad_abs_terms                      # of the evaluation without flips
        o32 = RuleOracle(arch, variables, dtype=torch.float32, gates=self.oracle.gates, **oracle_kw)
        self.g32 = o32.loss_and_grads(x, y, iso, cam)[2]
        g64 = self.ref[2]
        self.names = [k for k in g64 if is_trainable(k)]
        self.gmax = max(np.abs(g64[k]).max() for k in self.names)
        self.e32 = {}
        for k in self.names:
            if not is_zero_bias(k):
                s = max(np.abs(g64[k]).max(), 1e-6 * self.gmax)
                self.e32[k] = float(np.abs(np.asarray(self.g32[k], np.float64) - g64[k]).max() / s)
        self.report = None
        self._plain32 = None

    def plain32(self):
        """A plain, unpinned float32 evaluation of the same graph → {name: gradient} (the CPU tier's stand-in for a kernel)."""
        if self._plain32 is None:
            o = GradOracle(self.arch, self.variables, dtype=torch.float32, **self.kw)
            self._plain32 = o.loss_and_grads(self.x, self.y, self.iso, self.cam)
        return self._plain32

    def assert_admissible(self, exclude=()):
        """`exclude`: tensors the test holds to the round-off allowance alone (a gradient that cancels to nothing: its e32 is 1)."""
        worst = max((k for k in self.e32 if k not in exclude), key=self.e32.get, default=None)
        if worst is None:      # every tensor excluded (an open case): the precondition is asserted on all of them
            worst = max(self.e32, key=self.e32.get)
        assert self.e32[worst] <= E32_MAX, "e32 of %s is %.3g > %.3g: another seed or input, not another cap" % (worst, self.e32[worst], E32_MAX)
        assert self.candidates <= MAX_CANDIDATES, "%d on-kink activations > %d" % (self.candidates, MAX_CANDIDATES)

    def rel_tol(self, name):
        return max(REL_TOL, E32_FACTOR * self.e32[name])


_CASES = {}          # the last KEEP_CASES cases: the tests of one (model, input) run next to each other
KEEP_CASES = 4


def case(arch, variables, x, y, iso, cam, **oracle_kw):
    """The memoised Case of a (model, input)."""
    h = hashlib.sha1(repr((arch, float(iso), float(cam), sorted(oracle_kw.items()))).encode())
    for k in sorted(variables):
        h.update(k.encode())
        h.update(np.ascontiguousarray(np.asarray(variables[k], np.float32)).tobytes())
    for a in (x, y):
        h.update(repr(np.asarray(a).shape).encode())
        h.update(np.ascontiguousarray(np.asarray(a, np.float32)).tobytes())
    key = h.hexdigest()
    c = _CASES.pop(key, None)
    if c is None:
        c = Case(arch, variables, x, y, iso, cam, **oracle_kw)
    _CASES[key] = c                                  # most recent last
    while len(_CASES) > KEEP_CASES:
        _CASES.pop(next(iter(_CASES)))
    return c


def bounds(c, ref_grads, abs_terms, name, old_tol, old_allowance, gmax=None, keep_old=False):
    """(per-entry bound of the rule, s_T) of tensor `name` against the evaluation `ref_grads` whose |term| sums are `abs_terms`."""
    gmax = c.gmax if gmax is None else gmax
    ref = np.asarray(ref_grads[name], np.float64)
    allow = GRAD_NOISE_C * 2.0 ** -24 * np.asarray(abs_terms[name], np.float64).reshape(ref.shape)
    s = max(np.abs(ref).max(), 1e-6 * gmax)
    old = np.maximum(old_tol * s, allow) if old_allowance else np.full(ref.shape, old_tol * s)
    new = old if keep_old else np.maximum(c.rel_tol(name) * s, allow)
    if not old_allowance:
        new = np.minimum(new, old)        # the comparison being replaced had no allowance: it gets it, capped by its old tolerance
    assert (new <= old).all(), (name, float(new.max()), float(old.max()))      # never weaker than what it replaces
    return new, s


def check_grads(c, got, ref_grads=None, abs_terms=None, names=None, old_tol=2e-4, old_allowance=True, exclude=()):
    """Every trainable tensor of `got` ({name: gradient}) against `ref_grads` (default: the case's fp64 evaluation; or one of its
    flipped evaluations, or a fixture of it) under the rule.  `exclude`: tensors that keep the old bound (a gradient that cancels,
    whose e32 is beyond the precondition; an open item; a case that is not admissible).  Raises AssertionError naming the tensors
    that miss; otherwise → (entries checked, {family: (worst |g - g64| / s_T, its tensor, e32 of that tensor)}), also left in ``c.report``."""
    if abs_terms is None:
        abs_terms = c.abs_terms if ref_grads is None else c.oracle.grad_abs_terms
    ref_grads = c.ref[2] if ref_grads is None else ref_grads
    names = [k for k in (c.names if names is None else names) if is_trainable(k)]
    gmax = max(np.abs(ref_grads[k]).max() for k in names)
    report, failures, checked = {}, [], 0
    for nm in names:
        ref = np.asarray(ref_grads[nm], np.float64)
        g = np.asarray(got[nm], np.float64).reshape(ref.shape)
        if is_zero_bias(nm):
            assert np.abs(ref).max() < 1e-9 * gmax, nm                      # analytically zero
            tol0 = np.full(ref.shape, 1e-5 * gmax)                          # ... and round-off of a sum whose terms cancel exactly
            # (the allowance also where the comparison being replaced had none: those tests get it)
            tol0 = np.maximum(tol0, GRAD_NOISE_C * 2.0 ** -24 * np.asarray(abs_terms[nm], np.float64).reshape(ref.shape))
            if not (np.abs(g) <= tol0).all():
                failures.append((nm, float(np.abs(g).max()), gmax))
        else:
            tol, s = bounds(c, ref_grads, abs_terms, nm, old_tol, old_allowance, gmax, nm in exclude)
            d = np.abs(g - ref)
            fam, rel = family(nm), float(d.max() / s)
            if fam not in report or rel > report[fam][0]:
                report[fam] = (rel, nm, c.e32[nm])
            if not (d <= tol).all():
                failures.append((nm, "worst |g - g64| / s_T %.3g" % rel, "worst |g - g64| / bound %.3g" % float((d / tol).max()),
                                 "e32 %.3g" % c.e32[nm], "s_T %.3g" % s))
        checked += ref.size
    assert not failures, failures[:4]
    c.report = report
    return checked, report


def worst_over_bound(c, got, old_tol=2e-4, old_allowance=True, exclude=()):
    """max over tensors and entries of |got - g64| / bound, against the case's own fp64 evaluation (the CPU tier's mutants)."""
    worst = 0.0
    for nm in (k for k in c.e32 if k not in exclude):
        tol, _ = bounds(c, c.ref[2], c.abs_terms, nm, old_tol, old_allowance)
        d = np.abs(np.asarray(got[nm], np.float64).reshape(tol.shape) - c.ref[2][nm])
        worst = max(worst, float((d / tol).max()))
    return worst


def format_report(report):
    return "  ".join("%s %.2e (e32 %.1e)" % (f, report[f][0], report[f][2]) for f in FAMILIES if f in report)


def hold_to_rule(c, got, loss=None, sd_z=None, old_tol=2e-4, old_allowance=True, names=None, label="", exclude=(), admissible=True):
    """The whole comparison of one evaluation (`got` = {name: gradient}; `loss`, `sd_z` optional, 1e-5 relative) with the case's
    oracle: preconditions from the reference alone, then the rule under the kink procedure with at most MAX_EXCUSED flips.
    Prints and returns ({family: (worst distance, tensor, e32)}, excused).
    `admissible=False`: a case kept for the kernel paths its size reaches although it cannot meet the preconditions (more than
    MAX_CANDIDATES activations on their kink at any input of that size).  That it cannot is asserted; every tensor keeps `old_tol`, and
    as before the rule a mismatch is not excused (the kink procedure refuses more than MAX_CANDIDATES candidates)."""
    if admissible:
        c.assert_admissible(exclude)
    else:
        assert c.candidates > MAX_CANDIDATES, "the case is admissible (%d candidates): hold it to the rule" % c.candidates
        exclude = tuple(c.e32)

    def compare(ref_loss, ref_sd, ref_grads):
        if loss is not None:
            assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
        if sd_z is not None:
            assert abs(sd_z - ref_sd) <= 1e-5 * ref_sd, (sd_z, ref_sd)
        check_grads(c, got, ref_grads, None, names, old_tol, old_allowance, exclude)      # oracle.grad_abs_terms: of the evaluation compared
    excused = grads_match_up_to_kinks(c.oracle, c.x, c.y, c.iso, c.cam, compare, max_kinks=MAX_CANDIDATES, got=got)
    assert excused <= MAX_EXCUSED, excused
    print("train_grad_rule %s: candidates %d, excused %d;  %s" % (label, c.candidates, excused, format_report(c.report)))
    return c.report, excused
