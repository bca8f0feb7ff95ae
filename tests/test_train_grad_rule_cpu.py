"""CPU tier: the rule the GPU tests hold the training step's gradients to (tests/train_grad_rule.py) has teeth, and every GPU case
is admissible under it — shown with this repository's oracle alone, nothing a kernel computes.  (But three cases that the GPU tests
keep at the tolerance they had, for the kernel paths only their size reaches: NOT_ADMISSIBLE.  For those it is shown that they are
not: more on-kink activations than the rule takes.)

For the (model, input) of every distinct GPU case of tests/test_gpu_train.py and tests/test_gpu_train_pr.py:
  (a) the preconditions hold: every pinned e32_T <= 2.5e-5, at most 64 activations on their ReLU kink;
  (b) a plain, unpinned float32 evaluation of the oracle's graph passes the rule under the kink procedure, <= 2 excused flips;
  (c) three subtly wrong evaluations (fp64, so nothing but the slip separates them from the reference) miss the rule on at least one
      tensor by more than twice the entry's bound, and the kink procedure cannot excuse them:
        nm1      the two batch means of the BN backward divided by N - 1 instead of N   (forward, loss, sd_z unchanged)
        drop1    one element left out of those two batch sums: a slot or a lane a reduction misses   (forward unchanged)
        unbiased the forward's batch variance divided by N - 1.
The mutants' own activations sit where the reference's do (nm1, drop1: identical forward), so the candidates are the same.
"""
import numpy as np
import pytest
import torch

import train_grad_rule as R
from conftest import FULL_ARCH
from oracle.nf_oracle import BN_EPS
import test_gpu_train as T
import test_gpu_train_pr as TP


class _BNWithSlippedBackward(torch.autograd.Function):
    """Forward: the oracle's training-mode BN, (h - mean) / sqrt(var + eps) over batch and pixels.  Backward: BN's, with one slip
    in the two batch means  mean(dy)  and  mean(dy * y)  it subtracts."""

    @staticmethod
    def forward(ctx, h, kind):
        m = h.mean(dim=(0, 2, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + BN_EPS)
        y = (h - m) * rstd
        ctx.save_for_backward(y, rstd)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        y, rstd = ctx.saved_tensors
        n = dy.shape[0] * dy.shape[2] * dy.shape[3]
        s1, s2 = dy.sum(dim=(0, 2, 3), keepdim=True), (dy * y).sum(dim=(0, 2, 3), keepdim=True)
        if ctx.kind == "nm1":
            m1, m2 = s1 / (n - 1), s2 / (n - 1)
        else:   # drop1: the first element of every channel is missing from both sums
            m1, m2 = (s1 - dy[:1, :, :1, :1]) / n, (s2 - (dy * y)[:1, :, :1, :1]) / n
        return (dy - m1 - y * m2) * rstd, None


def _unbiased(h, out):
    m = h.mean(dim=(0, 2, 3), keepdim=True)
    return (h - m) / torch.sqrt(h.var(dim=(0, 2, 3), unbiased=True, keepdim=True) + BN_EPS)


MUTANTS = {"nm1": lambda h, out: _BNWithSlippedBackward.apply(h, "nm1"),
           "drop1": lambda h, out: _BNWithSlippedBackward.apply(h, "drop1"),
           "unbiased": _unbiased}


def mutant_grads(c, kind):
    o = R.RuleOracle(c.arch, c.variables, bn=MUTANTS[kind], **c.kw)
    return o.loss_and_grads(c.x, c.y, c.iso, c.cam)


def _shipped():
    from conftest import SHIPPED_CKPT
    from noise_flow_amd.ckpt import load_checkpoint
    return load_checkpoint(SHIPPED_CKPT)


def _direct(arch, vseed, B, hw, xseed, b1=0.000479, set_gain=None, **kw):
    """The (model, input) of a test of tests/test_gpu_train.py that builds its case in its body."""
    from conftest import make_inputs, trained_like_variables
    v = trained_like_variables(arch, 4, seed=vseed)
    if set_gain is not None:
        v["model/sdn_gain/gain_val"] = np.asarray([set_gain], np.float32)
    x, y = make_inputs(B, hw[0], hw[1], seed=xseed, b1=b1)
    return T._case(arch, v, x, y, 800, 2, **kw)


def _golden_shipped():
    import os
    from conftest import GOLDEN_DIR
    g = np.load(os.path.join(GOLDEN_DIR, "train_step_shipped.npz"))
    return T._case(FULL_ARCH, _shipped(), g["x"], g["y"], float(g["iso"]), float(g["cam"]))


DIRECT = [("reversed-binding", lambda: _direct("sdn5|unc|unc|gain4|unc", 21, 5, (32, 32), 23, b1=0.003696, binding="sample_first"), 2e-4),
          ("shared-variables", lambda: _direct("sdn4|unc|gain4|sdn4|gain4", 12, 5, (16, 16), 9), 2e-4),
          ("gain-at-its-optimum", lambda: _direct("sdn5|gain4|unc", 2, 8, (32, 32), 5, set_gain=0.016486794), 2e-4),
          ("golden-shipped", _golden_shipped, 2e-4)]


# (id, builder, the tolerance the case's GPU comparison had before the rule).  Widths beyond 64: a representative of each route —
# 132 on 7x5 and 96 on 32x32 (also the forced bf16 x 6 cases), 200 (two channel tiles), 512; the fixture at width 48.
CASES = ([("other-%d" % i, (lambda p=p: T._other_case(*p)), 2e-4) for i, p in enumerate(T.OTHER_CASES)]
         + [("tiled-%d" % i, (lambda p=p: T._tiled_case(*p)), 2e-4) for i, p in enumerate(T.TILED_CASES)]
         + [("wide-%d" % i, (lambda p=p: T._wide_case(*p)), 1e-3) for i, p in enumerate(T.WIDE_CASES)]
         + [("beyond32-%d" % i, (lambda p=p: T._beyond_32_case(*p)), 1e-3) for i, p in enumerate(T.BEYOND_32_CASES)]
         + [("pr-%d" % i, (lambda p=p: TP._pr_case(p[2], p[3])), 1e-3) for i, p in enumerate(TP.PR_CASES)]
         + [("pr-fused", lambda: TP._pr_case(*TP.PR_FUSED_CASE), 1e-3),
            ("full-arch-shipped", lambda: T._full_arch_case(_shipped()), 2e-4),
            ("golden-width48", T._wide_golden_case, 2e-4)] + DIRECT)


# the cases of the GPU tests' NOT_ADMISSIBLE: 1100 patches of 8x8 at width 32, unc|unc at width 96 on 6 patches of 32x32, 8 patches of
# the patch-resident persistent loop
NOT_ADMISSIBLE = ({"wide-%d" % i for i, p in enumerate(T.WIDE_CASES) if p in T.NOT_ADMISSIBLE}
                  | {"beyond32-%d" % i for i, p in enumerate(T.BEYOND_32_CASES) if p[:4] in T.NOT_ADMISSIBLE}
                  | {"pr-%d" % i for i, p in enumerate(TP.PR_CASES) if (p[2], p[3]) == (8, 2)})
assert len(NOT_ADMISSIBLE) == 3


@pytest.mark.parametrize("cid,build,old_tol", CASES, ids=[c[0] for c in CASES])
def test_case_is_admissible_plain_fp32_passes_and_mutants_fail(cid, build, old_tol):
    c = build()
    if cid in NOT_ADMISSIBLE:
        # kept by the GPU tests at the tolerance they had, for the kernel paths only their size reaches; that no rule can be applied
        # is a fact of the reference: more on-kink activations than the kink procedure takes
        assert c.candidates > R.MAX_CANDIDATES, (cid, c.candidates)
        with pytest.raises(AssertionError):
            c.assert_admissible()
        print("%s: candidates %d: not admissible" % (cid, c.candidates))
        return
    # (the gain at its optimum: the gradients of the sdn / gain variables cancel, e32 of gain_val is 1; the GPU test keeps them
    # at its former tolerance and gain_val on the allowance alone)
    exclude = tuple(k for k in c.e32 if k.startswith("model/sdn_gain/")) if cid == "gain-at-its-optimum" else ()
    # (a) from the reference alone
    c.assert_admissible(exclude)
    worst = max((k for k in c.e32 if k not in exclude), key=c.e32.get)
    print("%s: candidates %d, worst e32 %.2e (%s)" % (cid, c.candidates, c.e32[worst], worst))
    # (b) a plain fp32 evaluation of the same graph
    loss32, sd32, g32, _ = c.plain32()
    report, excused = R.hold_to_rule(c, g32, old_tol=old_tol, label=cid + " plain fp32", exclude=exclude)
    assert abs(loss32 - c.ref[0]) <= 1e-5 * abs(c.ref[0])
    # (c) the mutants (a model without a coupling has no batch norm to get wrong)
    for kind in (MUTANTS if "unc" in c.arch else ()):
        loss, sd, g, _ = mutant_grads(c, kind)
        if kind != "unbiased":
            assert abs(loss - c.ref[0]) <= 1e-12 * abs(c.ref[0]) and abs(sd - c.ref[1]) <= 1e-12 * c.ref[1]     # backward only
        over = R.worst_over_bound(c, g, old_tol=old_tol, exclude=exclude)
        print("%s: mutant %s at %.1f times the bound" % (cid, kind, over))
        assert over > 2.0, (cid, kind, over)
        with pytest.raises(AssertionError):
            R.hold_to_rule(c, g, old_tol=old_tol, label=cid + " " + kind, exclude=exclude)


def test_the_gap_being_closed_at_the_patch_resident_case():
    """The nm1 mutant at the patch-resident case (width 32, 32x32, B = 5, seed 4) is inside the 1e-3 of each tensor's scale the suite
    applied on every matrix-core, patch-resident and GEMM path: a trainer whose BN backward normalises by N - 1 passed.  Under the
    rule it fails."""
    pr, grid, B, seed = TP.PR_CASES[0]
    c = TP._pr_case(B, seed)
    g = mutant_grads(c, "nm1")[2]
    worst_old = 0.0
    for nm in c.e32:
        s = max(np.abs(c.ref[2][nm]).max(), 1e-6 * c.gmax)
        worst_old = max(worst_old, float(np.abs(g[nm] - c.ref[2][nm]).max() / s))
    assert worst_old < 1e-3, worst_old                    # passed the old tolerance ...
    assert worst_old > 2e-4                               # ... and is no round-off: twice the largest relative bound of the rule
    with pytest.raises(AssertionError):
        R.check_grads(c, g, old_tol=1e-3)                # ... and fails the rule


@pytest.mark.parametrize("build,sfx", [(lambda: T._wide_case(*T.WIDE_CASES[2]), "l_1/W"), (lambda: T._wide_case(*T.WIDE_CASES[2]), "l_2/W"),
                                       (lambda: T._beyond_32_case(*T.BEYOND_32_CASES[9]), "l_1/W"),
                                       (lambda: T._beyond_32_case(*T.BEYOND_32_CASES[7]), "l_1/W")],
                         ids=["5x7-l_1", "5x7-l_2", "width200-l_1", "17-couplings-l_1"])
def test_one_pass_variance_moves_the_yardstick_at_the_open_cases(build, sfx):
    """Three of the open items of tests/train_grad_rule.py: models without an sdn layer in front, whose l_1 activations are a bias plus a
    small signal (mean^2 / variance up to 167).  The same float32 evaluation with the batch variance formed as E[h^2] - E[h]^2 — what
    the kernels do, over fp32 partial sums — is several times further from the fp64 one than with torch's two-pass variance, on
    exactly the tensors the kernels miss the rule on.  Evidence for the cause; no bound is made of it."""
    c = build()
    o = R.RuleOracle(c.arch, c.variables, dtype=torch.float32, gates=c.oracle.gates, one_pass_variance=True, **c.kw)
    g = o.loss_and_grads(c.x, c.y, c.iso, c.cam)[2]
    for nm in (k for k in c.e32 if k.endswith(sfx)):
        s = max(np.abs(c.ref[2][nm]).max(), 1e-6 * c.gmax)
        one_pass = float(np.abs(np.asarray(g[nm], np.float64) - c.ref[2][nm]).max() / s)
        print("%s: e32 %.2e two-pass, %.2e one-pass" % (nm, c.e32[nm], one_pass))
        assert one_pass > 3.0 * c.e32[nm], (nm, one_pass, c.e32[nm])
