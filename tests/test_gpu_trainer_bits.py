"""The trainer's host orchestration (csrc/nf_train.hip: which kernel family runs a coupling, which launches are fused with their
neighbours, which work goes to the side stream) decides launches, operands and event order — never arithmetic.  The kernels add
slotted partial sums in a fixed order and use no atomics, so a step gives the same bits on every run, and a rewrite of the host code
that keeps every launch, grid and operand must give the bits of the code before it: tests/golden/trainer_host_bits.npz was recorded
with tools/make_golden_trainer_bits.py on an MI355X (the grids depend on the CU count) from the build of commit 336408c, the last
one before the host code was reorganised around train_path() / the step plan / the coupling context.  array_equal on the uint32
views; no tolerance — a differing bit is a launch, a grid or an operand that changed, not a rounding question.  The vocab-* cases
were added to the fixture from the build of commit 5e09953 (make_golden_trainer_bits.py --only vocab- --into), the last one in
which the trainer wrote the layer kinds' formulas out separately from the evaluator: they pin k_prep / k_finish on every sdn and
gain kind and every 1x1 setting across the move to the shared csrc/nf_layers.h.

CASES are the smallest shapes that reach each branch of the host code (the comment behind each says which).  Every case makes
`steps` calls of forward_backward + apply on one handle (three where the pending side-stream events have to cross a step
boundary) and keeps: the raw gradient of the last call; the raw parameters at the end (Adam moves all of them, the BN running
moments move by their EMA); and (loss, sd_z) of every call on patches of a multiple of 64 pixels, where k_prior leaves
per-wavefront partials that k_loss adds in a fixed order — on other shapes k_prior adds with float atomics in arrival order and two
runs of ONE build differ in the last bit of the reported loss (nothing else reads it), so it is not recorded there.  The
evaluator cases keep per-patch NLL, the latent, a sample and the running moments the calls leave (the batch-mean sd_z is added
by device atomics and is not recorded).

What the fixture holds (it has to stay under 512 KiB): vectors of up to FULL_MAX values in full; of longer ones, per layer
block, the first and last 64 values, the sum of the uint32 bit patterns and the sum of the patterns times their 1-based position
(both mod 2^64: a changed bit anywhere changes the first, two changes that cancel there do not cancel in the second).  The raw
gradient is kept in full for models of up to FULL_MAX = 4 Ki parameters — with a threshold of 16 Ki the 26 width-32 cases alone
would hold 0.9 MB of incompressible floats."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_host_bits.npz")
FULL_MAX = 4096
SWITCHES = ("NF_TRAIN_TILED", "NF_TRAIN_WIDE_MFMA", "NF_TRAIN_SERIAL", "NF_TRAIN_PR", "NF_TRAIN_PR_GRID", "NF_TRAIN_GEMM_C1",
            "NF_TRAIN_BAND", "NF_TRAIN_NB_FLOOR", "NF_TRAIN_PR_SIDE_FULL", "NF_TRAIN_PR_BOTH_MAX", "NF_BS_WIDE")
CHILD_SWITCH = "NF_TRAIN_GEMM"      # read once per process: a case that sets it runs in a child

U3, FOLD, G3 = "unc|unc|unc", "sdn5|unc|unc|gain4|unc", "unc|gain4|unc"
G8 = {"NF_TRAIN_PR_GRID": "8"}      # 8 "CUs": 1 patch = no side stream, 3 = both products, 5 = d l_last/W only, 20 = persistent loop


def _c(cid, arch, width, hw, B, env=None, steps=1, mode="train", fp=1, decomp="LU", iso=400, cam=1, vocab=False):
    return dict(id=cid, arch=arch, width=width, hw=hw, B=B, env=dict(env or {}), steps=steps, mode=mode,
                fp=fp, decomp=decomp, iso=iso, cam=cam, vocab=vocab)


def _v(kind, fp, decomp, iso, cam):
    """One layer of the vocabulary beyond the default kinds with a coupling behind it (and the 1x1 layer of the given
    flow_permutation / decomp setting in between): width 4, 8x8 patches (64 pixels: (loss, sd_z) is kept), B = 3, one step."""
    return _c("vocab-%s-fp%d-%s-iso%d" % (kind, fp, decomp, iso), kind + "|unc", 4, (8, 8), 3, fp=fp, decomp=decomp, iso=iso, cam=cam, vocab=True)


CASES = [
    # ---- tiled family (widths 4 / 8)
    _c("tiled-u3-w4-10x12", U3, 4, (10, 12), 11),                                   # NT 256, chained without a Conv2d1x1
    _c("tiled-fold-w8-16x24", FOLD, 8, (16, 24), 6),                                # NT 512, the fold, a chain cut by another layer
    _c("tiled-full-w4-32x32", FULL_ARCH, 4, (32, 32), 9),                           # NT 1024, the shipped architecture
    _c("tiled-u3-w4-10x12-T0", U3, 4, (10, 12), 11, {"NF_TRAIN_TILED": "0"}),
    _c("tiled-u3-w4-10x12-T1", U3, 4, (10, 12), 11, {"NF_TRAIN_TILED": "1"}),
    _c("tiled-u3-w4-10x12-T2", U3, 4, (10, 12), 11, {"NF_TRAIN_TILED": "2"}),
    _c("tiled-exit-w4-8x8-B400", "unc|unc", 4, (8, 8), 400),                        # npatch > 384: the layer kernels
    # ---- layer kernels and the wide matrix-core stages (widths 16 / 32)
    _c("wide-w16-16x24", FOLD, 16, (16, 24), 6),
    _c("wide-w32-20x12", FOLD, 32, (20, 12), 7),
    _c("wide-w32-5x7", "unc|unc", 32, (5, 7), 3),
    _c("wide-w32-64x64", "unc|unc", 32, (64, 64), 2),                               # the operand tile does not fit
    _c("wide-w32-20x12-M0", FOLD, 32, (20, 12), 7, {"NF_TRAIN_WIDE_MFMA": "0"}),
    _c("wide-w32-20x12-M127", FOLD, 32, (20, 12), 7, {"NF_TRAIN_WIDE_MFMA": "127"}),
    _c("wide-w32-20x12-M511", FOLD, 32, (20, 12), 7, {"NF_TRAIN_WIDE_MFMA": "511"}),
    _c("wide-w32-8x8-B1100", "unc|unc", 32, (8, 8), 1100),                          # more patches than slots
    _c("wide-w32-20x12-serial", FOLD, 32, (20, 12), 7, {"NF_TRAIN_SERIAL": "1"}),
    # ---- patch-resident family (width 32 on 32x32)
    _c("pr-u3-B1", U3, 32, (32, 32), 1, G8), _c("pr-fold-B1", FOLD, 32, (32, 32), 1, G8),
    _c("pr-u3-B3", U3, 32, (32, 32), 3, G8), _c("pr-fold-B3", FOLD, 32, (32, 32), 3, G8),
    _c("pr-u3-B5", U3, 32, (32, 32), 5, G8), _c("pr-fold-B5", FOLD, 32, (32, 32), 5, G8),
    _c("pr-u3-B20", U3, 32, (32, 32), 20, G8), _c("pr-fold-B20", FOLD, 32, (32, 32), 20, G8),
    _c("pr-fold-B3-P1", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="1")),
    _c("pr-fold-B3-P2", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="2")),
    _c("pr-fold-B3-P5", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="5")),
    _c("pr-fold-B3-P9", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="9")),
    _c("pr-fold-B3-P17", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="17")),
    _c("pr-fold-B3-P33", FOLD, 32, (32, 32), 3, dict(G8, NF_TRAIN_PR="33")),
    _c("pr-fold-B3-nogrid", FOLD, 32, (32, 32), 3),
    # ---- GEMM path
    _c("gemm-w5", G3, 5, (8, 8), 4), _c("gemm-w24", G3, 24, (8, 8), 4), _c("gemm-w96", G3, 96, (8, 8), 4),
    _c("gemm-w160", G3, 160, (8, 8), 4), _c("gemm-w256", G3, 256, (8, 8), 4),       # 256: the dual product
    _c("gemm-w24-c1", G3, 24, (8, 8), 4, {"NF_TRAIN_GEMM_C1": "1"}),
    _c("gemm-w8-forced", G3, 8, (8, 8), 4, {CHILD_SWITCH: "1"}),
    # ---- entry points
    _c("steps3-tiled", U3, 4, (10, 12), 11, steps=3), _c("steps3-wide", FOLD, 32, (20, 12), 7, steps=3),
    _c("steps3-pr", FOLD, 32, (32, 32), 3, G8, steps=3), _c("steps3-gemm", G3, 24, (8, 8), 4, steps=3),
    _c("forward-only", FOLD, 8, (16, 24), 6, mode="forward"),
    _c("ends-in-gain", "unc|unc|gain4", 4, (10, 12), 5),                            # a stack ending in a non-coupling layer: k_dz_init
    _c("bs-pr-u3", U3, 32, (32, 32), 3, mode="bs"),                                 # the patch-resident evaluator, no Conv2d1x1 in front
    _c("bs-pr-fold", FOLD, 32, (32, 32), 3, mode="bs"),                             # ... with one
    _c("bs-gemm-w24", G3, 24, (16, 16), 4, {"NF_BS_WIDE": "1"}, mode="bs"),         # the GEMM evaluator
    # ---- the layer vocabulary beyond sdn5 / sdn4 / gain4 / PLU (recorded from commit 5e09953, the last one with the layer kinds
    #      written out separately in the trainer): every other sdn / gain kind, the LU2 / NONE / permutation 1x1 settings spread
    #      over them, two cases at an ISO outside the table (sdn6: the gain exponent is 0; gain3: the ISO-800 entry)
    _v("sdn", 1, "LU2", 400, 0), _v("sdn1", 1, "NONE", 800, 1), _v("sdn2", 0, "LU", 1600, 2), _v("sdn3", 2, "LU", 100, 3),
    _v("sdn6", 1, "LU2", 250, 4), _v("gain", 1, "NONE", 3200, 0), _v("gain1", 0, "LU", 400, 1), _v("gain2", 1, "LU2", 800, 2),
    _v("gain3", 1, "NONE", 250, 3), _v("sdn6", 1, "LU", 1600, 2), _v("gain3", 2, "LU", 100, 4),
]
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def _seed(case):
    return 7 * case["width"] + case["hw"][0] + 3 * case["hw"][1] + len(case["arch"])


def _variables(case):
    if case.get("vocab"):      # (test_gpu_batchstats_bits.py passes case records of its own) the random sweep's recipe: variables of the 1x1 setting, trained-like CNNs, conditional scales of O(1)
        from noise_flow_amd import params
        from test_gpu_random_sweep import _condition
        v = params.init_variables(case["arch"], case["width"], 4, _seed(case), case["fp"], case["decomp"])
        v.update({k: a for k, a in trained_like_variables(case["arch"], case["width"], seed=_seed(case)).items() if k in v})
        return _condition(v, case["arch"], case["width"], case["iso"], np.random.RandomState(_seed(case)))
    v = trained_like_variables(case["arch"], case["width"], seed=_seed(case))
    scale = np.float32((4.0 / case["width"]) ** 0.5)      # activations of O(1) at every width (the helper is tuned for width 4)
    for k in v:
        if k.endswith("l_2/W") or k.endswith("l_last/W"):
            v[k] = (v[k] * scale).astype(np.float32)
    return v


class _env:
    """The case's switches while its trainer / model is created and run (most are read at create, NF_BS_WIDE per call)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.env.items() if k != CHILD_SWITCH})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _blocks(layers, width):
    from noise_flow_amd import _lib
    lib, pos, out = _lib.load(), 0, []
    for L in layers:
        n = int(lib.nf_layer_param_count(L.nf_type, int(getattr(L, "width", 0) or width)))
        out.append((pos, pos + n))
        pos += n
    return out


def _keep(res, name, a, blocks=None):
    """A vector in full, or — beyond FULL_MAX values — per block its ends and two sums of its bit patterns."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if a.size <= FULL_MAX:
        res[name] = a
        return
    ends, sums = [], []
    for lo, hi in (blocks or [(0, a.size)]):
        blk = a[lo:hi]
        bits = blk.view(np.uint32).astype(np.uint64)
        ends.append(blk if blk.size <= 128 else np.concatenate([blk[:64], blk[-64:]]))
        sums.append((bits.sum(dtype=np.uint64), (bits * np.arange(1, bits.size + 1, dtype=np.uint64)).sum(dtype=np.uint64)))
    res[name + "_ends"] = np.concatenate(ends)
    res[name + "_sums"] = np.asarray(sums, np.uint64).reshape(-1)


def _train_case(case, res):
    from noise_flow_amd import default_hps
    from noise_flow_amd.train import Trainer
    H, W = case["hw"]
    iso, cam = [case["iso"]], [case["cam"]]
    x, y = make_inputs(case["B"], H, W, seed=_seed(case) + 20)
    hps = default_hps(arch=case["arch"], width=case["width"], flow_permutation=case["fp"], decomp=case["decomp"])
    tr = Trainer([H, W, 4], hps, variables=_variables(case), optim="adam", max_batch=case["B"])
    blocks = _blocks(tr.layers, case["width"])
    losses = []
    if case["mode"] == "forward":
        losses.append(np.asarray(tr.forward(x, y, [0.0], [0.0], iso, cam), np.float32))
    for _ in range(case["steps"] if case["mode"] == "train" else 0):
        g, loss = tr.forward_backward(x, y, [0.0], [0.0], iso, cam)
        losses.append(loss.cpu().numpy().copy())
        grad = g.cpu().numpy().copy()
        tr.apply(1e-3)
    if (H * W) % 64 == 0:      # (other shapes: k_prior adds the per-patch sums of the latent with float atomics, in arrival order)
        res["loss"] = np.concatenate(losses)
    if case["mode"] == "train":
        _keep(res, "grad", grad, blocks)
    _keep(res, "params", tr.raw_params(), blocks)
    tr.close()


def _bs_case(case, res):
    from test_gpu_batchstats import _model
    H, W = case["hw"]
    B = case["B"]
    x, y = make_inputs(B, H, W, seed=_seed(case) + 20)
    v = _variables(case)
    m = _model(case["arch"], v, (H, W, 4), case["width"])
    nll, _ = m._loss(x, y, [0.0], [0.0], [400], [1])
    z, _ = m.inverse(x, None, y, [0.0], [0.0], [400], [1])
    eps = np.random.RandomState(_seed(case)).randn(B, H, W, 4).astype(np.float32)
    xs = m.sample(y, 0.6, y, [0.0], [0.0], [400], [1], eps=eps)
    res["nll"] = np.asarray(nll, np.float32).reshape(-1)
    _keep(res, "z", z, [(i * H * W * 4, (i + 1) * H * W * 4) for i in range(B)])
    _keep(res, "sample", xs, [(i * H * W * 4, (i + 1) * H * W * 4) for i in range(B)])
    mv = m.variables      # the running moments after two NLL-direction calls and one sampling call
    res["moments"] = np.concatenate([np.asarray(mv[k], np.float32).reshape(-1) for k in sorted(mv) if "bn_nvp_conv" in k])


def case_outputs(case):
    """What the fixture holds of one case, from the library that is loaded: {"<case id>__<name>": array}."""
    if case["env"].get(CHILD_SWITCH) and os.environ.get(CHILD_SWITCH) != case["env"][CHILD_SWITCH]:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "case.npz")
            env = dict(os.environ)
            env[CHILD_SWITCH] = case["env"][CHILD_SWITCH]
            subprocess.run([sys.executable, os.path.abspath(__file__), case["id"], out], check=True, env=env, timeout=300)
            with np.load(out) as f:
                return {k: f[k] for k in f.files}
    res = {}
    with _env(case["env"]):
        (_bs_case if case["mode"] == "bs" else _train_case)(case, res)
    for name, a in res.items():
        assert a.dtype in (np.float32, np.uint64) and (a.dtype == np.uint64 or np.isfinite(a).all()), (case["id"], name)
    return {"%s__%s" % (case["id"], name): a for name, a in res.items()}


def differing(got, want):
    """Keys whose arrays differ in dtype, shape or any bit."""
    bad = []
    for key in sorted(set(got) | set(want)):
        if key not in got or key not in want:
            bad.append(key)
            continue
        g, w = got[key], want[key]
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append(key)
            continue
        view = np.uint32 if g.dtype == np.float32 else np.uint64
        diff = g.view(view) != w.view(view)
        print("%s: %d of %d values differ in some bit" % (key, int(diff.sum()), diff.size))
        if diff.any():
            bad.append(key)
    return bad


def test_the_cases_cover_the_regimes_they_name():
    """No GPU: the facts the case table relies on, restated from csrc/nf_train.hip."""
    ids = set(CASE_IDS)
    for c in CASES:
        H, W = c["hw"]
        if c["id"].startswith("tiled-") and "exit" not in c["id"]:
            assert c["width"] in (4, 8) and H * W <= 1024 and c["B"] <= 384
        if c["id"].startswith("pr-") and c["env"].get("NF_TRAIN_PR_GRID") == "8":
            n, cus = c["B"], 8
            split = 4 * n <= 3 * cus and 4 * n >= cus           # pr_split()
            both = 2 * n <= cus                                  # both_ok
            assert (split, split and both, n > cus) == {1: (False, False, False), 3: (True, True, False),
                                                        5: (True, False, False), 20: (False, False, True)}[n]
        if c["id"].startswith("gemm-w") and "forced" not in c["id"]:
            assert c["width"] not in (4, 8, 16, 32)
    assert [c["hw"] for c in CASES[:3]] == [(10, 12), (16, 24), (32, 32)]      # NT 256 / 512 / 1024
    assert ((64 + 2) * (64 + 2) * 4 + 64 * 64) * 4 > 60 * 1024                  # wide-w32-64x64: gu_tile does not fit
    assert 1100 > 1024 and 400 > 384
    assert {"steps3-tiled", "steps3-wide", "steps3-pr", "steps3-gemm", "forward-only", "ends-in-gain"} <= ids


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_trainer_gives_the_bits_of_the_host_code_before_the_reorganisation(case):
    prefix = case["id"] + "__"
    with np.load(GOLDEN) as f:
        want = {k: f[k] for k in f.files if k.startswith(prefix)}
    assert want, "no golden arrays for %s" % case["id"]
    bad = differing(case_outputs(case), want)
    assert not bad, bad


if __name__ == "__main__":      # the child of a case that needs NF_TRAIN_GEMM: python test_gpu_trainer_bits.py <case id> <out.npz>
    np.savez(sys.argv[2], **case_outputs(CASES[CASE_IDS.index(sys.argv[1])]))
