"""Randomised sweep: architectures drawn from ``noise_flow_arch``'s whole vocabulary, every coupling width, ragged patch
shapes from 1x1 to 64x64 (and, tiled, up to 160x160), all settings of ``hps.flow_permutation`` / ``hps.decomp``, ISO in and outside the table — each
case through both directions of the HIP path (whichever kernel family the shape selects) against the fp64 oracle.

The hand-picked cases of the other files pin the geometry edges; this file looks for what nobody thought of.
Tolerance: per-patch NLL 1e-5 relative, tensors 1e-5 of their scale — or, where random weights make the stack
ill-conditioned, twice the distance of the oracle's own float32 flavour from its fp64 one (the kernel may not be
further from the truth than a plain fp32 evaluation of the reference's op sequence is)."""
import os

import numpy as np
import pytest

from conftest import make_inputs, trained_like_variables

pytestmark = pytest.mark.gpu

VOCAB = ["sdn5", "sdn4", "gain4", "sdn", "gain", "sdn1", "sdn2", "sdn3", "sdn6", "gain1", "gain2", "gain3"]
SETTINGS = [(1, "LU"), (1, "LU"), (1, "LU2"), (1, "NONE"), (0, "LU"), (2, "LU")]
ISO_TABLE = [100, 400, 800, 1600, 3200]


def _draw_case(seed):
    rng = np.random.RandomState(1000 + seed)
    width = int(rng.choice([4, 4, 4, 8, 16, 32]))
    if os.environ.get("NF_SWEEP_WIDTHS"):      # one-off sweeps over other widths (tools/oneoff_*.py): same draw otherwise
        width = int(np.random.RandomState(77 + seed).choice([int(w) for w in os.environ["NF_SWEEP_WIDTHS"].split(",")]))
    n = int(rng.randint(1, 6))
    arch, n_cond = [], 0
    for _ in range(n):
        lyr = "unc" if rng.rand() < 0.5 else str(rng.choice(VOCAB))
        if lyr != "unc":
            if n_cond == 4:        # the C ABI takes at most 4 conditional layers per model
                lyr = "unc"
            else:
                n_cond += 1
        arch.append(lyr)
    # one parameter set per family: two sdn-family (or gain-family) layers that read different variable sets may share an
    # arch, but two layers over the SAME variables must agree on their shapes (sdn5 [3,5] vs sdn6 [1,5] cam_params)
    if "sdn5" in arch and "sdn6" in arch:
        arch = [a if a != "sdn6" else "sdn5" for a in arch]
    if "gain" in arch and "gain1" in arch:       # ... or on their scale (gain: sigmoid(g), gain1: exp(1e-5 g))
        arch = [a if a != "gain1" else "gain" for a in arch]
    shape_kind = rng.randint(0, 4)
    if shape_kind == 0:
        H, W = int(rng.choice([32, 64])), int(rng.choice([32, 64]))
    elif shape_kind == 1:
        H, W = int(rng.randint(1, 12)), int(rng.randint(1, 12))
    else:
        H, W = int(rng.randint(1, 65)), int(rng.randint(1, 65))
    fp, decomp = SETTINGS[rng.randint(len(SETTINGS))]
    iso = int(rng.choice(ISO_TABLE + [250]))
    if "sdn1" in arch or "sdn2" in arch or "sdn3" in arch or "gain2" in arch:
        iso = int(rng.choice(ISO_TABLE))          # per-ISO tables scaled for their own ISO (see _condition)
    cam = int(rng.randint(0, 5))
    B = int(rng.choice([1, 2, 5]))
    return "|".join(arch), width, (H, W), fp, decomp, iso, cam, B


def _condition(v, arch, width, iso, rng):
    """Keep the random model's scales O(1) (as test_remaining_arch_vocabulary does) and the wide CNNs' activations tame."""
    kinds = set(arch.split("|"))
    for k in list(v):
        if "r_gain_param_" in k:
            v[k] = np.asarray([(-np.log(iso) + 0.3 * rng.randn()) / 1e-2], np.float32)
        elif "gain_param_" in k:
            if kinds & {"sdn2", "sdn3", "gain2"}:
                v[k] = np.asarray([(-np.log(max(iso, 100)) + 0.3 * rng.randn()) / 1e-1], np.float32)
            else:
                v[k] = np.asarray([0.3 * rng.randn() / 1e-5], np.float32)
        elif k in ("model/b1", "model/b2"):
            v[k] = np.asarray([rng.randn()], np.float32)
        elif k == "model/g1":
            v[k] = np.asarray([-np.log(iso) / 1e-5 if "gain1" in kinds else -np.log(iso)], np.float32)
        elif k == "model/g2":
            v[k] = np.asarray([-0.7 / 1e-5 if "gain1" in kinds else -0.7], np.float32)
        elif k == "model/sdn_gain/cam_params":
            v[k] = (1.0 + 0.2 * rng.randn(*v[k].shape)).astype(np.float32)
        elif k == "model/sdn_gain/gain_params":
            v[k] = (-np.log(np.asarray([100, 400, 800, 1600, 3200.0])) * 0.8 + 0.1 * rng.randn(5)).astype(np.float32)
        elif k in ("model/sdn_gain/beta1", "model/sdn_gain/beta2"):
            v[k] = np.asarray([-1.0 + 0.3 * rng.randn()], np.float32)
        elif width > 4 and (k.endswith("l_2/W") or k.endswith("l_last/W")):
            v[k] = (v[k] * np.float32((4.0 / width) ** 0.5)).astype(np.float32)
        elif "Conv2d_1x1" in k and not ("/P_" in k or "sign_S" in k) and ("A_matpar_none" in k or "_filters_" in k):
            v[k] = (np.asarray(v[k]) + 0.1 * rng.randn(*np.shape(v[k]))).astype(np.float32)
    return v


def _within(a, ref64, ref32, floor_rtol):
    scale = np.abs(ref64).max()
    tol = max(floor_rtol * scale, 2.0 * np.abs(ref32 - ref64).max())
    err = np.abs(np.asarray(a, np.float64) - ref64).max()
    assert err <= tol, "max err %.3e > tol %.3e (scale %.3e)" % (err, tol, scale)


@pytest.mark.parametrize("seed", list(range(150)))
def test_random_model_matches_oracle(seed):
    _check_case(seed, _draw_case(seed))


@pytest.mark.parametrize("seed", list(range(600, 616)))
def test_random_model_wide_couplings_match_oracle(seed):
    """The same sweep at coupling widths BEYOND 32 (sidd/ArgParser.py:43 defaults --width to 512): the LDS-staged GEMM kernel
    (csrc/nf_gemm.hip) — widths that are and are not one of its padded sizes, ragged patches of up to 2 048 pixels."""
    from noise_flow_amd import _lib
    arch, _, (H, W), fp, decomp, iso, cam, B = _draw_case(seed)
    rng = np.random.RandomState(seed)
    width = int(rng.choice([33, 48, 64, 96, 128, 200, 256, 320]))
    if "unc" not in arch.split("|"):
        arch = "unc|" + arch
    while H * W > 2048:
        H, W = max(1, H // 2), W
    m = _check_case(seed, (arch, width, (H, W), fp, decomp, iso, cam, min(B, 2)))
    assert m._flow.lib.nf_kernel_path(m._flow.ptr, 0) == _lib.NF_PATH_GEMM


@pytest.mark.parametrize("seed", list(range(900, 940)))
def test_random_model_on_the_split_bf16_kernel_and_the_exact_one(seed):
    """The sweep aimed at the default kernel of the headline shape: width 4 and 32x32 forced (the plain draw meets them together in
    about 3 % of its cases), batch from {1, 2, 5, 33}, everything else as drawn; at least one coupling.  Each case on the split-bf16
    kernel and on the exact-fp32 one, each against the oracle with _check_case's tolerances; and the two kernels' latents agree to
    max(1e-6 of scale, twice the distance of the oracle's fp32 flavour from fp64)."""
    from noise_flow_amd import _lib
    arch, _, _, fp, decomp, iso, cam, _ = _draw_case(seed)
    if "unc" not in arch.split("|"):
        arch = arch + "|unc"
    B = int(np.random.RandomState(seed).choice([1, 2, 5, 33]))
    case = (arch, 4, (32, 32), fp, decomp, iso, cam, B)
    got = {}
    for cnn_dtype, path in (("fp32", _lib.NF_PATH_SPLIT_BF16), ("fp32_exact", _lib.NF_PATH_MFMA4)):
        keep = {}
        m = _check_case(seed, case, cnn_dtype=cnn_dtype, keep=keep)
        for direction in (0, 1):
            assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == path, (case, cnn_dtype, direction)
        got[cnn_dtype] = keep
    a, b = got["fp32"], got["fp32_exact"]
    tol = max(1e-6 * np.abs(a["z64"]).max(), 2.0 * np.abs(a["z32"] - a["z64"]).max())
    d = np.abs(a["z"] - b["z"]).max()
    assert d <= tol, "%r: split vs exact latents %.3e > %.3e" % (case, d, tol)


def _large_shape(seed):
    rng = np.random.RandomState(5000 + seed)
    kind = rng.randint(0, 4)
    if kind == 0:
        return int(rng.randint(65, 161)), int(rng.randint(1, 65))
    if kind == 1:
        return int(rng.randint(1, 65)), int(rng.randint(65, 161))
    return int(rng.randint(65, 161)), int(rng.randint(65, 161))


@pytest.mark.parametrize("seed", list(range(800, 824)))
def test_random_model_large_patches(seed):
    """The same sweep on patches BEYOND 64x64 (overlapping tiles): whole vocabulary, widths 4 .. 32, every
    permutation / decomposition setting, one or both sides beyond 64, against the oracle on the whole image."""
    arch, width, _, fp, decomp, iso, cam, B = _draw_case(seed)
    _check_case(seed, (arch, width, _large_shape(seed), fp, decomp, iso, cam, min(B, 2)))


def _check_case(seed, case_tuple, cnn_dtype=None, keep=None):
    """``cnn_dtype``: the model's (None = the default kernels); ``keep``: a dict that receives the latents (kernel, fp64, fp32 oracle)."""
    from noise_flow_amd import NoiseFlow, default_hps, params
    from oracle.nf_oracle import NoiseFlowOracle
    arch, width, (H, W), fp, decomp, iso, cam, B = case_tuple
    rng = np.random.RandomState(seed)
    v = params.init_variables(arch, width, 4, seed, fp, decomp)
    base = trained_like_variables(arch, width, seed=seed)
    for k in v:
        if k in base:
            v[k] = base[k]
    v = _condition(v, arch, width, iso, rng)
    hps = default_hps(arch=arch, width=width, flow_permutation=fp, decomp=decomp)
    m = NoiseFlow([H, W, 4], False, hps, variables=v, cnn_dtype=cnn_dtype)
    o64 = NoiseFlowOracle(arch, v, flow_permutation=fp, decomp=decomp)
    o32 = NoiseFlowOracle(arch, v, dtype=np.float32, flow_permutation=fp, decomp=decomp)
    assert m.get_layer_names() == [L["name"] for L in o64.layers]
    x, y = make_inputs(B, H, W, seed=seed + 7)
    case = "arch=%s width=%d %dx%d fp=%d decomp=%s iso=%d cam=%d B=%d" % (arch, width, H, W, fp, decomp, iso, cam, B)
    yy, args = y, ([0.0], [0.0], [iso], [cam])
    try:
        nll, sd = m._loss(x, yy, *args)
        ref_nll, ref_sd, ref_z = o64.nll(x, yy, iso, cam)
        nll32, _, z32 = o32.nll(x, yy, iso, cam)
        tol = np.maximum(1e-5 * np.abs(ref_nll), 2.0 * np.abs(nll32 - ref_nll)) + 1e-4
        assert (np.abs(nll - ref_nll) <= tol).all(), np.abs(nll - ref_nll).max()
        z, obj = m.inverse(x, None, yy, *args)
        _within(z, ref_z, z32, 1e-5)
        if keep is not None:
            keep.update(z=np.asarray(z, np.float64), z64=ref_z, z32=z32)
        eps = np.random.RandomState(seed + 3).randn(B, H, W, 4).astype(np.float32)
        xs = m.sample(yy, 0.8, yy, *args, eps=eps)
        _within(xs, o64.sample(eps, 0.8, yy, iso, cam), o32.sample(eps, 0.8, yy, iso, cam), 1e-5)
        # the two directions invert each other
        back = m.forward(np.asarray(z, np.float32), None, yy, *args)
        back32 = o32.forward(z32, yy, iso, cam)       # how well a plain fp32 evaluation closes the loop on this model
        tol = max(5e-5 * np.abs(x).max(), 4.0 * np.abs(back32 - x).max())
        assert np.abs(np.asarray(back) - x).max() <= tol, "round trip %.3e > %.3e" % (np.abs(np.asarray(back) - x).max(), tol)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (case, e))
    return m


@pytest.mark.parametrize("seed", list(range(200, 240)))
def test_random_model_batch_statistics(seed):
    """The same draw in the reference's training-mode graph (``is_training=True``, layers.py:386-398): both activations of
    every coupling CNN normalised with the moments of the call's own patches.  B >= 2 so that the moments are not those
    of a single patch only; tolerances as tests/test_gpu_batchstats.py."""
    from noise_flow_amd import NoiseFlow, default_hps, params
    from oracle.nf_oracle import NoiseFlowOracle
    arch, width, (H, W), fp, decomp, iso, cam, B = _draw_case(seed)
    if "unc" not in arch.split("|"):
        arch = arch + "|unc"
    B = max(B, 2)
    if H * W * B < 16:              # the variance of a handful of values is too noisy a denominator for a parity check
        H, W = H + 4, W + 4
    # (patches beyond the scalar-weight kernel's LDS tiles at this width take the GEMM route of nf_*_batchstats, like the widths
    # beyond 32: no refusal left to test — tests/test_gpu_batchstats.py::test_batchstats_on_the_gemm_route; the sweep keeps the
    # oracle's fp64 convolutions small)
    H, W = min(H, 40), min(W, 40)
    rng = np.random.RandomState(seed)
    v = params.init_variables(arch, width, 4, seed, fp, decomp)
    base = trained_like_variables(arch, width, seed=seed)
    for k in v:
        if k in base:
            v[k] = base[k]
    v = _condition(v, arch, width, iso, rng)
    hps = default_hps(arch=arch, width=width, flow_permutation=fp, decomp=decomp)
    m = NoiseFlow([H, W, 4], True, hps, variables=v)
    o64 = NoiseFlowOracle(arch, v, flow_permutation=fp, decomp=decomp)
    o32 = NoiseFlowOracle(arch, v, dtype=np.float32, flow_permutation=fp, decomp=decomp)
    x, y = make_inputs(B, H, W, seed=seed + 7)
    case = "arch=%s width=%d %dx%d fp=%d decomp=%s iso=%d cam=%d B=%d" % (arch, width, H, W, fp, decomp, iso, cam, B)
    args = ([0.0], [0.0], [iso], [cam])
    try:
        nll, _ = m._loss(x, y, *args)
        ref_nll, _, ref_z = o64.nll(x, y, iso, cam, training=True)
        nll32, _, z32 = o32.nll(x, y, iso, cam, training=True)
        tol = np.maximum(5e-5 * np.abs(ref_nll), 2.0 * np.abs(nll32 - ref_nll)) + 1e-3
        assert (np.abs(nll - ref_nll) <= tol).all(), np.abs(nll - ref_nll).max()
        eps = np.random.RandomState(seed + 3).randn(B, H, W, 4).astype(np.float32)
        xs = m.sample(y, 0.8, y, *args, eps=eps)
        _within(xs, o64.sample(eps, 0.8, y, iso, cam, training=True), o32.sample(eps, 0.8, y, iso, cam, training=True), 2e-4)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (case, e))


@pytest.mark.parametrize("seed", list(range(300, 360)))
def test_random_model_training_gradients(seed):
    """One forward + backward of the trainer (C ABI ``nf_trainer_*``) on a random draw — the whole layer vocabulary, every
    ``flow_permutation`` / ``decomp`` setting — against the fp64 autograd oracle: loss, sd_z and every gradient tensor
    (tolerances of tests/test_gpu_train.py)."""
    from noise_flow_amd import default_hps, params
    from noise_flow_amd.train import Trainer
    from oracle.nf_grad_oracle import GradOracle, is_trainable
    from noise_flow_amd import params as P
    arch, width, (H, W), fp, decomp, iso, cam, B = _draw_case(5000 + seed)
    if "unc" not in arch.split("|"):
        arch = arch + "|unc"
    hw_max = int(os.environ.get("NF_SWEEP_MAXHW", "32"))    # one-off sweeps at large widths: fewer activations, fewer of them on a kink
    H, W = min(H, hw_max), min(W, hw_max)
    B = max(B, 2) + seed % 4
    if H * W * B < 32:
        H, W = H + 4, W + 4
    rng = np.random.RandomState(seed)
    v = params.init_variables(arch, width, 4, seed, fp, decomp)
    base = trained_like_variables(arch, width, seed=seed)
    for k in v:
        if k in base:
            v[k] = base[k]
    v = _condition(v, arch, width, iso, rng)
    x, y = make_inputs(B, H, W, seed=seed)
    case = "arch=%s width=%d %dx%d fp=%d decomp=%s iso=%d cam=%d B=%d" % (arch, width, H, W, fp, decomp, iso, cam, B)
    tr = Trainer([H, W, 4], default_hps(arch=arch, width=width, flow_permutation=fp, decomp=decomp), variables=v, optim="adam", max_batch=16)
    names = [nm for L in tr.layers for nm in P.layer_variable_names(L, tr._tmpl) if nm is not None]
    # 2e-4 of a tensor's scale at widths <= 8, 5e-4 beyond (longer fp32 sums).  Activations on a ReLU kink are handled exactly
    # below (grads_match_up_to_kinks), not by a loose tolerance.
    rtol = 2e-4 if width <= 8 else 5e-4
    # A draw whose coupling CNN sees a nearly constant input (a random sdn stack can shrink z by orders of magnitude) has batch
    # variances far below BN's epsilon: the normalised activations are then ~1e-2 small, float32 resolves them to ~1e-4 of
    # themselves and dozens of them sit on their ReLU kink — for ANY fp32 evaluation, the reference's included.  Such draws
    # keep the loss / sd_z check and get a coarse gradient check only.
    from oracle.nf_oracle import NoiseFlowOracle
    fo = NoiseFlowOracle(arch, v, flow_permutation=fp, decomp=decomp)
    fo.nll(x, y, iso, cam, training=True)
    min_var = min(float(np.min(m[k])) for m in fo.last_batch_moments.values() for k in ("var1", "var2") if k in m)
    if min_var < 1e-6:
        rtol = 5e-2

    grads, loss = tr.forward_backward(x, y, [0.0], [0.0], [iso], [cam])
    lv = loss.cpu().numpy()
    got = tr.raw_to_variables(grads.cpu().numpy())
    go = GradOracle(arch, v, flow_permutation=fp, decomp=decomp)
    from conftest import grad_noise_allowance
    sd_rtol = 1e-5 if min_var >= 1e-6 else 5e-5     # sd_z = sqrt(E z^2 - (E z)^2) of nearly constant latents cancels too

    def compare(ref_loss, ref_sd, ref_grads):
        assert abs(lv[0] - ref_loss) <= 1e-5 * abs(ref_loss) + 1e-4, "loss %r vs %r" % (lv[0], ref_loss)
        assert abs(lv[1] - ref_sd) <= sd_rtol * ref_sd, "sd_z"
        gmax = max(np.abs(ref_grads[nm]).max() for nm in names if is_trainable(nm))
        for nm in names:
            if not is_trainable(nm):
                continue
            ref = np.asarray(ref_grads[nm], np.float64)
            g = np.asarray(got[nm], np.float64).reshape(ref.shape)
            if nm.endswith("l_1/b") or nm.endswith("l_2/b"):      # analytically zero (BN subtracts the batch mean)
                tol0 = np.maximum(2e-5 * gmax, grad_noise_allowance(go, nm).reshape(ref.shape))
                assert (np.abs(g) <= tol0).all(), (nm, np.abs(g).max(), gmax)
            else:
                # rtol of the tensor's scale, or the round-off allowance of the sum the entry is — computed by the fp64 oracle
                # for the evaluation being compared (conftest.py::grad_noise_allowance), not by a second GPU run
                tol = np.maximum(rtol * max(np.abs(ref).max(), 1e-6 * gmax), grad_noise_allowance(go, nm).reshape(ref.shape))
                assert (np.abs(g - ref) <= tol).all(), (nm, np.abs(g - ref).max(), np.abs(ref).max(), float(np.max(tol)))

    # The loss is piecewise smooth: an activation within float32 round-off of a ReLU kink takes one branch in the fp64
    # oracle and possibly the other on the GPU, and the gradients upstream then differ by that one activation's path.  ONE
    # evaluation, no re-draws: the oracle reports exactly the activations whose margin is below 32 units of the round-off
    # of the sum that produced them, and only the other branch at (a subset of) those is accepted — conftest.py.
    from conftest import grads_match_up_to_kinks
    try:
        excused = grads_match_up_to_kinks(go, x, y, iso, cam, compare,
                                          max_kinks=int(os.environ.get("NF_SWEEP_MAXKINKS", "48")) if min_var >= 1e-6 else 0, got=got)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (case, e))
    assert excused <= 12, (case, excused)


@pytest.mark.parametrize("seed", list(range(400, 430)))
def test_random_model_fp16_cnn_mode(seed):
    """``cnn_dtype='fp16'`` (BASELINE configs[4]) on a random draw: width 4 on full 32x32 / 64x64 patches
    (v_mfma_f32_4x4x4_16b_f16), widths 8 / 16 / 32 on any shape (v_mfma_f32_32x32x16_f16) — against the oracle's
    emulation of the rounding points (NLL 1e-4 relative, tensors 2e-3 of scale, as tests/test_gpu_wide.py) and no further
    from the fp32 model than the quantisation noise of an independent fp16 evaluation explains."""
    from noise_flow_amd import NoiseFlow, default_hps, params
    from oracle.nf_oracle import NoiseFlowOracle
    arch, width, (H, W), fp, decomp, iso, cam, B = _draw_case(seed)
    if "unc" not in arch.split("|"):
        arch = "unc|" + arch
    if width == 4:
        H = W = 32 if seed % 2 else 64
    rng = np.random.RandomState(seed)
    v = params.init_variables(arch, width, 4, seed, fp, decomp)
    base = trained_like_variables(arch, width, seed=seed)
    for k in v:
        if k in base:
            v[k] = base[k]
    v = _condition(v, arch, width, iso, rng)
    hps = default_hps(arch=arch, width=width, flow_permutation=fp, decomp=decomp)
    m = NoiseFlow([H, W, 4], False, hps, variables=v, cnn_dtype="fp16")
    o16 = NoiseFlowOracle(arch, v, cnn_dtype="fp16", flow_permutation=fp, decomp=decomp)
    o32 = NoiseFlowOracle(arch, v, flow_permutation=fp, decomp=decomp)
    oplain = NoiseFlowOracle(arch, v, cnn_dtype="fp16_plain", flow_permutation=fp, decomp=decomp)
    x, y = make_inputs(B, H, W, seed=seed + 7)
    case = "arch=%s width=%d %dx%d fp=%d decomp=%s iso=%d cam=%d B=%d" % (arch, width, H, W, fp, decomp, iso, cam, B)
    args = ([0.0], [0.0], [iso], [cam])
    try:
        nll, _ = m._loss(x, y, *args)
        ref, _, rz = o16.nll(x, y, iso, cam)
        n32, _, z32 = o32.nll(x, y, iso, cam)
        npl, _, zpl = oplain.nll(x, y, iso, cam)
        noise = np.abs(npl - n32).max()
        assert (np.abs(nll - ref) <= 1e-4 * np.abs(ref) + 0.05 * noise + 1e-3).all(), "nll vs emulation %.3e (noise %.3e)" % (np.abs(nll - ref).max(), noise)
        # two fp16 evaluations are two draws of the same quantisation noise (a handful of patches each): the library's
        # distance from the fp32 model is held to a multiple of the independent evaluation's, or 2e-4 relative (test_gpu_wide)
        assert np.abs(nll - n32).max() <= max(6.0 * noise, 2e-4 * np.abs(n32).max()) + 1e-3, \
            "nll vs fp32 %.3e, fp16 noise %.3e, |nll| %.3e" % (np.abs(nll - n32).max(), noise, np.abs(n32).max())
        z, _ = m.inverse(x, None, y, *args)
        zs = np.abs(rz).max()
        assert np.abs(np.asarray(z, np.float64) - rz).max() <= 2e-3 * zs, "z vs emulation"
        eps = np.random.RandomState(seed + 3).randn(B, H, W, 4).astype(np.float32)
        xs = m.sample(y, 0.8, y, *args, eps=eps)
        rx = o16.sample(eps, 0.8, y, iso, cam)
        assert np.abs(np.asarray(xs, np.float64) - rx).max() <= 2e-3 * np.abs(rx).max(), "sample vs emulation"
    except AssertionError as e:
        raise AssertionError("%s: %s" % (case, e))
