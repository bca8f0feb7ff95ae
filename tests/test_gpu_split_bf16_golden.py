"""The split-bf16 flow kernel (width 4, 32x32 patches: the default kernel) gives bit for bit what it gave before its operand split
was rewritten to convert each piece once.

tests/golden/split_bf16_bits.npz was recorded with tools/make_golden_split_bf16.py on an MI355X from the build of commit 1414324,
the last one whose split rounded every piece twice (a packed v_cvt_pk_bf16_f32 for the stored word and a single-value one for the
remainder).  The rewrite changes instruction counts only: the three pieces of a value are the same round-to-nearest-even bf16s,
each the rounded remainder of the one before, so every output is the same fp32.  A differing bit means a piece changed: that is a
bug in the split, not a tolerance question, hence array_equal.

Both directions of the kernel: the per-patch NLL of the first 64 synthetic patches (forward), the images sampled for 4 clean
patches from the in-kernel Philox draw of one seed and draw offset (reverse, nf_flow_split_kernel<true>) and from a supplied
epsilon (reverse, nf_flow_split_kernel<false>)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_bf16_bits.npz")
N_NLL, N_SAMPLE = 64, 4
SEED, DRAW_OFFSET = 20240611, 4096
COND = dict(nlf0=[0.000479], nlf1=[0.000002], iso=[100.0], cam=[2.0])   # ISO 100, S6: the benchmark's condition


def compute_outputs():
    """What the fixture holds, from the library that is loaded (float32 arrays)."""
    import torch
    from noise_flow_amd import NoiseFlow, default_hps
    from noise_flow_amd.ckpt import load_checkpoint
    from noise_flow_amd.patches import synth_patches

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variables = load_checkpoint(os.path.join(root, "models", "NoiseFlow", "ckpt", "model.ckpt.best"))
    model = NoiseFlow([32, 32, 4], False, default_hps(), variables=variables, device=0)
    assert model.cnn_dtype == "fp32"   # the split-bf16 kernel, not "fp32_exact"
    x, y = synth_patches(0, 0, N_NLL, device=0)
    nll, _ = model._loss(x, y, COND["nlf0"], COND["nlf1"], COND["iso"], COND["cam"])
    ys = y[:N_SAMPLE].contiguous()
    model._draws = DRAW_OFFSET
    drawn = model.sample(ys, yy=ys, seed=SEED, **COND)
    eps = torch.from_numpy(np.random.RandomState(SEED).randn(N_SAMPLE, 32, 32, 4).astype(np.float32)).to(ys.device)
    fed = model.forward(eps, yy=ys, **COND)
    to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return {"nll": to_np(nll).astype(np.float32), "sample_philox": to_np(drawn), "sample_eps": to_np(fed)}


@pytest.fixture(scope="module")
def outputs():
    return compute_outputs()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["nll", "sample_philox", "sample_eps"])
def test_split_kernel_bits_are_those_of_the_double_rounding_split(outputs, key):
    want = np.load(GOLDEN)[key]
    got = outputs[key]
    assert got.dtype == want.dtype and got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    print("%s: %d of %d values differ in some bit" % (key, int(diff.sum()), diff.size))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
