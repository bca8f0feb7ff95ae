"""The split-bf16 flow kernel walks a counted run of (mix, coupling) pairs whose A images it addresses by a scalar offset that
advances by a constant stride, and reads the LDS operands of a unit while the unit before it multiplies.  Neither changes a
product, their order or a rounding, so every output is bit for bit what the kernel gave when it read each coupling's offset from
its parameter block: tests/golden/split_bf16_runs.npz was recorded with tools/make_golden_split_bf16_runs.py on an MI355X from the
build of commit 659fab9, the last one that did.  array_equal on the uint32 views; a differing bit is a wrong address or a read
that overtook a write, not a tolerance question.

What tests/golden/split_bf16_bits.npz (64 and 4 patches of the shipped model) does not reach:

* B = 1 (one workgroup) and B = B_BIG = the resident capacity of an MI355X + 1 (256 CUs x 4 workgroups + 1): workgroup 0 takes a
  second patch and the offset of the run must start again.  Of the large batch the fixture keeps the NLL of the first, a middle and
  the last patch and the sampled images of the first and the last;
* models with 1, 2 and 17 `unc` layers (17: the deepest that gets the layout), seeded, from the builders of
  tests/test_split_bf16.py;
* a model whose first coupling has no mix in front while the later ones do (the run starts at the second coupling, so its first
  offset is not the first image's), and one without any mix (flow_permutation 2: no run, every coupling reads its offset field);
  in the sampling direction every model's program starts with a coupling, the run behind it;
* the three entry points: NLL, sampling from a supplied epsilon, sampling from the in-kernel Philox draw (B = 2).
"""
import os

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs
from test_split_bf16 import DEEPEST_SPLIT, deep_variables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_bf16_runs.npz")
B_BIG = 1025                       # MI355X: 256 CUs x 4 resident workgroups + 1
KEEP = (0, B_BIG // 2, B_BIG - 1)  # patches of the large batch whose NLL the fixture keeps
SEED, DRAW_OFFSET = 20250309, 8192
MODELS = ("shipped", "unc1", "unc2", "unc17", "first_without_mix", "no_mix")
KINDS = ("nll_one", "nll_big", "sample_eps", "sample_philox")


def _build(name):
    """(model, x, y or None, conditioning) of one case."""
    from noise_flow_amd import NoiseFlow, default_hps, params
    from noise_flow_amd.ckpt import load_checkpoint
    from noise_flow_amd.noise_flow_model import FlowHandle
    if name == "shipped":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        v = load_checkpoint(os.path.join(root, "models", "NoiseFlow", "ckpt", "model.ckpt.best"))
        m = NoiseFlow([32, 32, 4], False, default_hps(arch=FULL_ARCH), variables=v, device=0)
        x, y = make_inputs(B_BIG, seed=41)
        return m, x, y, dict(nlf0=[0.000479], nlf1=[0.000002], iso=[100.0], cam=[2.0])
    n = {"unc1": 1, "unc2": 2, "unc17": DEEPEST_SPLIT}.get(name, 3)
    arch = "|".join(["unc"] * n)
    v = deep_variables(n, seed=40 + n, damp=0.5 if n > 2 else 1.0)
    perm = 2 if name == "no_mix" else 1
    m = NoiseFlow([32, 32, 4], False, default_hps(arch=arch, width=4, flow_permutation=perm), variables=v, device=0)
    if name == "first_without_mix":
        layers = m._flow.layers
        assert layers[0].kind == "conv1x1" and layers[1].kind == "coupling"
        tmpl = params.template_binding(layers, "loss_first")
        old = m._flow
        m._flow = FlowHandle(arch, v, [32, 32, 4], 4, device=0, layers=layers[1:], tmpl=tmpl)
        old.close()
    x, _ = make_inputs(B_BIG, seed=40 + n, b1=1.0, b2=0.25)
    return m, x, None, dict(nlf0=[0.0], nlf1=[0.0], iso=[100.0], cam=[0.0])


def compute_outputs():
    """What the fixture holds, from the library that is loaded: {"<model>__<kind>": float32 array}."""
    import torch
    from noise_flow_amd import _lib
    assert torch.cuda.get_device_properties(0).multi_processor_count * 4 + 1 == B_BIG, "B_BIG is the resident capacity of an MI355X + 1"
    out = {}
    for name in MODELS:
        m, x, y, cond = _build(name)
        for direction in (0, 1):
            assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == _lib.NF_PATH_SPLIT_BF16, (name, direction)
        xt = torch.from_numpy(x).cuda()
        yt = torch.from_numpy(y).cuda() if y is not None else None
        eps = torch.from_numpy(np.random.RandomState(SEED).randn(*x.shape).astype(np.float32)).cuda()
        one = m._loss(xt[:1].contiguous(), yt[:1].contiguous() if yt is not None else None, **cond)[0]
        big = m._loss(xt, yt, **cond)[0]
        fed = m.sample(eps, 1.0, yt, eps=eps, **cond)
        m._draws = DRAW_OFFSET
        y2 = yt[:2].contiguous() if yt is not None else None
        drawn = m.sample(xt[:2].contiguous(), None, y2, seed=SEED, **cond)
        keep = torch.as_tensor(KEEP, device=big.device)
        res = {"nll_one": one, "nll_big": big[keep], "sample_eps": fed[keep[[0, 2]]], "sample_philox": drawn}
        for kind, t in res.items():
            a = t.detach().cpu().numpy().astype(np.float32)
            assert np.isfinite(a).all(), (name, kind)
            out["%s__%s" % (name, kind)] = a
        # the first patch alone and at the head of the large batch: the same bits (also recorded, both)
        assert np.array_equal(out[name + "__nll_one"].view(np.uint32), out[name + "__nll_big"][:1].view(np.uint32)), name
    return out


@pytest.fixture(scope="module")
def outputs():
    return compute_outputs()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_split_kernel_bits_are_those_of_the_field_reading_kernel(outputs, name, kind):
    key = "%s__%s" % (name, kind)
    want = np.load(GOLDEN)[key]
    got = outputs[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    diff = got.view(np.uint32) != want.view(np.uint32)
    print("%s: %d of %d values differ in some bit" % (key, int(diff.sum()), diff.size))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
