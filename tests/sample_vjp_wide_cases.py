"""Models and cases of nf_sample_vjp on the matrix-core kernel (NF_CFG_SVJP_MFMA, csrc/nf_sample_grad_wide.hip) — helper, not a test.
Shared by tests/test_sample_vjp_wide_cpu.py and tests/test_gpu_sample_vjp_wide.py; the rule, constants, kink handling and preconditions
are those of tests/sample_vjp_ref.py, unchanged.

Models
  D(w)   deep model: ``sampling_variables(FULL_ARCH, w)`` with every l_2/W and l_last/W multiplied once more by 0.5.  As it stands that
         8-coupling model fails E32_MAX in the sampling direction at width 32 (e32 up to 2.9e-5 at temp 1), and paper_like_variables
         does too; with the extra 0.5, e32 <= 5e-7.
  scaled ``sampling_variables(WIDE_ARCH, w)`` as they are.
  V      vocabulary model: ``test_gpu_nll_grad_wide._vocab_variables(decomp)`` with the same 0.5 (without it the `rows` case reaches e32
         1.1e-5).
Inputs are ``case_inputs(B, H, W, seed)``; `keep` lists the patch indices that are used — the others have more than 6 on-kink
activations.  The shapes cover each dispatch arm of the kernel (<1,2>, <2,2>, <4,2>, <4,4>, <4,8>), a last strip that is not full,
W < 32 and one-pixel axes.
"""
import numpy as np

from conftest import FULL_ARCH
from sample_vjp_ref import CAM, ISO, TUPLES5, VOCAB_ARCH, WIDE_ARCH, SampleVjpRef, case_inputs, sampling_variables

NO_SDN_ARCH = "unc|gain4|unc"
DEEP_TEMP = 0.6
NFGW_MAX_COUPLINGS_32 = 12   # csrc/nf_device.h, nfgw_max_couplings(32): the gate record of a 32x32 patch beside the rest in 160 KiB


def _halved(v):
    for k in v:
        if k.endswith("l_2/W") or k.endswith("l_last/W"):
            v[k] = (v[k] * np.float32(0.5)).astype(np.float32)
    return v


def deep_variables(width):
    return _halved(sampling_variables(FULL_ARCH, width))


def vocab_variables(decomp="LU"):
    from test_gpu_nll_grad_wide import _vocab_variables
    return _halved(_vocab_variables(decomp))


# name -> (model key, hw, [(B, seed, keep or None)], temp, conditioning): conditioning "call" = (ISO, CAM), "vocab" = (1600, 3),
# "rows" = TUPLES5, None = a model without an sdn-kind layer (y = None)
def _deep(width, hw, draws, ident=None):
    return (ident or "D(%d) %dx%d" % (width, hw[0], hw[1]), ("deep", width), hw, draws, DEEP_TEMP, "call")


TABLE = (
    [_deep(32, (32, 32), [(4, 1, [2]), (4, 2, [1])]), _deep(32, (30, 27), [(3, 0, [0])]), _deep(32, (17, 31), [(3, 0, [1, 2])])] +
    [_deep(32, hw, [(3, 0, None)]) for hw in ((9, 32), (7, 32), (32, 5), (16, 16), (8, 8), (1, 32), (32, 1), (1, 1))] +
    [_deep(17, (32, 32), [(4, 1, None)])] +
    [("scaled w%d %dx%d" % (w, hw[0], hw[1]), ("scaled", w), hw, [(3, 0, None)], 1.0, "call") for w, hw in ((32, (32, 32)), (32, (31, 29)), (24, (32, 32)))] +
    [("V %r cond" % (hps,), ("vocab", tuple(sorted(hps.items()))), (12, 12), [(3, 0, None)], 1.0, "vocab") for hps in ({}, {"flow_permutation": 0}, {"decomp": "NONE"})] +
    [("V %r rows" % (hps,), ("vocab", tuple(sorted(hps.items()))), (12, 12), [(5, 0, None)], 1.0, "rows") for hps in ({}, {"flow_permutation": 0}, {"decomp": "NONE"})] +
    [("no sdn w32 8x8", ("nosdn", 32), (8, 8), [(3, 0, None)], 1.0, None)]
)
NAMES = [row[0] for row in TABLE]
DEEP_32x32 = NAMES[0]
_MODELS, _CASES = {}, {}


def model(key):
    """→ (arch, variables, coupling width, {flow_permutation / decomp}, reference), built once per model."""
    if key not in _MODELS:
        kind = key[0]
        if kind == "deep":
            arch, v, width, hps = FULL_ARCH, deep_variables(key[1]), key[1], {}
        elif kind == "scaled":
            arch, v, width, hps = WIDE_ARCH, sampling_variables(WIDE_ARCH, key[1]), key[1], {}
        elif kind == "vocab":
            hps = dict(key[1])
            arch, v, width = VOCAB_ARCH, vocab_variables(hps.get("decomp", "LU")), 32
        else:
            arch, v, width, hps = NO_SDN_ARCH, sampling_variables(NO_SDN_ARCH, key[1]), key[1], {}
        _MODELS[key] = (arch, v, width, hps, SampleVjpRef(arch, v, **hps))
    return _MODELS[key]


def get_case(name):
    """→ (model key, ref, width, y or None, eps, g, temp, iso, cam, rows: bool), the arrays built once (the reference memoises by them)."""
    if name not in _CASES:
        _, key, hw, draws, temp, cnd = TABLE[NAMES.index(name)]
        _, _, width, _, ref = model(key)
        parts = []
        for B, seed, keep in draws:
            y, eps, g = case_inputs(B, hw[0], hw[1], seed)
            sel = list(range(B)) if keep is None else keep
            parts.append((y[sel], eps[sel], g[sel]))
        y, eps, g = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(3))
        iso, cam = {"call": (ISO, CAM), "vocab": (1600.0, 3.0), None: (None, None),
                    "rows": (np.array([t[0] for t in TUPLES5], np.float64), np.array([t[1] for t in TUPLES5], np.float64))}[cnd]
        _CASES[name] = (key, ref, width, None if cnd is None else y, eps, g, temp, iso, cam, cnd == "rows")
    return _CASES[name]
