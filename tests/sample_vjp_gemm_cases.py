"""Models and cases of nf_sample_vjp on the GEMM kernel (NF_CFG_SVJP_GEMM, csrc/nf_sample_grad_gemm.hip) — helper, not a test.
Shared by tests/test_sample_vjp_gemm_cpu.py and tests/test_gpu_sample_vjp_gemm.py; the rule, constants, kink handling and preconditions
are those of tests/sample_vjp_ref.py, unchanged.

Models
  scaled    ``sampling_variables(WIDE_ARCH, w)`` as they are, temperature 1: every channel live, every padded width (64 / 128 / 256 / 512).
  embedded  ``test_grad_gemm_cpu.embedded_variables(deep_variables(32), W)``, W = 128 / 512: the 32 live channels of D(32)
            (tests/sample_vjp_wide_cases.py) scattered one per slab of a width-W model, held to the WIDTH-32 reference of D(32) on the two
            patches of that file's DEEP_32x32 at temperature 0.6 — the full 32x32 patch at the real widths (4 and 16 bands, 8 couplings).
            Dense models there have 19 .. 33 on-kink activations per patch, beyond the cap.
  V         vocabulary model at width 64: ``test_gpu_nll_grad_gemm._vocab_variables()`` (the weight scaling of the GEMM gradient tests)
            with the extra 0.5 of ``sample_vjp_wide_cases._halved`` and, for decomp='NONE', the same matrices as the variable itself.
  no sdn    ``sampling_variables(NO_SDN_ARCH, 64)``, y = None.
Inputs are ``case_inputs(4, H, W, seed)`` (5 patches for `rows`); `keep` lists the patch indices that are used — the others have more than
6 on-kink activations in the float64 reference.  Per row below: on-kink activations per kept patch, largest pinned e32 (from the reference
alone, on the CPU).
"""
import numpy as np

from sample_vjp_ref import CAM, ISO, TUPLES5, VOCAB_ARCH, WIDE_ARCH, SampleVjpRef, case_inputs, sampling_variables
from sample_vjp_wide_cases import DEEP_32x32, DEEP_TEMP, NO_SDN_ARCH, _halved, deep_variables
from sample_vjp_wide_cases import get_case as wide_case
from sample_vjp_wide_cases import model as wide_model

VW = 64                      # the vocabulary model's coupling width
NFGG_MAX_COUPLINGS = 32      # csrc/nf_gemm_layout.h
EMBEDDED_WIDTHS = (128, 512)


def vocab_variables(decomp="LU"):
    from oracle import nf_oracle as O
    from test_gpu_nll_grad_gemm import _vocab_variables
    v = _halved(_vocab_variables())
    if decomp == "NONE":   # the same matrices, as the variable itself
        for lyr, i in O.parse_arch(VOCAB_ARCH):
            if lyr == "unc":
                A = O.conv1x1_from_variables(v, i, "LU", np.float64)[0]
                for name in O.conv1x1_variable_names(i, "LU").values():
                    del v[name]
                v[O.conv1x1_variable_names(i, "NONE")["A"]] = A.astype(np.float32)
    return v


def _scaled(width, hw, draws):
    return ("scaled w%d %dx%d" % (width, hw[0], hw[1]), ("scaled", width), hw, draws, 1.0, "call")


# name -> (model key, hw, [(B, seed, keep or None)], temp, conditioning) as tests/sample_vjp_wide_cases.py
TABLE = (
    [_scaled(40, (32, 32), [(4, 1, None)]),                      # 2 bands, padding 40 -> 64
     _scaled(64, (32, 32), [(4, 0, [1]), (4, 2, [2])]),          # 2 full bands
     _scaled(33, (16, 16), [(4, 0, [0, 1])]),                    # smallest padded case
     _scaled(128, (11, 14), [(4, 0, None)]),                     # one partial band
     _scaled(128, (16, 16), [(4, 3, [0, 1, 3])]),                # exactly one full band
     _scaled(200, (9, 13), [(4, 3, None)]),                      # WP = 256
     _scaled(256, (8, 8), [(4, 3, None)]),
     _scaled(300, (7, 10), [(4, 1, [0, 1, 2])]),                 # WP = 512, 2 bands
     _scaled(512, (5, 9), [(4, 2, [0, 2]), (4, 3, [2, 3])])] +   # WP = 512
    [_scaled(64, hw, [(4, 0, None)]) for hw in ((1, 1), (1, 32), (32, 1), (7, 32), (32, 5))] +   # one-pixel axes, W < 32
    [_scaled(64, (17, 31), [(4, 0, None)])] +                    # odd pitch, the second owned pixel partly idle
    [("V %r cond" % (hps,), ("vocab", tuple(sorted(hps.items()))), (12, 12), [(4, 0, None)], 1.0, "vocab")
     for hps in ({}, {"flow_permutation": 0}, {"decomp": "NONE"})] +
    [("V %r rows" % (hps,), ("vocab", tuple(sorted(hps.items()))), (12, 12), [(5, 0, None)], 1.0, "rows")
     for hps in ({}, {"flow_permutation": 0}, {"decomp": "NONE"})] +
    [("no sdn w64 8x8", ("nosdn", 64), (8, 8), [(4, 0, None)], 1.0, None)]
)
NAMES = [row[0] for row in TABLE]
W64_32x32 = NAMES[1]
_MODELS, _CASES = {}, {}


def model(key):
    """→ (arch, variables, coupling width, {flow_permutation / decomp}, reference), built once per model."""
    if key not in _MODELS:
        kind = key[0]
        if kind == "scaled":
            arch, v, width, hps = WIDE_ARCH, sampling_variables(WIDE_ARCH, key[1]), key[1], {}
        elif kind == "vocab":
            hps = dict(key[1])
            arch, v, width = VOCAB_ARCH, vocab_variables(hps.get("decomp", "LU")), VW
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


def embedded_case(W):
    """→ (arch, variables of the width-W model, ref of D(32), 32, y, eps, g, temp, iso, cam): the kernel runs the width-W model, the
    reference (and its kink numbering) is D(32)'s on the two patches of DEEP_32x32."""
    from test_grad_gemm_cpu import embedded_variables
    key, ref, width, y, eps, g, temp, iso, cam, _ = wide_case(DEEP_32x32)
    arch, v32, _, _, _ = wide_model(key)
    assert width == 32 and temp == DEEP_TEMP and eps.shape == (2, 32, 32, 4)
    return arch, embedded_variables(v32, W), ref, 32, y, eps, g, temp, iso, cam


__all__ = ["EMBEDDED_WIDTHS", "NAMES", "NFGG_MAX_COUPLINGS", "TABLE", "VW", "W64_32x32", "deep_variables", "embedded_case", "get_case", "model",
           "vocab_variables"]
