"""CPU tier of nf_sample_vjp on the matrix-core kernel (NF_CFG_SVJP_MFMA, csrc/nf_sample_grad_wide.hip).  No device is touched.

1. Every case of tests/sample_vjp_wide_cases.py — the cases tests/test_gpu_sample_vjp_wide.py runs — holds the preconditions of
   tests/sample_vjp_ref.py (``reference_conditions``), and the REVERSIBLE float32 flavour of ``backward_sweep``, the arithmetic the
   kernel runs, meets the rule (``compare_with_kink_rule``) on it.
2. On the deep model at 32x32 the three mutants of tests/test_sample_vjp_rule_cpu.py stand at least MUTANT_FACTOR x above the bound.
3. ``nf_sample_vjp_supported`` with the new bit: 0 on every case, at width 8 (the scalar path) and together with
   NF_CFG_GRAD_TILED_WIDE at 32x32; 4. its refusals keep their words.

Measured on the CPU (float32 reversible sweep against float64, worst patch; the bound is max(1e-5, 4 e32) >= 1e-5): at most 0.16 of the
bound over the table (1.6e-6, gy of the deep model at 1x1).
"""
import ctypes as C

import numpy as np
import pytest

from sample_vjp_ref import WIDE_ARCH, backward_sweep, compare_with_kink_rule, reference_conditions, sampling_variables
from sample_vjp_wide_cases import DEEP_32x32, NAMES, NFGW_MAX_COUPLINGS_32, deep_variables, get_case, model
from test_sample_vjp_rule_cpu import MUTANT_FACTOR, _mutant_ratio


@pytest.mark.parametrize("name", NAMES)
def test_reversible_float32_sweep_meets_the_rule(name):
    _, ref, width, y, eps, g, temp, iso, cam, _ = get_case(name)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    got = backward_sweep(ref, y, eps, g, temp, iso, cam, np.float32, reversible=True)
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got[1:], log=print)


def test_mutants_stand_above_the_bound():
    _, ref, width, y, eps, g, temp, iso, cam, _ = get_case(DEEP_32x32)
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    sdn = [i for i, L in enumerate(ref.layers) if L["type"].startswith("sdn")]
    for mutant, tensor in ((("l1_tap", cpl[len(cpl) // 2]), "geps"), (("no_dls_lastcol", None), "geps"), (("gy_not_added", sdn[-1]), "gy")):
        r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, mutant, tensor)
        print("%s: %.3g x the bound" % (mutant[0], r))
        assert r >= MUTANT_FACTOR, (mutant, r)


# ---- nf_sample_vjp_supported ------------------------------------------------------------------------------------------------------
def _supported(arch, variables, width, hw, flags, **hps):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first", hps.get("flow_permutation", 1), hps.get("decomp", "LU"))
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    rc = lib.nf_sample_vjp_supported(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
    return rc, (lib.nf_last_error() or b"").decode()


def test_supported_set_with_the_bit():
    from noise_flow_amd import _lib
    assert _lib.NF_CFG_SVJP_MFMA == 256   # bit 8 stays unassigned: four CPU tests of the gradient flags pin it as "unknown bits"
    bit = _lib.NF_CFG_SVJP_MFMA
    for name in NAMES:
        key, _, width, _, eps, *_ = get_case(name)
        arch, v, _, hps, _ = model(key)
        rc, msg = _supported(arch, v, width, eps.shape[1:3], bit, **hps)
        assert rc == 0, (name, msg)
    rc, msg = _supported(WIDE_ARCH, sampling_variables(WIDE_ARCH, 8), 8, (16, 16), bit)   # the scalar path
    assert rc == 0, msg
    v32 = sampling_variables(WIDE_ARCH, 32)
    rc, msg = _supported(WIDE_ARCH, v32, 32, (32, 32), bit | _lib.NF_CFG_GRAD_TILED_WIDE)   # held whole
    assert rc == 0, msg
    rc, msg = _supported(WIDE_ARCH, v32, 32, (16, 48), bit)   # beyond 32x32 the scalar kernel, as far as it holds the shape
    assert rc == 0, msg
    arch = "|".join(["unc"] * NFGW_MAX_COUPLINGS_32)          # the most couplings the gate record of a 32x32 patch holds
    rc, msg = _supported(arch, sampling_variables(arch, 32), 32, (32, 32), bit)
    assert rc == 0, msg


def test_refusals_keep_their_words():
    from noise_flow_amd import _lib
    bit, E = _lib.NF_CFG_SVJP_MFMA, _lib.NF_EINVAL
    v32, v64 = sampling_variables(WIDE_ARCH, 32), sampling_variables(WIDE_ARCH, 64)
    deep = "|".join(["unc"] * (NFGW_MAX_COUPLINGS_32 + 1))
    rows = [
        (WIDE_ARCH, v32, 32, (32, 32), bit | _lib.NF_CFG_FP16_CNN, "fp32 handles only"),
        (WIDE_ARCH, v32, 32, (33, 32), bit, "32x32"),
        (WIDE_ARCH, v32, 32, (65, 64), bit | _lib.NF_CFG_GRAD_TILED_WIDE, "no tile mode"),
        (deep, sampling_variables(deep, 32), 32, (32, 32), bit, "couplings"),
        # without the bit the matrix-core layouts stay refused
        (WIDE_ARCH, v32, 32, (32, 32), _lib.NF_CFG_GRAD_MFMA, "matrix-core layout"),
        (WIDE_ARCH, v32, 32, (32, 32), _lib.NF_CFG_GRAD_TILED_WIDE, "matrix-core layout"),
        (WIDE_ARCH, v32, 32, (32, 32), 0, "LDS"),
    ]
    for arch, v, width, hw, flags, word in rows:
        rc, msg = _supported(arch, v, width, hw, flags)
        assert rc == E and msg.startswith("nf_sample_vjp") and word in msg, (width, hw, flags, rc, msg)
    # width 64: unchanged from a handle without the bit, whatever the other flags
    for base in (0, _lib.NF_CFG_GRAD_GEMM, _lib.NF_CFG_GRAD_TILED_GEMM):
        without, with_bit = (_supported(WIDE_ARCH, v64, 64, (16, 16), base | extra) for extra in (0, bit))
        assert without[0] == E and with_bit == without, (base, without, with_bit)


def test_deep_model_is_the_scaled_one():
    """D(w) is sampling_variables(FULL_ARCH, w) but for the two scaled weights of every coupling."""
    from conftest import FULL_ARCH
    a, b = sampling_variables(FULL_ARCH, 32), deep_variables(32)
    assert a.keys() == b.keys()
    for k in a:
        f = 0.5 if (k.endswith("l_2/W") or k.endswith("l_last/W")) else 1.0
        assert np.array_equal(b[k], (a[k] * np.float32(f)).astype(np.float32)), k
