"""CPU tier of nf_sample_vjp on the GEMM kernel (NF_CFG_SVJP_GEMM, csrc/nf_sample_grad_gemm.hip).  No device is touched.

1. Every case of tests/sample_vjp_gemm_cases.py — the cases tests/test_gpu_sample_vjp_gemm.py runs — holds the preconditions of
   tests/sample_vjp_ref.py (``reference_conditions``), and the REVERSIBLE float32 flavour of ``backward_sweep``, the arithmetic the
   kernel runs, meets the rule (``compare_with_kink_rule``) on it.  The embedded cases are D(32)'s two 32x32 patches, held to both on
   the width-32 reference; the width-128 / 512 models are shown to carry D(32)'s weights and zeros.
2. On the width-64 32x32 case the three mutants of tests/test_sample_vjp_rule_cpu.py stand at least MUTANT_FACTOR x above the bound.
3. The flag's value, and bit 8 is still unknown.
4. ``nf_sample_vjp_supported`` with the bit: 0 on every case and at NFGG_MAX_COUPLINGS couplings.
5. Its refusals name the limit; 6. without the bit every (rc, message) at width 64 is the parent's; 7. at widths 8 and 32 the bit
   changes nothing; 8. the ``sample_vjp_kernel="gemm"`` keyword is validated before a handle is made.

Measured on the CPU (float32 reversible sweep against float64, worst patch; the bound is max(1e-5, 4 e32) >= 1e-5): printed by test 1
(run with -s).
"""
import ctypes as C

import numpy as np
import pytest

from sample_vjp_gemm_cases import EMBEDDED_WIDTHS, NAMES, NFGG_MAX_COUPLINGS, W64_32x32, embedded_case, get_case, model
from sample_vjp_ref import (WIDE_ARCH, backward_sweep, compare_with_kink_rule, reference_conditions, sampling_variables)
from test_sample_vjp_rule_cpu import MUTANT_FACTOR, _mutant_ratio


# ---- 1. the cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reversible_float32_sweep_meets_the_rule(name):
    _, ref, width, y, eps, g, temp, iso, cam, _ = get_case(name)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    got = backward_sweep(ref, y, eps, g, temp, iso, cam, np.float32, reversible=True)
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got[1:], log=print)


@pytest.mark.parametrize("W", EMBEDDED_WIDTHS)
def test_embedded_model_is_the_width_32_one(W):
    """The embedded cases are held to the width-32 reference of D(32): its two patches meet the preconditions and the float32 reversible
    sweep meets the rule on them (the reference's own width: cheap), and the width-W model carries D(32)'s weights and nothing else (every other entry of the
    three convolutions is zero), so that the two are one function."""
    from sample_vjp_wide_cases import deep_variables
    arch, vW, ref, width, y, eps, g, temp, iso, cam = embedded_case(W)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    got = backward_sweep(ref, y, eps, g, temp, iso, cam, np.float32, reversible=True)
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got[1:], log=print)
    v32 = deep_variables(32)
    assert width == 32 and vW.keys() == v32.keys() and eps.shape == (2, 32, 32, 4) and temp == 0.6
    for k, a in v32.items():
        a, b = np.asarray(a, np.float64), np.asarray(vW[k], np.float64)
        if b.shape == a.shape:
            assert np.array_equal(b, a), k
        else:
            ones = (W - 32) if k.endswith("/var") else 0      # the padded channels' unit variances
            assert np.count_nonzero(b) <= np.count_nonzero(a) + ones, k
            assert np.isclose(np.abs(b).sum() - ones, np.abs(a).sum(), rtol=1e-9), k


# ---- 2. the mutants ------------------------------------------------------------------------------------------------------------------
def test_mutants_stand_above_the_bound():
    _, ref, width, y, eps, g, temp, iso, cam, _ = get_case(W64_32x32)
    assert width == 64 and eps.shape[1:3] == (32, 32)
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    sdn = [i for i, L in enumerate(ref.layers) if L["type"].startswith("sdn")]
    for mutant, tensor in ((("l1_tap", cpl[len(cpl) // 2]), "geps"), (("no_dls_lastcol", None), "geps"), (("gy_not_added", sdn[-1]), "gy")):
        r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, mutant, tensor)
        print("%s: %.3g x the bound" % (mutant[0], r))
        assert r >= MUTANT_FACTOR, (mutant, r)


# ---- nf_sample_vjp_supported ---------------------------------------------------------------------------------------------------------
def _supported(arch, variables, width, hw, flags, **hps):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first", hps.get("flow_permutation", 1), hps.get("decomp", "LU"))
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    rc = lib.nf_sample_vjp_supported(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
    return rc, (lib.nf_last_error() or b"").decode()


def _bare_couplings(n, flags):
    """n bare couplings of width 64 sharing one parameter block, on 8x8, through the C ABI (as tests/test_grad_gemm_cpu.py: the
    architecture grammar cannot exceed 32 couplings, a coupling comes with its 1x1 matrix and a model has at most 64 layers)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    _, descs, flat = params.pack("unc", _v("unc", 64), 64, "loss_first")
    cpl = [d for d in descs if d.width == 64][0]
    many = (_lib.nf_layer_desc * n)(*[_lib.nf_layer_desc(cpl.type, cpl.width, cpl.param_offset) for _ in range(n)])
    cfg = _lib.nf_config(8, 8, 4, n, -1, flags)
    rc = lib.nf_sample_vjp_supported(C.byref(cfg), many, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
    return rc, (lib.nf_last_error() or b"").decode()


_V = {}


def _v(arch, width):
    if (arch, width) not in _V:
        _V[(arch, width)] = sampling_variables(arch, width)
    return _V[(arch, width)]


# ---- 3. ----
def test_flag_value_and_bit_8_stays_unknown():
    from noise_flow_amd import _lib
    assert _lib.NF_CFG_SVJP_GEMM == 1024 and _lib.NF_SVJP_PATH_GEMM == 3
    for flags in (8, 8 | 1024):
        rc, msg = _supported(WIDE_ARCH, _v(WIDE_ARCH, 64), 64, (16, 16), flags)
        assert rc == _lib.NF_EINVAL and "unknown bits" in msg, (flags, rc, msg)


# ---- 4. (the test that fails without the feature: 1024 is an unknown bit there) ----
def test_supported_set_with_the_bit():
    from noise_flow_amd import _lib
    bit = _lib.NF_CFG_SVJP_GEMM
    for name in NAMES:
        key, _, width, _, eps, *_ = get_case(name)
        arch, v, _, hps, _ = model(key)
        rc, msg = _supported(arch, v, width, eps.shape[1:3], bit, **hps)
        assert rc == 0, (name, msg)
    for W in EMBEDDED_WIDTHS:
        arch, vW, *_ = embedded_case(W)
        rc, msg = _supported(arch, vW, W, (32, 32), bit)
        assert rc == 0, (W, msg)
    # together with the gradient flags it includes or stands beside: the same answer
    for extra in (_lib.NF_CFG_GRAD_GEMM, _lib.NF_CFG_GRAD_TILED_GEMM, _lib.NF_CFG_SVJP_MFMA | _lib.NF_CFG_SVJP_TILED):
        rc, msg = _supported(WIDE_ARCH, _v(WIDE_ARCH, 64), 64, (32, 32), bit | extra)
        assert rc == 0, (extra, msg)
    rc, msg = _bare_couplings(NFGG_MAX_COUPLINGS, bit)     # the most couplings the path takes
    assert rc == 0, msg


# ---- 5. ----
def test_refusals_with_the_bit_name_the_limit():
    from noise_flow_amd import _lib
    bit, E = _lib.NF_CFG_SVJP_GEMM, _lib.NF_EINVAL
    v64 = _v(WIDE_ARCH, 64)
    rows = [
        (WIDE_ARCH, v64, (33, 32), bit, "32x32"),
        (WIDE_ARCH, v64, (33, 32), bit, "no tile mode"),
        (WIDE_ARCH, v64, (65, 64), bit | _lib.NF_CFG_GRAD_TILED_GEMM, "no tile mode"),
        (WIDE_ARCH, v64, (65, 64), bit | _lib.NF_CFG_GRAD_TILED_GEMM, "NF_CFG_SVJP_GEMM"),
        (WIDE_ARCH, v64, (32, 32), bit | _lib.NF_CFG_FP16_CNN, "fp32 handles only"),
    ]
    for arch, v, hw, flags, word in rows:
        rc, msg = _supported(arch, v, 64, hw, flags)
        assert rc == E and msg.startswith("nf_sample_vjp") and word in msg, (hw, flags, rc, msg)
    rc, msg = _bare_couplings(NFGG_MAX_COUPLINGS + 1, bit)
    assert rc == E and msg.startswith("nf_sample_vjp") and "at most %d couplings" % NFGG_MAX_COUPLINGS in msg, (rc, msg)


# ---- 6. (the strings of the parent build) ----
PARENT_W64 = {
    "0": "nf_sample_vjp: coupling widths up to 32 (64 given; the GEMM families have no gradient kernel)",
    "NF_CFG_GRAD_GEMM": "nf_sample_vjp: the handle's gradient block is in the GEMM layout (NF_CFG_GRAD_GEMM / NF_CFG_GRAD_TILED_GEMM at coupling "
                        "width 64); the scalar layout only: no matrix-core or GEMM variant yet",
    "NF_CFG_GRAD_TILED_GEMM": "nf_sample_vjp: the handle's gradient block is in the GEMM layout (NF_CFG_GRAD_GEMM / NF_CFG_GRAD_TILED_GEMM at "
                              "coupling width 64); the scalar layout only: no matrix-core or GEMM variant yet",
}


def test_without_the_bit_width_64_answers_as_the_parent_did():
    from noise_flow_amd import _lib
    for name, want in PARENT_W64.items():
        flags = 0 if name == "0" else getattr(_lib, name)
        for hw in ((16, 16), (32, 32)):
            assert _supported(WIDE_ARCH, _v(WIDE_ARCH, 64), 64, hw, flags) == (_lib.NF_EINVAL, want), (name, hw)


# ---- 7. ----
def test_the_bit_changes_nothing_at_widths_up_to_32():
    from noise_flow_amd import _lib
    bit = _lib.NF_CFG_SVJP_GEMM
    for width, hw, base in ((8, (16, 16), 0), (32, (32, 32), _lib.NF_CFG_SVJP_MFMA), (32, (16, 16), 0), (32, (32, 32), 0),
                            (32, (32, 32), _lib.NF_CFG_FP16_CNN), (4, (65, 64), 0)):
        without, with_bit = (_supported(WIDE_ARCH, _v(WIDE_ARCH, width), width, hw, base | extra) for extra in (0, bit))
        assert with_bit == without, (width, hw, base, without, with_bit)
    rc, _ = _supported(WIDE_ARCH, _v(WIDE_ARCH, 8), 8, (16, 16), bit)
    assert rc == 0
    rc, _ = _supported(WIDE_ARCH, _v(WIDE_ARCH, 32), 32, (32, 32), bit | _lib.NF_CFG_SVJP_MFMA)
    assert rc == 0
    # (which kernel such a handle launches needs a handle: tests/test_gpu_sample_vjp_gemm.py asserts the paths on the device)


# ---- 8. ----
def test_keyword_validation():
    """FlowHandle validates the keyword before it makes a handle (NoiseFlow passes it through and needs a device: the GPU file)."""
    from noise_flow_amd.noise_flow_model import FlowHandle
    for width in (8, 32):
        with pytest.raises(ValueError, match="33 .. 512"):
            FlowHandle(WIDE_ARCH, _v(WIDE_ARCH, width), (16, 16, 4), width, sample_vjp_kernel="gemm")
    with pytest.raises(ValueError, match="fp32 handle"):
        FlowHandle(WIDE_ARCH, _v(WIDE_ARCH, 64), (16, 16, 4), 64, cnn_dtype="fp16", sample_vjp_kernel="gemm")
    with pytest.raises(ValueError, match="'scalar', 'mfma' or 'gemm'"):
        FlowHandle(WIDE_ARCH, _v(WIDE_ARCH, 64), (16, 16, 4), 64, sample_vjp_kernel="wide")
