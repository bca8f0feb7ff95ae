"""CPU tier of nf_sample_vjp: the reference helper (tests/sample_vjp_ref.py) is pinned to ``NoiseFlowOracle.sample`` and to its own
layer-by-layer sweep; the REVERSIBLE float32 flavour of that sweep — the arithmetic csrc/nf_sample_grad.hip runs — meets the rule on
every case of tests/test_gpu_sample_vjp.py; the mutants of the sweep stand at least 2x above the bound; and
``nf_sample_vjp_supported`` (host-only) is walked over its supported set and its refusals.  No device is touched.

Measured on the CPU (float32 reversible sweep against float64, worst patch; the bound is max(1e-5, 4 e32) >= 1e-5): at most 0.48 of the
bound on the shipped model (9x13, geps 4.8e-6), 0.6 .. 0.8e-6 on the width-16 / 32 cases.  Mutants, on geps: l1_tap 5e-3 .. 2e-1,
no_dls_lastcol 8e-3 .. 7e-1 of max|geps|.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH
from sample_vjp_ref import (CASES, SHIPPED_CASES, WIDE_ARCH, WIDTH_CASES, backward_sweep, compare_with_kink_rule, distances, get_case,
                            oracle_sample, reference_conditions, rule_weights, sampling_variables)

MUTANT_FACTOR = 2.0


@pytest.mark.parametrize("name", CASES, ids=repr)
def test_reference_is_the_oracle_and_the_sweep_is_autograd(shipped_variables, name):
    ref, width, y, eps, g, temp, iso, cam = get_case(name, shipped_variables)
    x64, gy64, ge64, gt64 = ref.sample_vjp(y, eps, g, temp, iso, cam)
    want = oracle_sample(ref, y, eps, temp, iso, cam)
    assert np.abs(x64 - want).max() <= 1e-12 * np.abs(want).max()
    for rev in (False, True):
        xs, gys, ges, gts = backward_sweep(ref, y, eps, g, temp, iso, cam, np.float64, reversible=rev)
        tol = 1e-12 if not rev else 1e-9     # the fp64 round trip through the stack is not exact: 1e-9 still pins every term
        assert np.abs(xs - x64).max() <= 1e-12 * np.abs(x64).max()
        assert np.abs(ges - ge64).max() <= tol * np.abs(ge64).max(), (rev, np.abs(ges - ge64).max() / np.abs(ge64).max())
        assert np.abs(gts - gt64).max() <= tol * np.abs(ge64 * eps).reshape(eps.shape[0], -1).sum(axis=1).max() / temp
        if gy64 is not None:
            assert np.abs(gys - gy64).max() <= tol * np.abs(gy64).max()
        else:
            assert gys is None


@pytest.mark.parametrize("name", CASES, ids=repr)
def test_reversible_float32_sweep_meets_the_rule(shipped_variables, name):
    ref, width, y, eps, g, temp, iso, cam = get_case(name, shipped_variables)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    got = backward_sweep(ref, y, eps, g, temp, iso, cam, np.float32, reversible=True)
    compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got[1:], log=print)


def _mutant_ratio(ref, y, eps, g, temp, iso, cam, mutant, tensor):
    """worst patch's distance of the fp64 mutant over the rule's bound, the smaller over the two norms."""
    want = ref.sample_vjp(y, eps, g, temp, iso, cam)
    r32 = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float32)
    w = rule_weights(ref, y, iso, cam, eps.shape)
    e32 = distances(r32[1:], want, y, eps, temp, w)
    d = distances(backward_sweep(ref, y, eps, g, temp, iso, cam, np.float64, mutant=mutant)[1:], want, y, eps, temp, w)
    return max(float((d[k] / np.maximum(1e-5, 4.0 * e32[k])).max()) for k in (tensor, tensor + "/w"))


@pytest.mark.parametrize("name", CASES, ids=repr)
def test_mutants_stand_above_the_bound(shipped_variables, name):
    ref, width, y, eps, g, temp, iso, cam = get_case(name, shipped_variables)
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    H, W = eps.shape[1:3]
    if H >= 2 and W >= 2:      # the dropped tap reads one pixel up and to the left of the last row: nothing there on a 1-pixel axis
        r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, ("l1_tap", cpl[len(cpl) // 2]), "geps")
        print("l1_tap: %.3g x the bound" % r)
        assert r >= MUTANT_FACTOR, r
    r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, ("no_dls_lastcol", None), "geps")
    print("no_dls_lastcol: %.3g x the bound" % r)
    assert r >= MUTANT_FACTOR, r
    sdn = [i for i, L in enumerate(ref.layers) if L["type"].startswith("sdn")]
    if len(sdn) > 1:           # the trailing sdn layer of the vocabulary model: where gy has teeth
        r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, ("gy_not_added", sdn[-1]), "gy")
        print("gy_not_added: %.3g x the bound" % r)
        assert r >= MUTANT_FACTOR, r


# ---- nf_sample_vjp_supported ------------------------------------------------------------------------------------------------------
def _supported(arch, variables, width, hw, flags=0):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    rc = lib.nf_sample_vjp_supported(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
    return rc, (lib.nf_last_error() or b"").decode()


def test_supported_set(shipped_variables):
    from noise_flow_amd import _lib
    for hw in SHIPPED_CASES + [(64, 37)]:
        for flags in (0, _lib.NF_CFG_GRAD_TILED, _lib.NF_CFG_EXACT_FP32):     # NF_CFG_GRAD_TILED on a shape held whole changes nothing
            rc, msg = _supported(FULL_ARCH, shipped_variables, 4, hw, flags)
            assert rc == 0, (hw, flags, msg)
    for width, hw in WIDTH_CASES:
        rc, msg = _supported(WIDE_ARCH, sampling_variables(WIDE_ARCH, width), width, hw)
        assert rc == 0, (width, hw, msg)
    # flags that act at other widths only leave the scalar block in place
    rc, msg = _supported(WIDE_ARCH, sampling_variables(WIDE_ARCH, 8), 8, (16, 16), _lib.NF_CFG_GRAD_MFMA | _lib.NF_CFG_GRAD_GEMM)
    assert rc == 0, msg


def test_refusals_name_the_limit(shipped_variables):
    from noise_flow_amd import _lib
    E = _lib.NF_EINVAL
    v32, v64 = sampling_variables(WIDE_ARCH, 32), sampling_variables(WIDE_ARCH, 64)
    rows = [
        (FULL_ARCH, shipped_variables, 4, (32, 32), _lib.NF_CFG_FP16_CNN, "fp32 handles only"),
        (FULL_ARCH, shipped_variables, 4, (65, 64), 0, "64x64"),
        (FULL_ARCH, shipped_variables, 4, (65, 64), _lib.NF_CFG_GRAD_TILED, "no tile mode"),
        (WIDE_ARCH, sampling_variables(WIDE_ARCH, 16), 16, (64, 64), 0, "1024 pixels"),
        (WIDE_ARCH, v32, 32, (32, 32), 0, "LDS"),
        ("unc", sampling_variables("unc", 8), 8, (58, 58), 0, "3072 pixels"),      # fits the LDS with one coupling; 768 threads x 4 pixels do not hold it
        (WIDE_ARCH, v32, 32, (16, 16), _lib.NF_CFG_GRAD_MFMA, "matrix-core layout"),
        (WIDE_ARCH, v32, 32, (16, 16), _lib.NF_CFG_GRAD_TILED_WIDE, "matrix-core layout"),
        (WIDE_ARCH, v64, 64, (16, 16), 0, "coupling widths up to 32"),
        (WIDE_ARCH, v64, 64, (16, 16), _lib.NF_CFG_GRAD_GEMM, "GEMM layout"),
        (WIDE_ARCH, v64, 64, (16, 16), _lib.NF_CFG_GRAD_TILED_GEMM, "GEMM layout"),
    ]
    for arch, v, width, hw, flags, word in rows:
        rc, msg = _supported(arch, v, width, hw, flags)
        assert rc == E and msg.startswith("nf_sample_vjp") and word in msg, (width, hw, flags, rc, msg)
