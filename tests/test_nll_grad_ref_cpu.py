"""CPU tier of the NLL input gradients: the reference helper (tests/nll_grad_ref.py) is pinned to ``NoiseFlowOracle`` — its NLL
to the oracle's, its gradients to central differences of the oracle's NLL, a closed form for a model without couplings — and
``nf_grad_supported`` (host-only) is walked over the supported set and its refusals.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, make_inputs, trained_like_variables
from nll_grad_ref import PinnedRef, _scalar_pair
from oracle.nf_oracle import NoiseFlowOracle

ISO, CAM = 800.0, 2.0


@pytest.fixture(scope="module")
def shipped_ref(shipped_variables):
    return PinnedRef(FULL_ARCH, shipped_variables)


@pytest.mark.parametrize("hw", [(32, 32), (9, 13)])
def test_helper_nll_is_the_oracles(shipped_ref, oracle_full, hw):
    """Same fp64 arithmetic in another summation order (conv2d against shifted matmuls, 4 H W terms per sum): a few 1e-16 x
    sqrt(terms) relative; held to 1e-12."""
    x, y = make_inputs(2, hw[0], hw[1], seed=3)
    nll, _, _ = shipped_ref.nll_and_grads(x, y, ISO, CAM)
    want = oracle_full.nll(x, y, ISO, CAM)[0]
    print("helper vs oracle nll, relative:", np.abs(nll - want) / np.abs(want))
    assert np.all(np.abs(nll - want) <= 1e-12 * np.abs(want))


def test_helper_gradients_are_central_differences_of_the_oracle(shipped_ref, oracle_full):
    """h = 1e-7 for x, 1e-6 for y; every probed entry within 1e-6 of max|grad| of its patch (measured: 1.5e-8)."""
    H, W, B = 9, 13, 2
    x, y = make_inputs(B, H, W, seed=4)
    _, gx, gy = shipped_ref.nll_and_grads(x, y, ISO, CAM)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    rng = np.random.RandomState(0)
    worst = 0.0
    for name, g, h in (("x", gx, 1e-7), ("y", gy, 1e-6)):
        for _ in range(12):
            idx = (slice(None), rng.randint(H), rng.randint(W), rng.randint(4))   # the same entry of every patch: patches are independent
            d = np.zeros_like(x64)
            d[idx] = h
            if name == "x":
                fd = (oracle_full.nll(x64 + d, y64, ISO, CAM)[0] - oracle_full.nll(x64 - d, y64, ISO, CAM)[0]) / (2 * h)
            else:
                fd = (oracle_full.nll(x64, y64 + d, ISO, CAM)[0] - oracle_full.nll(x64, y64 - d, ISO, CAM)[0]) / (2 * h)
            err = np.abs(fd - g[idx]) / np.abs(g).reshape(B, -1).max(axis=1)
            worst = max(worst, float(err.max()))
            assert np.all(err <= 1e-6), (name, idx[1:], err)
    print("worst central-difference distance: %.2e of max|grad|" % worst)


def test_closed_form_without_couplings():
    """arch sdn5|gain4: nll = sum 0.5 log s^2 + 0.5 x^2 / s^2 + const with s^2 = (a y + b) g^2, so
    gx = x / s^2 and gy = (a g^2 / 2 s^2) (1 - x^2 / s^2)."""
    arch = "sdn5|gain4"
    v = trained_like_variables(arch, 4, seed=2)
    ref = PinnedRef(arch, v)
    x, y = make_inputs(2, 5, 7, seed=6)
    _, gx, gy = ref.nll_and_grads(x, y, ISO, CAM)
    a, b = _scalar_pair(ref.layers[0], ISO, CAM)
    g = float(np.asarray(ref.layers[1]["gain_val"]).reshape(-1)[0])
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    s2 = (a * y64 + b) * g * g
    np.testing.assert_allclose(gx, x64 / s2, rtol=1e-12, atol=0)
    want_gy = (a * g * g / (2 * s2)) * (1 - x64 * x64 / s2)
    assert np.abs(gy - want_gy).max() <= 1e-12 * np.abs(want_gy).max()


# ---- nf_grad_supported -------------------------------------------------------------------------------------------------------
WIDE_ARCH = "sdn5|unc|unc|gain4|unc"


def _supported(arch, variables, width, hw, flags=0):
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    rc = lib.nf_grad_supported(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
    return rc, (lib.nf_last_error() or b"").decode()


@pytest.mark.parametrize("width,hw", [(4, (1, 1)), (4, (1, 5)), (4, (9, 13)), (4, (32, 32)), (4, (64, 64)), (4, (64, 37)),
                                      (8, (16, 16)), (8, (32, 32)), (8, (48, 48)), (16, (16, 16)), (16, (32, 32)), (32, (16, 16))])
def test_grad_supported_set(width, hw):
    rc, msg = _supported(WIDE_ARCH, trained_like_variables(WIDE_ARCH, width), width, hw)
    assert rc == 0, msg


def test_grad_supported_shipped(shipped_variables):
    for hw in ((32, 32), (64, 64), (9, 13)):
        rc, msg = _supported(FULL_ARCH, shipped_variables, 4, hw)
        assert rc == 0, msg
    from noise_flow_amd import _lib
    rc, msg = _supported(FULL_ARCH, shipped_variables, 4, (32, 32), _lib.NF_CFG_EXACT_FP32)   # ignored
    assert rc == 0, msg


@pytest.mark.parametrize("width,hw,fp16,word", [(4, (32, 32), True, "fp32"),        # NF_CFG_FP16_CNN
                                                (4, (65, 65), False, "64x64"),      # tiled evaluation
                                                (64, (16, 16), False, "width"),     # the GEMM families
                                                (16, (64, 64), False, "width 16"),  # registers / LDS
                                                (8, (64, 64), False, "LDS"),
                                                (32, (32, 32), False, "LDS")])
def test_grad_supported_refusals(width, hw, fp16, word):
    from noise_flow_amd import _lib
    rc, msg = _supported(WIDE_ARCH, trained_like_variables(WIDE_ARCH, width), width, hw, _lib.NF_CFG_FP16_CNN if fp16 else 0)
    assert rc == _lib.NF_EINVAL
    assert msg and word in msg, msg
