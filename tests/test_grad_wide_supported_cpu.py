"""CPU tier of the matrix-core gradient kernel (NF_CFG_GRAD_MFMA, csrc/nf_grad_wide.hip): what ``nf_grad_supported`` accepts and
refuses with and without the flag (host only, no device), and the test model of the deep cases.

``paper_like_variables(arch, w)``: ``conftest.trained_like_variables`` with every ``l_2/W`` multiplied by sqrt(4 / w) and every
``l_last/W`` by sqrt(5 / (w + 1)), cast back to float32.  The per-layer gain of ``trained_like_variables`` grows with the width; at
width 32 and 8 couplings its fp32 reference is 1e-3 .. 0.4 away from fp64 (cascading gate flips), with the scaling 4e-7 .. 3e-6.
"""
import numpy as np
import pytest

from conftest import FULL_ARCH, trained_like_variables
from test_nll_grad_ref_cpu import WIDE_ARCH, _supported

NO_SDN_ARCH = "unc|gain4|unc"


def paper_like_variables(arch, width, seed=0):
    v = trained_like_variables(arch, width, seed=seed)
    for k in list(v):
        if k.endswith("l_2/W"):
            v[k] = (v[k] * np.sqrt(4.0 / width)).astype(np.float32)
        elif k.endswith("l_last/W"):
            v[k] = (v[k] * np.sqrt(5.0 / (width + 1))).astype(np.float32)
    return v


# (arch, width, H x W) of every accuracy case of tests/test_gpu_nll_grad_wide.py
ROWS = ([(FULL_ARCH, 17, (32, 32)), (FULL_ARCH, 32, (32, 32)), (FULL_ARCH, 32, (30, 27)), (FULL_ARCH, 32, (17, 31))] +
        [(FULL_ARCH, 32, hw) for hw in ((9, 32), (7, 32), (32, 5), (8, 8), (1, 32), (32, 1), (1, 1), (24, 24))] +
        [(WIDE_ARCH, 32, (32, 32)), (WIDE_ARCH, 32, (31, 29)), (WIDE_ARCH, 24, (32, 32)), (NO_SDN_ARCH, 32, (32, 32))])

_VARS = {}


def _vars(arch, width):
    if (arch, width) not in _VARS:
        _VARS[(arch, width)] = paper_like_variables(arch, width)
    return _VARS[(arch, width)]


@pytest.mark.parametrize("arch,width,hw", ROWS)
def test_supported_with_the_flag(arch, width, hw):
    from noise_flow_amd import _lib
    rc, msg = _supported(arch, _vars(arch, width), width, hw, _lib.NF_CFG_GRAD_MFMA)
    assert rc == 0, msg
    rc, msg = _supported(arch, _vars(arch, width), width, hw, _lib.NF_CFG_GRAD_MFMA | _lib.NF_CFG_EXACT_FP32)   # ignored
    assert rc == 0, msg


@pytest.mark.parametrize("arch,width", [(FULL_ARCH, 17), (FULL_ARCH, 32), (WIDE_ARCH, 24), (WIDE_ARCH, 32), (NO_SDN_ARCH, 32)])
def test_full_patch_is_refused_without_the_flag(arch, width):
    """flags = 0 is today's supported set: widths 17 .. 32 pad to 32, whose relu(h2) tile of a 32x32 patch does not fit the LDS."""
    from noise_flow_amd import _lib
    rc, msg = _supported(arch, _vars(arch, width), width, (32, 32), 0)
    assert rc == _lib.NF_EINVAL and "LDS" in msg, (rc, msg)


@pytest.mark.parametrize("width,hw,extra,word", [(32, (33, 32), 0, "32x32"), (32, (64, 64), 0, "32x32"), (32, (32, 33), 0, "32x32"),
                                                 (64, (16, 16), 0, "width"), (32, (32, 32), "fp16", "fp32")])
def test_refusals_with_the_flag(width, hw, extra, word):
    from noise_flow_amd import _lib
    flags = _lib.NF_CFG_GRAD_MFMA | (_lib.NF_CFG_FP16_CNN if extra == "fp16" else 0)
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, flags)
    assert rc == _lib.NF_EINVAL
    assert msg and word in msg, msg


def test_coupling_limit_is_named():
    """The gate record is 8 KiB per coupling on a 32x32 patch: 12 couplings fit beside the tiles and one weight image, 13 do not.
    A shorter patch has a smaller record (4 KiB per coupling at 16 rows) and holds them."""
    from noise_flow_amd import _lib
    for n, hw, want in ((12, (32, 32), 0), (13, (32, 32), _lib.NF_EINVAL), (13, (16, 32), 0)):
        arch = "sdn5|" + "|".join(["unc"] * n)
        rc, msg = _supported(arch, _vars(arch, 32), 32, hw, _lib.NF_CFG_GRAD_MFMA)
        assert rc == want, (n, hw, rc, msg)
        if want:
            assert "12 couplings" in msg and "LDS" in msg, msg


def test_flag_has_no_effect_on_narrow_widths():
    from noise_flow_amd import _lib
    for width, hw in ((8, (16, 16)), (16, (32, 32)), (4, (64, 64))):
        rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, _lib.NF_CFG_GRAD_MFMA)
        assert rc == 0, msg
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 16), 16, (64, 64), _lib.NF_CFG_GRAD_MFMA)   # refused as without the flag
    assert rc == _lib.NF_EINVAL and "width 16" in msg, msg


def test_flag_only_adds_to_the_supported_set():
    """Shapes beyond 32x32 that the scalar kernel holds at flags = 0 (at most 1 024 pixels, LDS) stay supported, on the scalar
    kernel, with the flag."""
    from noise_flow_amd import _lib
    from test_grad_wide_layout_cpu import _fold
    for hw in ((16, 48), (8, 64), (48, 16)):
        for flags in (0, _lib.NF_CFG_GRAD_MFMA):
            rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 32), 32, hw, flags)
            assert rc == 0, (hw, flags, msg)
        assert _fold(32, hw, _lib.NF_CFG_GRAD_MFMA)[0][0] == _lib.NF_GRAD_PATH_SCALAR


def test_unknown_flag_bits_are_still_rejected():
    from noise_flow_amd import _lib
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 8), 8, (16, 16), 8)
    assert rc == _lib.NF_EINVAL and "unknown bits" in msg, msg


def test_nf_grad_scalar_switch():
    """NF_GRAD=scalar (read once per process, hence the child): a flagged handle goes to the scalar kernel where that kernel holds
    the shape, and stays on the matrix-core kernel where it does not."""
    import os
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = %r\n"
            "from test_grad_wide_layout_cpu import _fold\n"
            "from noise_flow_amd import _lib\n"
            "print(_fold(32, (16, 16), _lib.NF_CFG_GRAD_MFMA)[0][0], _fold(32, (32, 32), _lib.NF_CFG_GRAD_MFMA)[0][0])\n"
            % [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))])
    for env, want in (("scalar", "0 1"), ("", "1 1")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NF_GRAD=env), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.split("\n")[-2].strip() == want, (env, out.stdout, out.stderr)
