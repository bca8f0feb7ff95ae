"""CPU tier of the tiled input gradients at coupling width 32 (NF_CFG_GRAD_TILED_WIDE, csrc/nf_grad_wide.hip TILED): the flag's
value, what ``nf_grad_supported`` accepts and refuses with it, the plan ``nf_grad_tile_segments`` reports, that the bit is inert
at the narrower widths, and that ``nf_grad_fold`` hands the tiled path the weight image of the whole-patch matrix-core kernel.
Host arithmetic only; no device is touched.  The halo rule itself (4 per coupling) is pinned in fp64 by
tests/test_grad_tiles_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH
from test_grad_tiles_cpu import CPL, TILE, _axis
from test_grad_wide_supported_cpu import paper_like_variables
from test_nll_grad_ref_cpu import WIDE_ARCH, _supported

SHAPES = [(33, 33), (64, 64), (96, 80), (8, 66), (2, 40), (4096, 4096)]
DEEP_ARCH = "sdn5|" + "|".join(["unc"] * 13)      # one coupling more than the gate record of a 32x32 patch holds

_VARS = {}


def _vars(arch, width):
    if (arch, width) not in _VARS:
        _VARS[(arch, width)] = paper_like_variables(arch, width)
    return _VARS[(arch, width)]


def _flag():
    from noise_flow_amd import _lib
    return _lib.NF_CFG_GRAD_TILED_WIDE


@pytest.fixture(autouse=True)
def _no_forced_count(monkeypatch):
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)


def _plan(arch, width, hw, flags):
    """(return code of nf_grad_tile_segments, its rows, the op types of the NLL-order program)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, _vars(arch, width), width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    fp = flat.ctypes.data_as(C.POINTER(C.c_float))
    out = (C.c_int32 * 80)()
    n = lib.nf_grad_tile_segments(C.byref(cfg), descs, fp, flat.size, out, 16)
    ops = (C.c_int32 * 128)()
    n_ops = C.c_int32()
    cfg0 = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, 0)
    assert lib.nf_fold_params(C.byref(cfg0), descs, fp, flat.size, 0, ops, 64, C.byref(n_ops), None, 0, None, None) == 0
    return n, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))], [ops[2 * i] for i in range(n_ops.value)]


# ---- the flag -----------------------------------------------------------------------------------------------------------------
def test_flag_value_and_path_constant():
    from noise_flow_amd import _lib
    assert _flag() == 32 and _lib.NF_GRAD_PATH_TILED_WIDE32 == 3
    assert _lib.NF_CFG_GRAD_TILED == 16                                           # bit 8 stays unassigned


def test_flags_32_is_a_known_bit():
    """flags = 32 was "unknown bits"; bit 8 still is."""
    from noise_flow_amd import _lib
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 32), 32, (16, 16), 32)
    assert rc == 0, msg
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 8), 8, (16, 16), 32)
    assert rc == 0, msg
    for flags in (8, 8 | 32):
        rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 32), 32, (16, 16), flags)
        assert rc == _lib.NF_EINVAL and "unknown bits" in msg, msg


# ---- supported set and plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 17])
@pytest.mark.parametrize("arch", [WIDE_ARCH, FULL_ARCH])
@pytest.mark.parametrize("hw", SHAPES)
def test_supported_and_planned_beyond_32x32(arch, width, hw):
    from noise_flow_amd import _lib
    for flags in (_flag(), _flag() | _lib.NF_CFG_GRAD_MFMA | _lib.NF_CFG_GRAD_TILED | _lib.NF_CFG_EXACT_FP32):   # none of the others matters
        rc, msg = _supported(arch, _vars(arch, width), width, hw, flags)
        assert rc == 0, msg
        n, segs, types = _plan(arch, width, hw, flags)
        n_cpl = sum(1 for t in types if t in CPL)
        assert 1 <= n <= 16, (n, segs)
        assert segs[0][0] == 0 and segs[-1][1] == len(types)
        got = []
        for i, (op0, op1, halo, ny, nx) in enumerate(segs):
            c = sum(1 for t in types[op0:op1] if t in CPL)
            got.append(c)
            assert i == 0 or op0 == segs[i - 1][1]
            assert i == n - 1 or types[op1 - 1] in CPL
            assert 1 <= c <= 3 and halo == 4 * c and TILE - 2 * halo >= 8
            for size, cnt in ((hw[0], ny), (hw[1], nx)):
                assert cnt == _axis(size, halo)[0]                                # nf_tile_count, through nf_tile_plan
        assert sum(got) == n_cpl and max(got) - min(got) <= 1
    if hw[0] * hw[1] > 1024:          # without the bit: refused as before (up to 1 024 pixels the scalar kernel may hold the shape)
        rc, msg = _supported(arch, _vars(arch, width), width, hw, _lib.NF_CFG_GRAD_MFMA | _lib.NF_CFG_GRAD_TILED)
        assert rc == _lib.NF_EINVAL and msg


@pytest.mark.parametrize("forced,want", [(8, [1] * 8), (4, [2] * 4), (3, [3, 3, 2])])
def test_forced_counts(monkeypatch, forced, want):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    n, segs, types = _plan(FULL_ARCH, 32, (8, 66), _flag())
    assert n == forced and [s[2] for s in segs] == [4 * c for c in want]


def test_shapes_held_whole_report_no_segments():
    from noise_flow_amd import _lib
    from test_grad_wide_layout_cpu import _fold
    for hw in ((32, 32), (24, 24)):
        for arch in (WIDE_ARCH, FULL_ARCH):
            assert _plan(arch, 32, hw, _flag())[0] == 0, (arch, hw)
        assert _fold(32, hw, _flag())[0][0] == _lib.NF_GRAD_PATH_WIDE32          # as under NF_CFG_GRAD_MFMA
        assert _fold(32, hw, _lib.NF_CFG_GRAD_MFMA)[0][0] == _lib.NF_GRAD_PATH_WIDE32


def test_more_couplings_than_the_gate_record_holds_are_tiled():
    """13 couplings at 32x32: refused under NF_CFG_GRAD_MFMA (tests/test_grad_wide_supported_cpu.py), segments of at most 3 here —
    one tile per segment, the image itself."""
    from noise_flow_amd import _lib
    rc, msg = _supported(DEEP_ARCH, _vars(DEEP_ARCH, 32), 32, (32, 32), _lib.NF_CFG_GRAD_MFMA)
    assert rc == _lib.NF_EINVAL and "12 couplings" in msg
    rc, msg = _supported(DEEP_ARCH, _vars(DEEP_ARCH, 32), 32, (32, 32), _flag())
    assert rc == 0, msg
    n, segs, types = _plan(DEEP_ARCH, 32, (32, 32), _flag())
    assert n >= 5, (n, segs)
    for op0, op1, halo, ny, nx in segs:
        c = sum(1 for t in types[op0:op1] if t in CPL)
        assert 1 <= c <= 3 and halo == 4 * c and (ny, nx) == (1, 1)
    assert _plan(DEEP_ARCH, 32, (16, 32), _flag())[0] == 0                        # the shorter patch's record holds them: whole


# ---- refusals name their limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,hw,extra,word", [(32, (96, 80), "fp16", "fp32"), (32, (16, 16), "fp16", "fp32"),
                                                 (64, (96, 80), 0, "width"), (64, (16, 16), 0, "width"),
                                                 (32, (4097, 32), 0, "4096"), (32, (32, 4097), 0, "4096")])
def test_refusals_with_the_flag(width, hw, extra, word):
    from noise_flow_amd import _lib
    flags = _flag() | (_lib.NF_CFG_FP16_CNN if extra == "fp16" else 0)
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, flags)
    assert rc == _lib.NF_EINVAL
    assert msg and word in msg, msg


def test_infeasible_forced_count_fails(monkeypatch):
    """4 couplings in one segment: a halo of 16 leaves no core in a 32-pixel tile, and the gate record is sized for 3."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    for forced in ("2", "1"):
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", forced)
        for arch, hw in ((FULL_ARCH, (96, 80)), (FULL_ARCH, (8, 66)), (DEEP_ARCH, (32, 32))):
            assert _plan(arch, 32, hw, _flag())[0] == _lib.NF_EINVAL
            assert b"segments" in lib.nf_last_error()
            rc, msg = _supported(arch, _vars(arch, 32), 32, hw, _flag())
            assert rc == _lib.NF_EINVAL and "segments" in msg
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "3")
    assert _plan(FULL_ARCH, 32, (96, 80), _flag())[0] == 3


# ---- the bit is inert at widths 4 / 8 / 16 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8, 16])
def test_bit_is_inert_on_narrow_widths(width):
    from noise_flow_amd import _lib
    from test_grad_wide_layout_cpu import _fold
    for hw in ((16, 16), (32, 32), (40, 33), (64, 64), (96, 80)):
        for base in (0, _lib.NF_CFG_GRAD_TILED, _lib.NF_CFG_GRAD_MFMA, _lib.NF_CFG_GRAD_TILED | _lib.NF_CFG_GRAD_MFMA):
            a = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, base)
            b = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, base | _flag())
            assert a == b, (hw, base, a, b)                                       # return code and words
            pa, pb = _plan(WIDE_ARCH, width, hw, base), _plan(WIDE_ARCH, width, hw, base | _flag())
            assert pa == pb, (hw, base, pa, pb)
            fa, fb = _fold(width, hw, base), _fold(width, hw, base | _flag())
            if a[0] == 0:
                assert fa[0][0] == fb[0][0] and fa[0][1] == fb[0][1] and np.array_equal(fa[0][2].view(np.uint32), fb[0][2].view(np.uint32))
            else:
                assert fa[0] == fb[0] == _lib.NF_EINVAL


# ---- nf_grad_fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(33, 33), (64, 64), (96, 80), (2, 40)])
def test_fold_gives_the_matrix_core_image(hw):
    from noise_flow_amd import _lib
    from test_grad_wide_layout_cpu import _fold
    (path, ops, blk), _ = _fold(32, hw, _flag())
    (path0, ops0, blk0), _ = _fold(32, (32, 32), _lib.NF_CFG_GRAD_MFMA)
    assert path == _lib.NF_GRAD_PATH_TILED_WIDE32 == 3 and path0 == _lib.NF_GRAD_PATH_WIDE32
    assert ops == ops0 and blk.size == blk0.size and np.array_equal(blk.view(np.uint32), blk0.view(np.uint32))
