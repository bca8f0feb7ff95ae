"""CPU tier of the tiled input gradients at coupling widths 33 .. 512 (NF_CFG_GRAD_TILED_GEMM, csrc/nf_grad_gemm.hip TILED): the
flag's value, what ``nf_grad_supported`` accepts and refuses with it, the plan ``nf_grad_tile_segments`` reports, that shapes of
up to 32x32 stay on the whole-patch GEMM path, that ``nf_grad_fold`` hands the tiled path the weight image of the whole-patch GEMM
kernel, that the bit is inert at widths up to 32, that the refusals without the bit keep their words, and the Python keywords.
Host arithmetic only; no device is touched.  The halo rule itself (4 per coupling) is pinned in fp64 by
tests/test_grad_tiles_cpu.py and, on this path's own plans, by tests/test_nll_grad_rule_tiled_gemm_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH
from test_grad_tiles_cpu import CPL, TILE, _axis
from test_grad_wide_layout_cpu import _fold
from test_grad_wide_supported_cpu import paper_like_variables
from test_nll_grad_ref_cpu import WIDE_ARCH, _supported

SHAPES = [(33, 32), (64, 64), (96, 80), (4096, 4096)]
WIDTHS = [33, 64, 300, 512]

_VARS = {}


def _vars(arch, width):
    if (arch, width) not in _VARS:
        _VARS[(arch, width)] = paper_like_variables(arch, width)
    return _VARS[(arch, width)]


def _flag():
    from noise_flow_amd import _lib
    return _lib.NF_CFG_GRAD_TILED_GEMM


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
    assert _flag() == 128 and _lib.NF_GRAD_PATH_TILED_GEMM == 5
    assert _lib.NF_CFG_GRAD_GEMM == 64 and _lib.NF_GRAD_PATH_GEMM == 4


def test_flags_128_is_a_known_bit():
    """flags = 128 was "unknown bits"; bit 8 still is, alone and beside the new bit."""
    from noise_flow_amd import _lib
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 64), 64, (16, 16), 128)
    assert rc == 0, msg
    rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 8), 8, (16, 16), 128)
    assert rc == 0, msg
    for flags in (8, 8 | 128):
        rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 64), 64, (16, 16), flags)
        assert rc == _lib.NF_EINVAL and "unknown bits" in msg, msg


# ---- supported set and plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("hw", SHAPES)
def test_supported_and_planned_beyond_32x32(width, hw):
    from noise_flow_amd import _lib
    archs = (WIDE_ARCH, FULL_ARCH) if width in (64, 512) else (WIDE_ARCH,)
    for arch in archs:
        for flags in (_flag(), _flag() | _lib.NF_CFG_GRAD_GEMM | _lib.NF_CFG_GRAD_TILED):   # the bit implies NF_CFG_GRAD_GEMM
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
                    assert cnt == _axis(size, halo)[0]                            # nf_tile_count, through nf_tile_plan
            assert sum(got) == n_cpl and max(got) - min(got) <= 1


@pytest.mark.parametrize("forced,want", [(8, [1] * 8), (4, [2] * 4), (3, [3, 3, 2])])
def test_forced_counts(monkeypatch, forced, want):
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    n, segs, types = _plan(FULL_ARCH, 128, (8, 66), _flag())
    assert n == forced and [s[2] for s in segs] == [4 * c for c in want]


def test_infeasible_forced_count_fails(monkeypatch):
    """4 couplings in one segment: a halo of 16 leaves no core in a 32-pixel tile."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    for forced in ("2", "1"):
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", forced)
        for hw in ((96, 80), (8, 66)):
            assert _plan(FULL_ARCH, 64, hw, _flag())[0] == _lib.NF_EINVAL
            assert b"segments" in lib.nf_last_error()
            rc, msg = _supported(FULL_ARCH, _vars(FULL_ARCH, 64), 64, hw, _flag())
            assert rc == _lib.NF_EINVAL and "segments" in msg
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "3")
    assert _plan(FULL_ARCH, 64, (96, 80), _flag())[0] == 3


def test_shapes_held_whole_report_no_segments():
    from noise_flow_amd import _lib
    for width in (64, 300):
        for hw in ((32, 32), (24, 24), (1, 1)):
            for arch in (WIDE_ARCH, FULL_ARCH) if width == 64 else (WIDE_ARCH,):
                assert _plan(arch, width, hw, _flag())[0] == 0, (arch, hw)
            a, b = _fold(width, hw, _flag()), _fold(width, hw, _lib.NF_CFG_GRAD_GEMM)
            assert a[0][0] == b[0][0] == _lib.NF_GRAD_PATH_GEMM == 4              # program and block of the flag NF_CFG_GRAD_GEMM alone
            assert a[0][1] == b[0][1] and a[0][2].tobytes() == b[0][2].tobytes()


# ---- nf_grad_fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 300])
@pytest.mark.parametrize("hw", [(33, 32), (64, 64), (96, 80), (2, 40)])
def test_fold_gives_the_gemm_image(width, hw):
    from noise_flow_amd import _lib
    (path, ops, blk), _ = _fold(width, hw, _flag())
    (path0, ops0, blk0), _ = _fold(width, (32, 32), _lib.NF_CFG_GRAD_GEMM)
    assert path == _lib.NF_GRAD_PATH_TILED_GEMM == 5 and path0 == _lib.NF_GRAD_PATH_GEMM
    assert ops == ops0 and blk.size == blk0.size and blk.tobytes() == blk0.tobytes()


# ---- the bit is inert at widths up to 32 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 16, 32])
def test_bit_is_inert_up_to_width_32(width):
    from noise_flow_amd import _lib
    for hw in ((16, 16), (32, 32), (40, 33), (64, 64), (96, 80)):
        for base in (0, _lib.NF_CFG_GRAD_TILED, _lib.NF_CFG_GRAD_MFMA, _lib.NF_CFG_GRAD_TILED_WIDE, _lib.NF_CFG_GRAD_GEMM):
            a = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, base)
            b = _supported(WIDE_ARCH, _vars(WIDE_ARCH, width), width, hw, base | _flag())
            assert a == b, (hw, base, a, b)                                       # return code and words
            pa, pb = _plan(WIDE_ARCH, width, hw, base), _plan(WIDE_ARCH, width, hw, base | _flag())
            assert pa == pb, (hw, base, pa, pb)
            fa, fb = _fold(width, hw, base), _fold(width, hw, base | _flag())
            if a[0] == 0:
                assert fa[0][0] == fb[0][0] and fa[0][1] == fb[0][1] and fa[0][2].tobytes() == fb[0][2].tobytes()
            else:
                assert fa[0] == fb[0] == _lib.NF_EINVAL


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (96, 80)])
def test_fp16_is_refused(hw):
    from noise_flow_amd import _lib
    for flags in (_flag(), _flag() | _lib.NF_CFG_GRAD_GEMM):
        rc, msg = _supported(WIDE_ARCH, _vars(WIDE_ARCH, 64), 64, hw, flags | _lib.NF_CFG_FP16_CNN)
        assert rc == _lib.NF_EINVAL and "fp32" in msg, msg


@pytest.mark.parametrize("hw", [(8, 8), (40, 36)])
def test_coupling_limit_is_named(hw):
    """33 bare couplings sharing one parameter block, as tests/test_grad_gemm_cpu.py builds them: refused whole and on tiles."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack("unc", _vars("unc", 64), 64, "loss_first")
    cpl = [d for d in descs if d.width == 64][0]
    for n, want in ((32, 0), (33, _lib.NF_EINVAL)):
        many = (_lib.nf_layer_desc * n)(*[_lib.nf_layer_desc(cpl.type, cpl.width, cpl.param_offset) for _ in range(n)])
        cfg = _lib.nf_config(hw[0], hw[1], 4, n, -1, _flag())
        rc = lib.nf_grad_supported(C.byref(cfg), many, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size)
        msg = (lib.nf_last_error() or b"").decode()
        assert rc == want, (n, rc, msg)
        if want:
            assert "32 couplings" in msg, msg


def test_refusals_without_the_bit_keep_their_words():
    """NF_CFG_GRAD_GEMM alone or with NF_CFG_GRAD_TILED at 64x64: the refusal of a handle that has never heard of the new bit.  The
    words are taken from the library in this process (flags 64 and 64 | 16), and every other combination without the bit must give
    the same bytes; with the bit the same model and shape are supported."""
    from noise_flow_amd import _lib
    v = _vars(WIDE_ARCH, 64)
    rc64, msg64 = _supported(WIDE_ARCH, v, 64, (64, 64), 64)
    rc80, msg80 = _supported(WIDE_ARCH, v, 64, (64, 64), 64 | 16)
    assert rc64 == rc80 == _lib.NF_EINVAL and msg64 == msg80
    assert "no tile mode" in msg64 and "NF_CFG_GRAD_GEMM" in msg64 and "32x32" in msg64 and "64x64" in msg64
    for flags in (64 | 32, 64 | 16 | 32, 64 | 4, 64 | 2):
        assert _supported(WIDE_ARCH, v, 64, (64, 64), flags) == (rc64, msg64), flags
    for flags in (128, 64 | 128, 64 | 16 | 128):
        assert _supported(WIDE_ARCH, v, 64, (64, 64), flags)[0] == 0
    assert _supported(WIDE_ARCH, v, 64, (64, 64), 64) == (rc64, msg64)            # and asking with the bit left nothing behind
    rc0, msg0 = _supported(WIDE_ARCH, v, 64, (64, 64), 0)                         # without either flag: no gradient at these widths
    assert rc0 == _lib.NF_EINVAL and "the GEMM families have no gradient kernel" in msg0


# ---- Python -----------------------------------------------------------------------------------------------------------------
def test_grad_keywords(monkeypatch):
    """The stub of tests/test_grad_gemm_cpu.py::test_grad_kernel_keyword: the flags in the nf_config handed to nf_create."""
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from noise_flow_amd import noise_flow_model as nfm
    v = _vars(WIDE_ARCH, 64)
    seen = []

    class Recorded(Exception):
        pass

    class StubDev:
        def __init__(self, device=None):
            self.device = type("D", (), {"index": 0})()

    def recording(*a):
        seen.append(int(a[-1]))
        raise Recorded()

    monkeypatch.setattr(nfm, "_Dev", StubDev)
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "nf_config", recording)
        for kw, hps_kw in (({"grad_kernel": "gemm", "grad_tiles": True}, {}), ({}, {"grad_kernel": "gemm", "grad_tiles": True}),
                           ({"grad_kernel": "gemm"}, {}), ({"grad_tiles": True}, {}), ({"grad_kernel": "mfma", "grad_tiles": True}, {})):
            with pytest.raises(Recorded):
                NoiseFlow([64, 64, 4], False, default_hps(arch=WIDE_ARCH, width=64, **hps_kw), variables=v, **kw)
    assert seen == [64 | 16 | 128, 64 | 16 | 128, 64, 16, 4 | 16 | 32], seen
