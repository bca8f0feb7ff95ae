"""How the host describes the counted run of (mix, coupling) pairs to the split-bf16 kernel (nf_split_run_info: what nf_launch_flow
puts into the launch arguments, without a GPU).

The kernel addresses the A image of pair i of the run at run_aoff + i * run_astride and reads no NF12_CPL_AOFF field inside the run,
so the description must say exactly what the fields say — for every coupling of the run — or not exist: with run_first = -1 every
(mix, coupling) pair goes through the kernel's loop on its own and its field is read at the door of the loop, which is also how
couplings outside the run and couplings without a mix are served.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, trained_like_variables
from test_split_bf16 import DEEPEST_SPLIT, NF12_CPL_AOFF, _fold_layout

MIX, CPL_FWD, CPL_REV = 1, 2, 3
NF12_A_SIZE = 3072


def _info(ops, blk):
    from noise_flow_amd import _lib
    flat = (C.c_int32 * (2 * len(ops)))(*[v for op in ops for v in op])
    out = (C.c_int32 * 8)()
    blk = np.ascontiguousarray(blk, np.float32)
    _lib.check(_lib.load().nf_split_run_info(flat, len(ops), blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, out))
    return dict(zip(("first", "n", "moff", "coff", "stride", "type", "aoff", "astride"), (int(v) for v in out)))


def _field(blk, coff):
    return int(blk[coff + NF12_CPL_AOFF:coff + NF12_CPL_AOFF + 1].view(np.int32)[0])


def _set_field(blk, coff, value):
    blk[coff + NF12_CPL_AOFF:coff + NF12_CPL_AOFF + 1].view(np.int32)[0] = value


def _layout(arch, variables, direction, flow_permutation=1):
    from noise_flow_amd import _lib
    return _fold_layout(arch, variables, _lib.NF_PATH_SPLIT_BF16, direction=direction, flow_permutation=flow_permutation)


def _expected_run(ops):
    """(index of the first (mix, coupling) pair, number of pairs of that type that follow each other) or (-1, 0)."""
    for q in range(len(ops) - 1):
        if ops[q][0] == MIX and ops[q + 1][0] in (CPL_FWD, CPL_REV):
            n = 1
            while q + 2 * n + 1 < len(ops) and ops[q + 2 * n][0] == MIX and ops[q + 2 * n + 1][0] == ops[q + 1][0]:
                n += 1
            return q, n
    return -1, 0


def _check_description(ops, blk):
    r = _info(ops, blk)
    first, n = _expected_run(ops)
    assert (r["first"], r["n"]) == (first, n), (r, first, n)
    for i in range(n):
        (tm, moff), (tc, coff) = ops[first + 2 * i], ops[first + 2 * i + 1]
        assert tm == MIX and tc == r["type"]
        assert moff == r["moff"] + i * r["stride"] and coff == r["coff"] + i * r["stride"]
        assert _field(blk, coff) == r["aoff"] + i * r["astride"], (i, r)
        assert r["aoff"] + i * r["astride"] + NF12_A_SIZE <= blk.size
    return r


@pytest.mark.parametrize("direction", [0, 1])
def test_run_description_of_the_shipped_model_gives_every_couplings_field(shipped_variables, direction):
    ops, blk = _layout(FULL_ARCH, shipped_variables, direction)
    r = _check_description(ops, blk)
    # gain4 folds into its neighbours.  NLL direction: sdn5, then all eight pairs; sampling: the program starts with a coupling, the
    # run behind it is the other seven (its first image is the second one of the block), and the last mix stands alone before sdn5
    assert (r["first"], r["n"]) == ((1, 8) if direction == 0 else (1, 7))
    assert r["astride"] == NF12_A_SIZE
    first_image = min(_field(blk, o) for t, o in ops if t in (CPL_FWD, CPL_REV))
    assert r["aoff"] == first_image + (0 if direction == 0 else NF12_A_SIZE)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, DEEPEST_SPLIT])
def test_run_description_of_unc_stacks(n, direction):
    arch = "|".join(["unc"] * n)
    ops, blk = _layout(arch, trained_like_variables(arch, 4, seed=20 + n), direction)
    r = _check_description(ops, blk)
    assert r["n"] == (n if direction == 0 else n - 1)     # sampling: coupling first, the last mix on its own
    assert r["first"] == (0 if direction == 0 else (1 if n > 1 else -1))


@pytest.mark.parametrize("flow_permutation,has_run", [(0, True), (2, False)])
def test_run_description_with_the_other_mixing_layers(flow_permutation, has_run):
    """flow_permutation 0 folds the channel reversal to a mix (a run like any other); 2 has no mixing layer and therefore no run."""
    arch = "unc|unc|unc"
    ops, blk = _layout(arch, trained_like_variables(arch, 4, seed=3), 0, flow_permutation)
    r = _check_description(ops, blk)
    assert (r["first"] >= 0) == has_run


def test_fields_that_are_no_progression_leave_the_run_undescribed():
    arch = "unc|unc|unc|unc"
    ops, blk = _layout(arch, trained_like_variables(arch, 4, seed=4), 0)
    coffs = [o for t, o in ops if t == CPL_FWD]
    good = [_field(blk, c) for c in coffs]
    assert _check_description(ops, blk)["n"] == 4

    # two images exchanged between the first two of FOUR couplings: a_1, a_0, a_2, a_3 is no progression
    b = blk.copy()
    _set_field(b, coffs[0], good[1])
    _set_field(b, coffs[1], good[0])
    r = _info(ops, b)
    assert r["first"] == -1 and r["n"] == 0 and r["astride"] == 0, r

    # one coupling shares its neighbour's image
    b = blk.copy()
    _set_field(b, coffs[2], good[1])
    assert _info(ops, b)["first"] == -1

    # a progression that leaves the block (the last image would end beyond it), and a negative offset
    b = blk.copy()
    for i, c in enumerate(coffs):
        _set_field(b, c, good[0] + i * (NF12_A_SIZE + 4))
    assert _info(ops, b)["first"] == -1
    b = blk.copy()
    _set_field(b, coffs[0], -4)
    assert _info(ops, b)["first"] == -1


def test_a_reversed_progression_is_described_as_the_fields_say():
    """Two couplings whose images are exchanged: the fields ARE a progression (stride -3072), and the description follows them."""
    arch = "unc|unc"
    ops, blk = _layout(arch, trained_like_variables(arch, 4, seed=6), 0)
    coffs = [o for t, o in ops if t == CPL_FWD]
    a0, a1 = _field(blk, coffs[0]), _field(blk, coffs[1])
    _set_field(blk, coffs[0], a1)
    _set_field(blk, coffs[1], a0)
    r = _check_description(ops, blk)
    assert (r["aoff"], r["astride"]) == (a1, a0 - a1)
