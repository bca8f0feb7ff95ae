"""The trainer's matrix-core GEMMs (csrc/nf_train_mm.h), launched directly and held to fp32 resolution.

Training beyond width 64 runs its dense products on `k_mm_pix<.., PREC = 1>` (8 and 4 wavefronts) and `k_mm_kpix6`: "bf16 x 6",
fp32-accurate products on the bf16 matrix pipe.  The trainer picks them only from multi_processor_count x 128 pixels up (or under
NF_MM_MODE, read once per process), so no other test of the suite reaches them; here tools/probes/libmm_check.so (built by
build() with `make probe`, loaded with ctypes) launches every instantiation csrc/nf_train_gemm.h uses with more than 64 output
channels in mode 0 (the exact-fp32 twin), 2 and 3, with `mm::Ctx{n_cu, device, mode}`.

Rule, per output element, every mode:     |kernel - ref64| <= U_B * 2^-24 * T
T = the fp64 sum of the magnitudes of every term that reaches the element (|A| . |W|^T; with the BN + ReLU prologue |A| is
|h r| + |(b - m) r|; the stored BN backward adds |ba| + |xhat bq| and is scaled by rstd); ref64 applies prologue and epilogue in
fp64 to the fp32 inputs.  Batch sums: the slots are added in fp64 and held to U_S[P] * 2^-24 * sum over the pixels |summand|; the
buffer is pre-filled with NaN, so a slot that is neither written nor cleared shows, and the slots beyond `nslot` must still hold
it.  The partial products of the pixel-K launch are added in fp64 and held to the rule with T = sum over pixels |pro(A)| |B|.
A failure in mode 0 is a mistake of the reference, not a precision question.

U_B = 31 and U_S are derived in tests/test_train_mm_bound_cpu.py on the CPU, against the reference and never against a kernel
(twice the worst distance of a plain float32 evaluation: 15.36 units on the wide_range family at K = 132); the same file owns
cases, inputs and references, and shows that the emulated six-product scheme stays below 9.7 units while each single dropped
product is beyond 73 on some family of every case with K <= 132.  Mask inputs (the pre-BN activation of EPI 2 / 3 / 4) are kept
2^-16 (1 + |xhat|) away from their kink; there is no kink rule here.  (APRO 2 has no launch with more than 64 output channels, so
no A2 operand appears.)

Measured on an MI355X, worst element over 5 families x 3 seeds, units of 2^-24 T: see profiles/r14_train_mm_units.txt.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from test_split_bf16 import FAMILIES
from test_train_mm_bound_cpu import (KPIX_CASES, KPIX_IDS, KPIX_PART_CAP, PIX_CASES, PIX_IDS, SEEDS, U_B, U_S, kpix_operands,
                                     kpix_reference, pix_operands, pix_reference, units)

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tools", "probes", "libmm_check.so")
MODES = (0, 2, 3)
SLOT_STRIDE = 1024                  # mm::kSlotStride
WORST = {}                          # (instantiation, mode, what) -> worst units seen by the tests of this run


def _lib():
    assert os.path.exists(LIB), "tools/probes/libmm_check.so is missing: run build()"
    lib = C.CDLL(LIB)
    p, i, ll = C.c_void_p, C.c_int, C.c_longlong
    lib.mmc_pix.restype = i
    lib.mmc_pix.argtypes = [i, i, i, i, ll, i, i, p, i, p, i, p, i, p, p, p, p, p, i, p, p, i, i, p]
    lib.mmc_kpix.restype = i
    lib.mmc_kpix.argtypes = [i, ll, i, i, p, i, p, i, p, p, p, ll, i, p]
    return lib


def _gpu():
    import torch
    return torch, torch.cuda.get_device_properties(0).multi_processor_count, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _note(key, u):
    WORST[key] = max(WORST.get(key, 0.0), u)


def test_an_unknown_combination_is_refused():
    lib = _lib()
    assert lib.mmc_pix(2, 2, 0, 4, 1, 1, 1, None, 1, None, 4, None, 1, None, None, None, None, None, 1, None, None, 1, 1, None) == -1


@pytest.mark.parametrize("case", PIX_CASES, ids=PIX_IDS)
def test_k_mm_pix_every_mode_within_the_fp32_bound(case):
    torch, n_cu, stream = _gpu()
    lib = _lib()
    apro, epi, av, P, N, K, nslot = case
    ldb = (K + 3) & ~3
    inst = "pix<%d,%d,%d>" % (apro, epi, av)
    nan = float("nan")
    lines, bad = [], []
    for name in FAMILIES:
        for seed in SEEDS:
            o = pix_operands(case, name, seed)
            ref = pix_reference(case, o)
            d = {k: torch.from_numpy(v).cuda() for k, v in o.items()}
            Bt = torch.zeros(N, ldb, device="cuda")
            Bt[:, :K] = d["W"]
            ptr = lambda k: d[k].data_ptr() if k in d else None      # noqa: E731
            for mode in MODES:
                out = torch.full((P, N), nan, device="cuda")
                stats = torch.full((2 * N, SLOT_STRIDE), nan, device="cuda")
                rc = lib.mmc_pix(mode, apro, epi, av, P, N, K, d["A"].data_ptr(), K, Bt.data_ptr(), ldb, out.data_ptr(), N,
                                 ptr("abias"), ptr("abn"), ptr("ebias"), ptr("ebn"), ptr("eh"), N, ptr("ebb"),
                                 stats.data_ptr() if epi else None, nslot, n_cu, stream)
                assert rc == 0, (rc, mode)
                torch.cuda.synchronize()
                got = out.cpu().numpy().astype(np.float64)
                tag = "%s %s seed %d mode %d" % (PIX_IDS[PIX_CASES.index(case)], name, seed, mode)
                if ref["C"] is None:
                    assert np.isnan(got).all(), tag + ": EPI 4 stores nothing"
                else:
                    err = np.abs(got - ref["C"])
                    u = units(err, ref["T"]) if np.isfinite(got).all() else float("inf")
                    _note((inst, mode, "C"), u)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        at = np.unravel_index(np.nanargmax(np.where(ref["T"] > 0, err / ref["T"], 0)), err.shape)
                    lines.append("%s: C worst %.3f units of 2^-24 T at (pixel, channel) = (%d, %d): got %.9g, want %.9g"
                                 % (tag, u, at[0], at[1], got[at], ref["C"][at]))
                    if not u <= U_B:
                        bad.append(lines[-1])
                if epi:
                    s = stats.cpu().numpy().astype(np.float64)
                    assert np.isnan(s[:, nslot:]).all(), tag + ": a slot beyond nslot was written"
                    for j, (what, summand) in enumerate(ref["sums"]):
                        tot = s[j * N:(j + 1) * N, :nslot].sum(axis=1)
                        us = units(tot - summand.sum(axis=0), np.abs(summand).sum(axis=0)) if np.isfinite(tot).all() else float("inf")
                        _note((inst, mode, "sums P=%d" % P), us)
                        lines.append("%s: %s worst %.3f units of 2^-24 sum |summand| (U_S %d)" % (tag, what, us, U_S[P]))
                        if not us <= U_S[P]:
                            bad.append(lines[-1])
                    assert np.isnan(s[len(ref["sums"]) * N:]).all(), tag + ": rows of the sums buffer that are not this epilogue's were written"
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def _expected_chunks(npix, M, N):
    """mm_kpix_launch's S where the partial-product buffer, not the CU count, is the limit."""
    ceil = lambda a, b: -(-a // b)      # noqa: E731
    S = min(KPIX_PART_CAP // (M * N), max(1, npix // 128))      # what fits; chunks of at least 128 pixels
    chunk = ceil(ceil(npix, S), 32) * 32
    return ceil(npix, chunk)


@pytest.mark.parametrize("case", KPIX_CASES, ids=KPIX_IDS)
def test_k_mm_kpix_every_mode_within_the_fp32_bound(case):
    torch, n_cu, stream = _gpu()
    lib = _lib()
    npix, M, N = case
    nan = float("nan")
    tiles = (-(-M // 128)) * (-(-N // 128))
    assert KPIX_PART_CAP // (M * N) <= 2 * n_cu // tiles      # the buffer, not the CU count, limits S
    S_want = _expected_chunks(npix, M, N)
    assert S_want > 1
    lines, bad = [], []
    for name in FAMILIES:
        for seed in SEEDS:
            o = kpix_operands(case, name, seed)
            ref, T = kpix_reference(o)
            d = {k: torch.from_numpy(v).cuda() for k, v in o.items()}
            for mode in MODES:
                part = torch.full((KPIX_PART_CAP + 64,), nan, device="cuda")
                S = lib.mmc_kpix(mode, npix, M, N, d["A"].data_ptr(), M, d["B"].data_ptr(), N, d["abias"].data_ptr(), d["abn"].data_ptr(),
                                 part.data_ptr(), KPIX_PART_CAP, n_cu, stream)
                torch.cuda.synchronize()
                tag = "%s %s seed %d mode %d" % (KPIX_IDS[KPIX_CASES.index(case)], name, seed, mode)
                assert S == S_want, (tag, S, S_want)
                p = part.cpu().numpy().astype(np.float64)
                assert np.isnan(p[S * M * N:]).all(), tag + ": written beyond the S partial products"
                got = p[:S * M * N].reshape(S, M, N).sum(axis=0)
                u = units(got - ref, T) if np.isfinite(got).all() else float("inf")
                _note(("kpix<2,2,2,1,4,4>", mode, "sum of parts"), u)
                lines.append("%s: S = %d, worst %.3f units of 2^-24 T" % (tag, S, u))
                if not u <= U_B:
                    bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_zz_measured_distances_of_this_run():
    """Prints, per instantiation and mode, the worst distance the tests above saw (nothing to assert beyond what they did)."""
    print("\nunits of 2^-24 T (C, sum of parts; bound U_B = %d) resp. of 2^-24 sum |summand| (sums; bound U_S = %s)" % (U_B, U_S))
    for key in sorted(WORST):
        print("MM_UNITS %-18s mode %d %-22s %.3f" % (key[0], key[1], key[2], WORST[key]))
    assert all(np.isfinite(v) for v in WORST.values())
