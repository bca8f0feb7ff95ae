"""Dyadic probes on every fp16-CNN kernel family: bit for bit on the shift half, tail round-off only on the raw half.

The probe models, the two input families (`exact`, `rounding`), the fp64 chain and the case table with the seams each kernel has
at each shape are those of tests/fp16_probe.py (CASES names the seams and the source lines they were read from); the conditions
that make the assertions below meaningful — exact accumulations, real roundings, the library's fold landing on the design, the
oracle's flavours agreeing to the bit, the mutants every patch would show — are asserted on the CPU by
tests/test_fp16_exact_probe_cpu.py.  Every case asserts nf_kernel_path in both directions and, where a variant is forced
(NF_H16=4x4, NF_GEMM16=a; set while the handle is created), that the switch was read: the forced layout's block differs from
the default one (nf_fold_layout under the same environment — nf_kernel_path does not tell the variants apart).

Shift probe, both directions (`inverse`, `forward` = sampling with the supplied eps): where bit equality is claimed (the whole
`exact` family; in `rounding` the elements of fp16_probe.l_last_exact_mask) the output equals the fp64 chain rounded once to fp32
— compared as uint32, every element, every patch — elsewhere it is within BOUND_U[width] * 2^-24 * A; the pass-through half is
bit-identical and the per-patch log-det exactly 0.0.
Raw probe: log(out) = +-ls within one unit of 2^-24 A (1 + BOUND_U where l_last is not exact) mapped through tanh plus
RAW_T * 2^-24 * (1 + |ls|); the per-patch log-det within the sum of its elements' allowances plus GRAD_NOISE_C * 2^-24 * sum |ls|
(a lost or double-counted pixel moves it by |ls| of that pixel, >= 0.05 on at least half of them).

What these probes cannot see: the sdn / gain layers and the 1x1 mix (the model has none but the identity), near-ties of generic
inputs (tests/test_gpu_parity.py, test_gpu_wide.py, test_gpu_gemm.py hold those to 2e-3 of scale) and half denormals (no half
operand of the design is subnormal).

Measured on an MI355X: profiles/r16_fp16_exact_probe.txt.
"""
import ctypes as C

import numpy as np
import pytest

import fp16_probe as P
from conftest import GRAD_NOISE_C
from test_fp16_exact_probe_cpu import BOUND_U, _bits, _data, raw_reference
from test_gpu_split_bf16_probe import U24

pytestmark = pytest.mark.gpu

_ARGS = ([0.0], [0.0], [100], [0])
SWITCHES = ("NF_H16", "NF_GEMM16")


def _layout_block(case, v, path):
    """The kernel path's parameter block as nf_fold_layout builds it under the current environment (host only)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    _, _, width, (H, W) = case[:4]
    layers, descs, flat = params.pack("unc", v, width, "loss_first", 1, "LU")
    cfg = _lib.nf_config(H, W, 4, len(layers), -1, _lib.NF_CFG_FP16_CNN)
    ops = (C.c_int32 * 16)()
    n_ops, lw, nf = C.c_int32(), C.c_int32(), C.c_size_t()
    args = (C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, 0, path, ops, 8, C.byref(n_ops), C.byref(lw))
    _lib.check(lib.nf_fold_layout(*args, None, 0, C.byref(nf)))
    blk = np.zeros(nf.value, np.float32)
    _lib.check(lib.nf_fold_layout(*args, blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size, C.byref(nf)))
    return blk.view(np.uint32)


def _model(case, v, monkeypatch):
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    _, path, width, (H, W), env = case[:5]
    want = getattr(_lib, "NF_PATH_" + path)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if env:
        plain = _layout_block(case, v, want)
        monkeypatch.setenv(*env)
        assert not np.array_equal(_layout_block(case, v, want), plain), (case[0], "%s=%s was not read" % env)
    m = NoiseFlow([H, W, 4], False, default_hps(arch="unc", width=width), variables=v, cnn_dtype="fp16")
    for direction in (0, 1):
        assert m._flow.lib.nf_kernel_path(m._flow.ptr, direction) == want, (case[0], direction)
    return m


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_shift_probe_bit_for_bit_with_the_fp64_chain(case, seed, monkeypatch):
    """Measured on an MI355X (profiles/r16_fp16_exact_probe.txt, per case): 0 unequal bits in 8.2 M bit-exact element comparisons
    over the 25 cases x 2 families x 2 seeds x 2 directions, every log-det exactly 0.0; the bounded elements of `rounding` at most
    0.046 units of 2^-24 A (width 96 at 33x31, bound 0.092) — what the one rounding of the result to fp32 costs, as on the CPU."""
    width = case[2]
    m = _model(case, P.variables(P.design(width, seed), "shift"), monkeypatch)
    lines, bad = [], []
    for name in P.FAMILIES:
        d = _data(case[0], name, seed)
        x = P.probe_x(d["D"], name, "shift", d["z0"])
        z1 = x[..., 2:].astype(np.float64)
        z, obj = m.inverse(x, None, None, *_ARGS)
        xs = m.forward(x, None, None, *_ARGS)
        mask, A = d["mask"], d["A"] + np.abs(z1)
        for tag, out, want in (("inverse", z, z1 + d["shift"]), ("forward", xs, z1 - d["shift"])):
            out = np.asarray(out)
            assert np.array_equal(_bits(out[..., :2]), _bits(d["z0"])), (name, tag, "the pass-through half changed")
            neq = (_bits(out[..., 2:]) != _bits(want)) & mask
            patches = np.flatnonzero(neq.reshape(neq.shape[0], -1).any(axis=1)).tolist()
            u = np.where(mask, 0.0, np.abs(out[..., 2:].astype(np.float64) - want) / (U24 * A))
            at = tuple(int(i) for i in np.unravel_index(np.argmax(u), u.shape))
            lines.append("FP16PROBE shift %s %s %s seed %d: %d unequal of %d bit-exact elements (patches %s); %d bounded elements, worst "
                         "%.4f units of 2^-24 A (bound %g) at %s" % (case[0], name, tag, seed, int(neq.sum()), int(mask.sum()), patches,
                                                                      int((~mask).sum()), u.max(), BOUND_U[width], at))
            if neq.any() or not u.max() <= BOUND_U[width]:
                bad.append(lines[-1])
                if neq.any():
                    i = tuple(int(k) for k in np.argwhere(neq)[0])
                    bad.append("    first at (patch, row, col, ch) = %s: kernel %r, chain %r" % (i, float(out[..., 2:][i]), float(want[i])))
        ld = np.asarray(obj)
        lines.append("FP16PROBE shift %s %s log-det seed %d: max |log-det| %g" % (case[0], name, seed, np.abs(ld).max()))
        if not np.all(ld == 0.0):
            bad.append(lines[-1] + " — ls = 0 exactly: the log-det must be zero")
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_raw_probe_log_scale_and_log_det(case, seed, monkeypatch):
    """Measured on an MI355X (profiles/r16_fp16_exact_probe.txt, per case): per element at most 0.27 of the bound (width 4 at
    64x64, `exact`), the log-det at most 0.35 of its allowance (width 24 at 9x33)."""
    width = case[2]
    m = _model(case, P.variables(P.design(width, seed), "raw"), monkeypatch)
    lines, bad = [], []
    for name in P.FAMILIES:
        d = _data(case[0], name, seed)
        ls, bound, conv = raw_reference(d)
        x = P.probe_x(d["D"], name, "raw", d["z0"])
        z, obj = m.inverse(x, None, None, *_ARGS)
        xs = m.forward(x, None, None, *_ARGS)
        for tag, out, want in (("inverse", z, ls), ("forward", xs, -ls)):
            out = np.asarray(out)
            assert np.array_equal(_bits(out[..., :2]), _bits(d["z0"])), (name, tag, "the pass-through half changed")
            r = np.abs(np.log(out[..., 2:].astype(np.float64)) - want) / bound
            at = tuple(int(i) for i in np.unravel_index(np.argmax(r), r.shape))
            lines.append("FP16PROBE raw %s %s %s seed %d: worst %.3f of the bound at %s" % (case[0], name, tag, seed, r.max(), at))
            if not r.max() <= 1.0:
                bad.append(lines[-1])
        ld_ref = ls.sum(axis=(1, 2, 3))
        ld_tol = conv.sum(axis=(1, 2, 3)) + GRAD_NOISE_C * U24 * np.abs(ls).sum(axis=(1, 2, 3))
        ld_err = np.abs(np.asarray(obj, np.float64) - ld_ref)
        lines.append("FP16PROBE raw %s %s log-det seed %d: worst %.3f of its allowance" % (case[0], name, seed, (ld_err / ld_tol).max()))
        if not np.all(ld_err <= ld_tol):
            bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
