"""CPU tier: per-patch conditioning, host side.  ``nf_cond_rows`` against the oracle's own scalar functions for every conditional
layer kind, both directions; its error reporting; and the Python surface's length handling (one value per call, one per patch,
anything else).  No device is touched: ``nf_cond_rows`` is host arithmetic, like ``nf_fold_params``."""
import ctypes as C

import numpy as np
import pytest

from conftest import trained_like_variables
from oracle import nf_oracle as O

ISOS = (100, 400, 800, 1600, 3200, 250)   # 250: not in the tables (sdn5 / sdn4 / sdn6: gain parameter 0; Ex1-Ex3: the ISO-800 entry)
CAMS = (0, 1, 2, 3, 4)
HW = (6, 5)                               # GAIN2's log-det carries H*W*4: a shape with H != W


def cond_variables(arch, width, seed=0):
    """trained_like_variables with the conditional layers' parameters moved off their initial values, so that no two
    (ISO, camera) pairs give the same scalars (a fresh model has cam_params = 1 for every camera and one value for every ISO)."""
    v = trained_like_variables(arch, width, seed=seed)
    rng = np.random.RandomState(seed + 77)
    for k in sorted(v):
        a = v[k]
        if k.endswith("sdn_gain/cam_params"):
            v[k] = (a + 0.1 * rng.randn(*a.shape)).astype(np.float32)
        elif k.endswith("sdn_gain/gain_params") or k.endswith("sdn_gain/beta1") or k.endswith("sdn_gain/beta2"):
            v[k] = (a + 0.3 * rng.randn(*a.shape)).astype(np.float32)
        elif k in ("model/b1", "model/b2", "model/g2"):
            v[k] = (a + 0.2 * rng.randn(*a.shape)).astype(np.float32)
        elif k == "model/g1":    # gain: sigmoid(g1); gain1: exp(1e-5 g1)
            v[k] = (a + (0.2 if abs(float(a.reshape(-1)[0])) < 100 else 2e4) * rng.randn(*a.shape)).astype(np.float32)
        elif "gain_param_" in k:   # sdn1: exp(1e-2 .), sdn2 / sdn3 / gain2: exp(1e-1 .), gain3: exp(1e-5 .)
            s = 3e4 if abs(float(a.reshape(-1)[0])) > 1e4 else 3.0
            v[k] = (a + s * rng.randn(*a.shape)).astype(np.float32)
    return v


def rows_of(arch, variables, width, direction, conds, hw=HW):
    """nf_cond_rows through ctypes → (return code, COND_ROW_DTYPE[n])."""
    from noise_flow_amd import _lib, params
    from noise_flow_amd.noise_flow_model import COND_ROW_DTYPE
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, 0)
    conds = np.ascontiguousarray(conds, np.float32).reshape(-1, 4)
    rows = np.zeros(conds.shape[0], COND_ROW_DTYPE)
    rc = lib.nf_cond_rows(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, direction,
                          C.cast(conds.ctypes.data, C.POINTER(_lib.nf_cond)), conds.shape[0],
                          C.cast(rows.ctypes.data, C.POINTER(_lib.nf_cond_row)))
    return rc, rows


def oracle_scalars(L, iso, cam):
    """fp64 (a, b) with scale^2 = a*y + b for an SDN kind, (scale, None) for a gain kind, from the oracle's own functions."""
    t, p = L["type"], L.get("p")
    if t == "sdn5":
        b1, b2, gain = O.sdn_ex5_scalars(p, iso, cam)
        return b1 / gain, b2
    if t.startswith("gain"):
        return (O.gain_plain_scale(p, iso, np.float64) if t == "gain" else O.gain_ex123_scale(p, iso, t, np.float64)), None
    y = np.array([0.0, 1.0])
    if t == "sdn4":
        s = O.sdn_ex4_scale(y, p, iso)
    elif t == "sdn":
        s = O.sdn_plain_scale(y, p)
    elif t == "sdn6":
        s = O.sdn_ex6_scale(y, p, iso, cam)
    else:
        s = O.sdn_ex123_scale(y, p, iso, t)
    return s[1] ** 2 - s[0] ** 2, s[0] ** 2


def assert_fp32_of(got, want64, what):
    """`got` is the fp32 rounding of the fp64 value: within half an fp32 ulp (2^-24 relative) of it.  The slack of 1e-4 of that
    half-ulp (6e-12 relative) is for the oracle forming the value in another fp64 order: a = scale(1)^2 - scale(0)^2 for the kinds
    whose oracle function returns the scale, i.e. a few 1e-16 x b / a <= 1e3 = a few 1e-13 relative."""
    assert abs(float(got) - want64) <= 2.0 ** -24 * abs(want64) * (1 + 1e-4) + 1e-45, (what, float(got), want64)


ARCHS = ["sdn5|unc", "sdn4|unc", "sdn|unc", "sdn1|unc", "sdn2|unc", "sdn3|unc", "sdn6|unc", "gain|unc", "gain1|unc", "gain2|unc",
         "gain3|unc", "sdn5|unc|gain|unc|sdn3", "gain2|unc|sdn6"]


@pytest.mark.parametrize("arch", ARCHS)
def test_cond_rows_match_the_oracle_scalars(arch):
    v = cond_variables(arch, 4, seed=3)
    cond_layers = [L for L in O.bind_variables(arch, v) if L["type"] not in ("conv1x1", "coupling", "gain4")]
    conds = np.array([(iso, cam, 0.0, 0.0) for iso in ISOS for cam in CAMS], np.float32)
    for direction in (0, 1):
        rc, rows = rows_of(arch, v, 4, direction, conds)
        assert rc == 0
        order = cond_layers   # a slot belongs to a LAYER (model order); the sampling program meets the slots in reverse
        for k, (iso, cam, _, _) in enumerate(conds):
            want_ld = 0.0
            for slot, L in enumerate(order):
                a, b = oracle_scalars(L, float(iso), float(cam))
                what = (arch, direction, float(iso), float(cam), L["type"])
                if b is None:   # gain kinds: z *= a, already 1 / scale in the NLL direction
                    assert a > 0
                    assert_fp32_of(rows["a"][k, slot], 1.0 / a if direction == 0 else a, what)
                    if direction == 0:
                        want_ld -= (HW[0] * HW[1] * 4 if L["type"] == "gain2" else 1) * np.log(a)
                else:
                    assert_fp32_of(rows["a"][k, slot], a, what)
                    assert_fp32_of(rows["b"][k, slot], b, what)
            for slot in range(len(order), 4):   # unused slots
                assert rows["a"][k, slot] == 0.0 and rows["b"][k, slot] == 1.0
            assert abs(rows["ld"][k] - want_ld) <= 1e-12 * max(1.0, abs(want_ld)), (arch, direction, rows["ld"][k], want_ld)
            assert rows["reserved"][k] == 0.0
    # the parameters were moved so that the conditions are told apart: no two rows with different scalars' inputs coincide
    # (over the five table ISOs: at an ISO outside the table sdn6's only camera term is multiplied by a gain parameter of 0)
    conds = conds[:25]
    rc, rows = rows_of(arch, v, 4, 0, conds)
    uses_cam = any(L["type"] in ("sdn5", "sdn6") for L in cond_layers)
    uses_iso = any(L["type"] != "sdn" for L in cond_layers)
    keys = {(float(i) if uses_iso else 0.0, float(c) if uses_cam else 0.0) for i, c, _, _ in conds}
    assert len({r.tobytes() for r in rows}) == len(keys), arch


def test_cond_rows_bad_inputs():
    from noise_flow_amd import _lib
    lib = _lib.load()
    arch = "sdn5|unc|gain|unc|sdn3"
    v = cond_variables(arch, 4, seed=3)
    conds = np.array([(100, 0, 0, 0), (400, 1, 0, 0), (800, 2, 0, 0), (1600, 7, 0, 0), (3200, 4, 0, 0)], np.float32)
    rc, _ = rows_of(arch, v, 4, 0, conds)
    assert rc == _lib.NF_ECOND
    msg = lib.nf_last_error().decode()
    assert "3" in msg and "camera" in msg, msg
    rc, _ = rows_of(arch, v, 4, 1, conds[:3])
    assert rc == 0
    rc, rows = rows_of(arch, v, 4, 0, conds[:0])      # n = 0
    assert rc == 0 and rows.shape == (0,)
    rc, _ = rows_of(arch, v, 4, 2, conds[:3])         # direction
    assert rc == _lib.NF_EINVAL
    # a non-positive gain scale: sigmoid(g1) * iso + sigmoid(g2) <= 0 at a negative ISO
    rc, _ = rows_of(arch, v, 4, 0, np.array([(100, 0, 0, 0), (-1e6, 0, 0, 0)], np.float32))
    assert rc == _lib.NF_EINVAL
    assert "1" in lib.nf_last_error().decode()


def test_row_layout_is_the_header_struct():
    from noise_flow_amd import _lib
    from noise_flow_amd.noise_flow_model import COND_ROW_DTYPE
    assert C.sizeof(_lib.nf_cond_row) == 48 == COND_ROW_DTYPE.itemsize
    for name in ("a", "b", "ld", "reserved"):
        assert getattr(_lib.nf_cond_row, name).offset == COND_ROW_DTYPE.fields[name][1]


def test_python_length_handling():
    """One value per call (scalar or length 1) → None = today's path; one per patch → a table; anything else → ValueError."""
    import torch
    from noise_flow_amd.noise_flow_model import PatchCond, patch_cond
    B = 6
    assert patch_cond(None, None, 100.0, [2.0], B) is None
    assert patch_cond([0.0], [0.0], [100.0], np.array([2.0]), B) is None
    assert patch_cond([0.0], [0.0], torch.tensor([100.0]), torch.tensor(2.0), B) is None
    assert patch_cond([0.0], [0.0], [100.0], [2.0], 1) is None            # B = 1: length 1 is per call
    iso = [100, 400, 800, 1600, 3200, 250]
    for isos in (iso, np.asarray(iso, np.int64), torch.tensor(iso), [iso]):   # the wrapper hands [list] through
        pc = patch_cond(None, [0.5], isos, [3.0], B)                           # length-1 arguments are broadcast
        assert isinstance(pc, PatchCond) and pc.table.dtype == np.float32 and pc.table.shape == (B, 4)
        np.testing.assert_array_equal(pc.table[:, 0], iso)
        np.testing.assert_array_equal(pc.table[:, 1], 3.0)
        np.testing.assert_array_equal(pc.table[:, 2], 0.0)
        np.testing.assert_array_equal(pc.table[:, 3], 0.5)
    pc = patch_cond(None, None, iso, [0, 1, 2, 3, 4, 0], B)
    np.testing.assert_array_equal(pc.table[:, 1], [0, 1, 2, 3, 4, 0])
    for bad in ([100, 400], iso + [100], iso[:5]):
        with pytest.raises(ValueError):
            patch_cond(None, None, bad, [2.0], B)
    with pytest.raises(ValueError):
        patch_cond(None, None, [100.0], [0, 1], B)
    with pytest.raises(ValueError, match="is_training"):
        patch_cond(None, None, iso, [2.0], B, is_training=True)
    assert patch_cond(None, None, [100.0], [2.0], B, is_training=True) is None   # per call: batch statistics as before


def test_rows_are_gathered_from_the_distinct_conditions():
    """PatchCond.rows runs nf_cond_rows on the distinct tuples only and gathers: row b is the row of patch b's tuple."""
    from noise_flow_amd import _lib, params
    from noise_flow_amd.noise_flow_model import FlowHandle, patch_cond
    arch = "sdn5|unc|gain|unc|sdn3"
    v = cond_variables(arch, 4, seed=3)
    layers, descs, flat = params.pack(arch, v, 4, "loss_first")
    calls = []

    class Flow(FlowHandle):            # the handle's host half: no nf_create, so no device
        def __init__(self):
            self.lib = _lib.load()
            self._model_args = (_lib.nf_config(HW[0], HW[1], 4, len(layers), -1, 0), descs, flat)

        def cond_rows(self, direction, conds):
            calls.append(np.array(conds))
            return FlowHandle.cond_rows(self, direction, conds)

    B = 23
    iso = [ISOS[b % 5] for b in range(B)]
    cam = [CAMS[(b // 2) % 3] for b in range(B)]
    pc = patch_cond(None, None, iso, cam, B)
    for direction in (0, 1):
        got = pc.rows(Flow(), direction)
        rc, want = rows_of(arch, v, 4, direction, pc.table)
        assert rc == 0 and got.tobytes() == want.tobytes()
    assert all(len(c) == len({tuple(r) for r in pc.table}) < B for c in calls)
