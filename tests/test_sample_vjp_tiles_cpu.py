"""CPU tier of the tiled sampling VJP (NF_CFG_SVJP_TILED, csrc/nf_sample_grad.hip TILED): the flag and what ``nf_sample_vjp_supported``
accepts and refuses with it, the plan it shares with ``nf_nll_grad``, and the arithmetic the design rests on, pinned with
``SampleVjpRef`` and the tile arithmetic of ``nf_tile_plan``:

  * a sampling-VJP tile evaluated alone is exact 4 x (couplings) pixels inside every tile border that is not an image border, and one
    pixel less is not (fp64);
  * the call sequence of ``sample_vjp_tiled`` (csrc/nf_host.hip) written out on the reference — tensors kept between two segments,
    the cotangent handed from segment to segment through two tensors, core stores, gy stored by the first segment with an sdn-kind layer
    and added to by later ones, gtemp as per-tile core sums added in tile order — is whole-image autograd in fp64, meets the rule of
    tests/sample_vjp_ref.py in the reversible float32 flavour, and its mutants stand above the bound.

No device is touched.

Measured on the CPU (reversible float32 walk, worst share of the bound max(1e-5, 4 e32) over patches, tensors and both norms):
vocabulary model 70x36, 2 segments 0.03; shipped model 65x64 at 8 / 4 / 3 segments 0.22 / 0.24 / 0.27.  Mutants in fp64 (x the bound):
halo 3 in one-coupling segments 5.8e2 (geps), second segment's gy not added 1e5 (gy), gtemp over whole tiles 8.1e2 (gtemp).
"""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import FULL_ARCH, trained_like_variables
from sample_vjp_ref import (ISO, CAM, SHIPPED_TEMP, WIDE_ARCH, SampleVjpRef, backward_sweep, case_inputs, case_model,
                            compare_with_kink_rule, distances, reference_conditions, rule_weights, sampling_variables)
from test_sample_vjp_rule_cpu import MUTANT_FACTOR, _supported

TILE = 32           # csrc/nf_device.h, NF_GRAD_TILE
CPL = (2, 3)        # NF_OP_COUPLING_FWD / _REV


def _flag():
    from noise_flow_amd import _lib
    return _lib.NF_CFG_SVJP_TILED


def _wide_vars(width):
    return trained_like_variables(WIDE_ARCH, 4) if width == 4 else sampling_variables(WIDE_ARCH, width)


# the new ground: (arch, width, (H, W))
NEW_GROUND = [(FULL_ARCH, 4, (65, 64)), (FULL_ARCH, 4, (64, 65)), (FULL_ARCH, 4, (96, 80)), (FULL_ARCH, 4, (4096, 33)),
              (WIDE_ARCH, 8, (64, 64)), (WIDE_ARCH, 8, (56, 56)), (WIDE_ARCH, 16, (40, 33)), (WIDE_ARCH, 4, (70, 20))]


def _model(arch, width, shipped_variables):
    return shipped_variables if arch == FULL_ARCH else _wide_vars(width)


# ---- the flag and the supported set -------------------------------------------------------------------------------------------
def test_flag_is_a_new_bit_and_bit_8_stays_unknown():
    from noise_flow_amd import _lib
    assert _flag() == 512
    assert _lib.NF_SVJP_PATH_TILED == 2
    for hw in ((16, 16), (96, 80)):
        for flags in (8, 8 | 512):
            rc, msg = _supported(WIDE_ARCH, _wide_vars(8), 8, hw, flags)
            assert rc == _lib.NF_EINVAL and "unknown bits" in msg, msg


@pytest.mark.parametrize("arch,width,hw", NEW_GROUND)
def test_supported_with_the_flag(shipped_variables, arch, width, hw):
    """The test that fails without the feature: 512 is an unknown bit there."""
    rc, msg = _supported(arch, _model(arch, width, shipped_variables), width, hw, _flag())
    assert rc == 0, msg


@pytest.mark.parametrize("arch,width,hw", NEW_GROUND)
def test_refused_without_the_flag_as_before(shipped_variables, arch, width, hw):
    from noise_flow_amd import _lib
    v = _model(arch, width, shipped_variables)
    rc, msg = _supported(arch, v, width, hw, 0)
    assert rc == _lib.NF_EINVAL and msg.startswith("nf_sample_vjp"), msg
    rc, msg = _supported(arch, v, width, hw, _lib.NF_CFG_GRAD_TILED)
    assert rc == _lib.NF_EINVAL and msg.startswith("nf_sample_vjp") and "no tile mode" in msg, msg


def test_shapes_held_whole_resolve_as_before(shipped_variables):
    from noise_flow_amd import _lib
    for hw in ((32, 32), (9, 13), (64, 64), (1, 1), (64, 37)):
        rc, msg = _supported(FULL_ARCH, shipped_variables, 4, hw, _flag())
        assert rc == 0, (hw, msg)
    for width, hw in ((8, (16, 16)), (8, (48, 48)), (16, (32, 32))):
        rc, msg = _supported(WIDE_ARCH, _wide_vars(width), width, hw, _flag())
        assert rc == 0, (width, hw, msg)
    # the whole-patch limit of width 8 stays where grad_support holds the shape whole
    v = sampling_variables("unc", 8)
    for flags in (0, _flag()):
        rc, msg = _supported("unc", v, 8, (58, 58), flags)
        assert rc == _lib.NF_EINVAL and "3072 pixels" in msg, (flags, msg)


def test_refusals_with_the_flag(shipped_variables):
    from noise_flow_amd import _lib
    E = _lib.NF_EINVAL
    v32, v64 = sampling_variables(WIDE_ARCH, 32), sampling_variables(WIDE_ARCH, 64)
    rc, msg = _supported(FULL_ARCH, shipped_variables, 4, (65, 64), _flag() | _lib.NF_CFG_FP16_CNN)
    assert rc == E and msg.startswith("nf_sample_vjp") and "fp32 handles only" in msg, msg
    for extra in (0, _lib.NF_CFG_SVJP_MFMA | _lib.NF_CFG_GRAD_TILED_WIDE):
        rc, msg = _supported(WIDE_ARCH, v32, 32, (65, 64), _flag() | extra)
        assert rc == E and msg.startswith("nf_sample_vjp") and "coupling widths up to 16" in msg and "no tile mode" in msg, msg
        rc, today = _supported(WIDE_ARCH, v32, 32, (65, 64), _lib.NF_CFG_GRAD_TILED | extra)       # its present words, kept
        assert rc == E and msg.startswith(today), (today, msg)
    for extra in (0, _lib.NF_CFG_GRAD_GEMM, _lib.NF_CFG_GRAD_TILED_GEMM):
        rc, msg = _supported(WIDE_ARCH, v64, 64, (65, 64), _flag() | extra)
        rc0, today = _supported(WIDE_ARCH, v64, 64, (65, 64), _lib.NF_CFG_GRAD_TILED | extra)
        assert rc == E and rc0 == E and msg.startswith(today), (today, msg)
    rc, msg = _supported(WIDE_ARCH, v64, 64, (16, 16), _flag())
    assert rc == E and "coupling widths up to 32" in msg, msg


# ---- the plan is nf_nll_grad's ----------------------------------------------------------------------------------------------------
def _plan(arch, variables, width, hw, flags):
    """(return code of nf_grad_tile_segments, its rows, the op types of the NLL-order program)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, flags)
    fp = flat.ctypes.data_as(C.POINTER(C.c_float))
    out = (C.c_int32 * 80)()
    n = lib.nf_grad_tile_segments(C.byref(cfg), descs, fp, flat.size, out, 16)
    ops = (C.c_int32 * 128)()
    n_ops = C.c_int32()
    cfg0 = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, 0)
    assert lib.nf_fold_params(C.byref(cfg0), descs, fp, flat.size, 0, ops, 64, C.byref(n_ops), None, 0, None, None) == 0
    return n, [tuple(out[5 * i:5 * i + 5]) for i in range(max(n, 0))], [ops[2 * i] for i in range(n_ops.value)]


@pytest.mark.parametrize("forced", [None, 8, 4, 3])
def test_plan_with_the_flag_is_the_gradient_plan(monkeypatch, shipped_variables, forced):
    from noise_flow_amd import _lib
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    if forced:
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    for hw in ((96, 80), (65, 64)):
        a = _plan(FULL_ARCH, shipped_variables, 4, hw, _flag())
        b = _plan(FULL_ARCH, shipped_variables, 4, hw, _lib.NF_CFG_GRAD_TILED)
        assert a[0] == b[0] >= 1 and a[1] == b[1], (a, b)
        assert not forced or a[0] == forced


def test_infeasible_forced_count_fails(monkeypatch, shipped_variables):
    from noise_flow_amd import _lib
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", "2")
    assert _plan(FULL_ARCH, shipped_variables, 4, (96, 80), _flag())[0] == _lib.NF_EINVAL
    rc, msg = _supported(FULL_ARCH, shipped_variables, 4, (96, 80), _flag())
    assert rc == _lib.NF_EINVAL and "segments" in msg, msg


# ---- tile arithmetic ------------------------------------------------------------------------------------------------------------------
def _axis(size, tile, halo):
    """nf_tile_plan of one axis → [(origin, core0, core1)]."""
    from noise_flow_amd import _lib
    lib = _lib.load()
    o, a, b = ((C.c_int32 * 512)() for _ in range(3))
    n = lib.nf_tile_plan(size, min(size, tile), halo, o, a, b, 512)
    assert 0 < n <= 512, (size, halo, n)
    return list(zip(o[:n], a[:n], b[:n]))


def _tiles(H, W, tile, halo):
    """The tiles of an H x W image in tile order (row-major): (oy, ox, th, tw, core rows, core columns)."""
    th, tw = min(H, tile), min(W, tile)
    return [(oy, ox, th, tw, (ay, by), (ax, bx)) for oy, ay, by in _axis(H, tile, halo) for ox, ax, bx in _axis(W, tile, halo)]


# ---- the halo, in fp64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,c", [("sdn5|unc", 1), ("sdn5|unc|unc", 2), (WIDE_ARCH, 3), ("sdn5|unc|sdn3", 1)])
def test_vjp_halo_is_four_per_coupling_in_fp64(arch, c):
    """Every tile evaluated on its own with the cotangent as given, only its core kept: with a halo of 4c the tiled geps (and gy) IS
    the whole image's (<= 1e-13 of max|.|; measured 0), with 4c - 1 geps is not (> 1e-12; measured on these inputs 7.3e-3, 7.1e-5, 6.8e-7, 1.74e-2 with gy 6.1e-3).
    90x70 image, 64-pixel tiles, trained_like_variables(arch, 4, seed=1), temperature 0.6."""
    ref = SampleVjpRef(arch, trained_like_variables(arch, 4, seed=1))
    y, eps, g = (v.astype(np.float64) for v in case_inputs(1, 90, 70, 0))
    _, gy, ge, _ = ref.sample_vjp(y, eps, g, SHIPPED_TEMP, ISO, CAM)
    err = {}
    for halo in (4 * c, 4 * c - 1):
        ty, te = np.full(y.shape, np.nan), np.full(y.shape, np.nan)
        for oy, ox, th, tw, (ay, by), (ax, bx) in _tiles(90, 70, 64, halo):
            cut = lambda v: np.ascontiguousarray(v[:, oy:oy + th, ox:ox + tw])   # noqa: E731
            _, a, b, _ = ref.sample_vjp(cut(y), cut(eps), cut(g), SHIPPED_TEMP, ISO, CAM)
            ty[:, ay:by, ax:bx] = a[:, ay - oy:by - oy, ax - ox:bx - ox]
            te[:, ay:by, ax:bx] = b[:, ay - oy:by - oy, ax - ox:bx - ox]
        err[halo] = (np.abs(te - ge).max() / np.abs(ge).max(), np.abs(ty - gy).max() / np.abs(gy).max())
        print("couplings %d halo %2d: geps %.2e gy %.2e" % (c, halo, err[halo][0], err[halo][1]))
    assert max(err[4 * c]) <= 1e-13
    assert err[4 * c - 1][0] > 1e-12


# ---- the walk: tile by tile, segment by segment -----------------------------------------------------------------------------------------
def _segment_layers(ref, segs, types):
    """The plan's segments (ops of the NLL-order program) as layer ranges of the reference: by couplings — the program folds some
    layers into their neighbours, and a segment ends right behind its last coupling (the last one at the end)."""
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    out, l0, c0 = [], 0, 0
    for i, (op0, op1, halo, _, _) in enumerate(segs):
        n = sum(1 for t in types[op0:op1] if t in CPL)
        assert halo == 4 * n
        l1 = len(ref.layers) if i == len(segs) - 1 else cpl[c0 + n - 1] + 1
        out.append((l0, l1, halo))
        l0, c0 = l1, c0 + n
    assert c0 == len(cpl)
    return out


def _sub(ref, l0, l1):
    s = copy.copy(ref)
    s.layers = ref.layers[l0:l1]
    s._smemo, s._memo = {}, {}
    return s


def tiled_walk(ref, seg_layers, y, eps, g, temp, iso, cam, dtype, reversible, halo_short=0, skip_gy_of=None, gtemp_whole_tiles=False):
    """``sample_vjp_tiled`` on the reference → (gy or None, geps, gtemp).  Forward, sampling order: the tensor at every segment
    boundary is kept (whole images: the tiled forward launches are nf_sample's).  Backward, NLL order: every tile of a segment
    starts from the tensor kept behind it (the last segment from eps, scaled by temp), takes the cotangent the segment in front of it
    stored (the first one g) and stores its core; gy is stored by the first segment that has an sdn-kind layer and added to by later
    ones; the last segment leaves one sum of g eps per tile, over its core, and those are added per image in tile order.
    Mutants: halo_short (a one-coupling segment's halo that many pixels short), skip_gy_of (that segment's gy is not added),
    gtemp_whole_tiles (the sums run over whole tiles)."""
    B, H, W, _ = eps.shape
    S = len(seg_layers)
    subs = [_sub(ref, l0, l1) for l0, l1, _ in seg_layers]
    keep = []   # (the sweeps memoise by id: every array handed to one stays alive)
    zero = np.zeros_like(eps)
    kept = [None] * (S + 1)      # kept[s]: the tensor in front of NLL segment s; kept[S] stands for eps
    cur = eps
    for s in range(S - 1, 0, -1):
        cur = backward_sweep(subs[s], y, cur, zero, temp if s == S - 1 else 1.0, iso, cam, dtype, reversible=reversible)[0]
        cur = cur.astype(np.float32) if dtype == np.float32 else cur
        kept[s] = cur
    gcur = g
    gy = None
    gtemp = np.zeros(B, np.float64)
    for s in range(S):
        halo = seg_layers[s][2]
        if halo == 4:
            halo -= halo_short
        last = s == S - 1
        src, tmp = (eps, temp) if last else (kept[s + 1], 1.0)
        nxt = np.full(eps.shape, np.nan, np.float64)
        part = np.full(eps.shape, np.nan, np.float64)
        has_sdn = subs[s].has_sdn() and y is not None
        sums = []
        for oy, ox, th, tw, (ay, by), (ax, bx) in _tiles(H, W, TILE, halo):
            cut = lambda v: None if v is None else np.ascontiguousarray(v[:, oy:oy + th, ox:ox + tw])   # noqa: E731
            ins = (cut(y), cut(src), cut(gcur))
            keep.append(ins)
            _, tgy, tg, _ = backward_sweep(subs[s], ins[0], ins[1], ins[2], tmp, iso, cam, dtype, reversible=reversible)
            core = (slice(None), slice(ay - oy, by - oy), slice(ax - ox, bx - ox))
            nxt[:, ay:by, ax:bx] = tg[core]
            if has_sdn:
                part[:, ay:by, ax:bx] = tgy[core]
            if last:
                ge = tg / tmp * np.asarray(ins[1], np.float64)
                sums.append((ge if gtemp_whole_tiles else ge[core]).reshape(B, -1).sum(axis=1))
        assert not np.isnan(nxt).any()
        if has_sdn and s != skip_gy_of:
            assert not np.isnan(part).any()
            gy = part if gy is None else gy + part
        if last:
            for t in sums:          # tile order
                gtemp = gtemp + t
        gcur = nxt.astype(np.float32) if dtype == np.float32 else nxt
    if gy is None and y is not None and ref.has_sdn():
        gy = np.zeros(eps.shape, np.float64)
    return gy, np.asarray(gcur, np.float64), gtemp


_WALK = {}


def _walk_case(kind, forced, shipped_variables, monkeypatch):
    """→ (ref, width, y, eps, g, temp, iso, cam, segment layer ranges) of one walk case under a forced plan."""
    key = (kind, forced)
    monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    if key not in _WALK:
        if kind == "vocab":
            arch, v, width, _ = case_model(("vocab", {}), shipped_variables)
            hw, inputs, temp, iso, cam = (70, 36), case_inputs(3, 70, 36, 0), 1.0, 1600.0, 3.0
        else:
            arch, v, width = FULL_ARCH, shipped_variables, 4
            hw, inputs, temp, iso, cam = (65, 64), case_inputs(2, 65, 64, 0), SHIPPED_TEMP, ISO, CAM
        base = _WALK.get((kind, "ref"))
        if base is None:
            base = _WALK[(kind, "ref")] = (SampleVjpRef(arch, v), inputs)
        ref, inputs = base
        n, segs, types = _plan(arch, v, width, hw, _flag())
        assert n == forced, (n, segs)
        _WALK[key] = (ref, width) + inputs + (temp, iso, cam, _segment_layers(ref, segs, types))
    return _WALK[key]


WALKS = [("vocab", 2), ("shipped", 8), ("shipped", 4), ("shipped", 3)]


@pytest.mark.parametrize("kind,forced", WALKS)
def test_walk_is_whole_image_autograd_in_fp64(monkeypatch, shipped_variables, kind, forced):
    ref, width, y, eps, g, temp, iso, cam, seg_layers = _walk_case(kind, forced, shipped_variables, monkeypatch)
    y64, e64, g64 = (v.astype(np.float64) for v in (y, eps, g))
    _, gy, ge, gt = ref.sample_vjp(y64, e64, g64, temp, iso, cam)
    wy, we, wt = tiled_walk(ref, seg_layers, y64, e64, g64, temp, iso, cam, np.float64, reversible=False)
    assert np.abs(we - ge).max() <= 1e-12 * np.abs(ge).max()
    assert np.abs(wy - gy).max() <= 1e-12 * np.abs(gy).max()
    assert np.abs(wt - gt).max() <= 1e-12 * np.abs(ge / temp * e64).reshape(eps.shape[0], -1).sum(axis=1).max()
    if kind == "vocab":
        assert sum(1 for l0, l1, _ in seg_layers if _sub(ref, l0, l1).has_sdn()) == 2      # gy comes from two segments


@pytest.mark.parametrize("kind,forced", WALKS)
def test_reversible_float32_walk_meets_the_rule(monkeypatch, shipped_variables, kind, forced):
    ref, width, y, eps, g, temp, iso, cam, seg_layers = _walk_case(kind, forced, shipped_variables, monkeypatch)
    reference_conditions(ref, width, y, eps, g, temp, iso, cam)
    got = tiled_walk(ref, seg_layers, y, eps, g, temp, iso, cam, np.float32, reversible=True)
    res = compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got, log=print)
    print("worst share of the bound: %.2f" % max(d / max(1e-5, 4.0 * e) for rows in res.values() for d, e in rows))


def _mutant_ratio(ref, y, eps, g, temp, iso, cam, got, tensor):
    """worst patch's distance of an fp64 mutant over the rule's bound, the smaller over the two norms."""
    want = ref.sample_vjp(y, eps, g, temp, iso, cam)
    r32 = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float32)
    w = rule_weights(ref, y, iso, cam, eps.shape)
    e32 = distances(r32[1:], want, y, eps, temp, w)
    d = distances(got, want, y, eps, temp, w)
    names = (tensor, tensor + "/w") if tensor != "gtemp" else (tensor,)
    return min(float((d[k] / np.maximum(1e-5, 4.0 * e32[k])).max()) for k in names)


def test_mutants_stand_above_the_bound(monkeypatch, shipped_variables):
    ref, width, y, eps, g, temp, iso, cam, seg_layers = _walk_case("shipped", 8, shipped_variables, monkeypatch)
    got = tiled_walk(ref, seg_layers, y, eps, g, temp, iso, cam, np.float64, reversible=False, halo_short=1)
    r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, got, "geps")
    print("halo one pixel short in the one-coupling segments: %.3g x the bound" % r)
    assert r >= MUTANT_FACTOR, r
    got = tiled_walk(ref, seg_layers, y, eps, g, temp, iso, cam, np.float64, reversible=False, gtemp_whole_tiles=True)
    r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, got, "gtemp")
    print("gtemp over whole tiles: %.3g x the bound" % r)
    assert r >= MUTANT_FACTOR, r
    ref, width, y, eps, g, temp, iso, cam, seg_layers = _walk_case("vocab", 2, shipped_variables, monkeypatch)
    got = tiled_walk(ref, seg_layers, y, eps, g, temp, iso, cam, np.float64, reversible=False, skip_gy_of=1)
    r = _mutant_ratio(ref, y, eps, g, temp, iso, cam, got, "gy")
    print("second segment's gy not added: %.3g x the bound" % r)
    assert r >= MUTANT_FACTOR, r
