"""CPU tier of the rule for the tiled gradient at coupling width 32 (tests/test_gpu_nll_grad_tiled_wide.py), in the manner of
tests/test_nll_grad_rule_cpu.py: shown on the reference alone, for EVERY accuracy case of that GPU file, that the arithmetic the
tiled path documents stays inside the rule's bound, and that the slips a tiled kernel can make do not.  No device is touched.

``tiled_sweep`` is ``nll_grad_ref.backward_sweep`` (reversible flavour) cut the way csrc/nf_host.hip::grad_tiled cuts a call: the
forward pass keeps the tensor in front of every segment; then, last segment first, every min(H,32) x min(W,32) tile of the plan is
evaluated ON ITS OWN — zero padding at the tile's border, the edge channel of l_last following the IMAGE border, the layers in
front of the segment's first coupling taken forward from the loaded tensor, every other input rebuilt from its output — with g =
the tile's own z (last segment) or the gradient the segment behind it stored, and only the core window is kept: g for the next
segment, gy stored by the first segment (in this order) that has an sdn layer and added to by the others.  The plan (segments,
halo 4 x couplings, tile origins and cores) is the library's own: nf_grad_tile_segments and nf_tile_plan.

Per case:
  * in float64 the tiled sweep is torch.autograd of the whole image (1e-12 of max|grad|);
  * in float32 it stays inside the bound max(1e-5, 4 e32) in both norms (ratios printed with -s);
  * the mutants, each in float64: beyond TWICE the combined bound on at least one element, or listed in DROPPED with the ratio —
      short_halo   the halo one pixel short (3 instead of 4) in every segment of ONE coupling;
      tile_edge    the edge channel (the kernel's index into the E table) taken from the tile border instead of the image border
                   (DROPPED on every case: it cannot reach a core, see the table);
      gy_not_added gy of a later launch not added to what an earlier one stored;
      core_shift   the core window off by one (a tile keeps [core0 + 1, core1 + 1) instead of [core0, core1)).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import FULL_ARCH
import nll_grad_ref as R
import test_gpu_nll_grad_tiled_wide as G
from test_gpu_nll_grad import ISO, CAM, TUPLES5, VOCAB_ARCH, WIDE_ARCH
from test_gpu_nll_grad_wide import VW, _model, _vocab, shipped_sdn_variables
from test_grad_tiles_cpu import _axis
from test_grad_wide_supported_cpu import NO_SDN_ARCH
from test_nll_grad_rule_cpu import _ratios

ROWS3 = np.array([(i, c, 0, 0) for i, c in TUPLES5[:3]], np.float32)


def _specs():
    """(label, model, arch, width, (H, W), inputs, forced S or None, iso, cam) of every accuracy case of the GPU file."""
    out = []
    for hw, B, seed in G.WIDE3_CASES:
        out.append(("w3 %dx%d" % hw, "paper", WIDE_ARCH, 32, hw, (B, seed), None, ISO, CAM))
    for forced in (1, 2, 3):
        out.append(("w3 40x36 S=%d" % forced, "paper", WIDE_ARCH, 32, (40, 36), (2, 1), forced, ISO, CAM))
    out.append(("w3 64x64", "paper", WIDE_ARCH, 32, (64, 64), (1, G.SEED_64), None, ISO, CAM))
    for forced in (None, 8, 4, 3):
        out.append(("full 8x66" + (" S=%d" % forced if forced else ""), "paper", FULL_ARCH, 32, (8, 66), (4, 1), forced, ISO, CAM))
    out.append(("full 8x66 shipped sdn", "paper sdn", FULL_ARCH, 32, (8, 66), (4, 4), None, ISO, CAM))
    out.append(("vocab per-call", "vocab", VOCAB_ARCH, VW, G.VOCAB_HW, (3, G.VOCAB_SEED), 2, 1600.0, 3.0))
    out.append(("vocab rows", "vocab", VOCAB_ARCH, VW, G.VOCAB_HW, (3, G.VOCAB_ROWS_SEED), 2, ROWS3[:, 0], ROWS3[:, 1]))
    out.append(("no-sdn 66x12", "paper", NO_SDN_ARCH, 32, (66, 12), ("randn", 2, 0), None, None, None))
    out.append(("w17 40x36", "paper", WIDE_ARCH, 17, G.W17_HW, (2, G.W17_SEED), None, ISO, CAM))
    return out


SPECS = _specs()
LABELS = [s[0] for s in SPECS]
_RANDN = {}


def _halos(arch, variables, width, hw):
    """The gradient halos of nf_grad_tile_segments for this model and shape (it reads NF_GRAD_TILE_SEGMENTS)."""
    from noise_flow_amd import _lib, params
    lib = _lib.load()
    layers, descs, flat = params.pack(arch, variables, width, "loss_first")
    cfg = _lib.nf_config(hw[0], hw[1], 4, len(layers), -1, _lib.NF_CFG_GRAD_TILED_WIDE)
    out = (C.c_int32 * 80)()
    n = lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, out, 16)
    assert n >= 1, (n, lib.nf_last_error())
    return [out[5 * i + 2] for i in range(n)]


def _case(spec, shipped_variables, monkeypatch):
    """(reference, width, x, y, iso, cam, [(first layer, one-past-last layer, couplings)]) of a spec.  The plan is the library's
    (nf_grad_tile_segments under the spec's forced count), restated over the reference's layers: the couplings dealt in its counts,
    a segment ending right after its last coupling, the last one taking the rest."""
    label, model, arch, width, hw, ikey, forced, iso, cam = spec
    if model == "paper sdn":
        v, ref = _model(arch, width, shipped_sdn_variables(shipped_variables))
    elif model == "vocab":
        v, ref = _model(arch, width, _vocab())
    else:
        v, ref = _model(arch, width)
    if ikey[0] == "randn":
        if (ikey, hw) not in _RANDN:
            _RANDN[(ikey, hw)] = np.random.RandomState(ikey[2]).randn(ikey[1], hw[0], hw[1], 4).astype(np.float32)
        x, y = _RANDN[(ikey, hw)], None
    else:
        x, y = G._inputs(ikey[0], hw, ikey[1])
    monkeypatch.delenv("NF_GRAD_TILE_SEGMENTS", raising=False)
    if forced:
        monkeypatch.setenv("NF_GRAD_TILE_SEGMENTS", str(forced))
    counts = [h // 4 for h in _halos(arch, v, width, hw)]
    assert not forced or len(counts) == forced, counts
    cpl = [i for i, L in enumerate(ref.layers) if L["type"] == "coupling"]
    assert sum(counts) == len(cpl)
    plan, lo, k = [], 0, 0
    for s, c in enumerate(counts):
        hi = len(ref.layers) if s == len(counts) - 1 else cpl[k + c - 1] + 1
        plan.append((lo, hi, c))
        lo, k = hi, k + c
    return ref, width, x, y, iso, cam, plan


# ---- the tiled sweep ---------------------------------------------------------------------------------------------------------------
def _cnn_on_tile(c, z0, g1, g2, edge):
    """``_Cnn.forward`` with the edge channel given: [1, 1, th + 2, tw + 2], 1 where the padded position is outside the IMAGE."""
    a1 = (F.conv2d(z0, c.w1, c.b1, padding=1) - c.m1) / c.sd1 * g1
    a2 = (F.conv2d(a1, c.w2, c.b2) - c.m2) / c.sd2 * g2
    hp = F.pad(a2, (1, 1, 1, 1))
    o = F.conv2d(torch.cat([hp, edge.expand(hp.shape[0], -1, -1, -1)], 1), c.wl, c.bl) * c.el
    return o[:, :2], o[:, 2:]


def tiled_sweep(ref, x, y, iso, cam, plan, dtype=np.float64, mutant=None):
    """(gx, gy or None) float64 numpy of the tiled, segmented, reversible sweep (module docstring) in `dtype`, on the gates of the
    float64 evaluation of the whole image.  mutant: None | "short_halo" | "tile_edge" | "gy_not_added" | "core_shift"."""
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    gates = ref.gates(x, y, iso, cam)
    to = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dt).permute(0, 3, 1, 2).contiguous()   # noqa: E731
    layers = ref.layers
    B, H, W, _ = x.shape
    n = 4 * H * W
    isos = np.broadcast_to(np.asarray(iso, np.float64).reshape(-1), (B,)) if iso is not None else [None] * B
    cams = np.broadcast_to(np.asarray(cam, np.float64).reshape(-1), (B,)) if cam is not None else [None] * B
    col = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dt).reshape(B, 1, 1, 1)   # noqa: E731
    th, tw = min(H, 32), min(W, 32)
    with torch.no_grad():
        xt, yt = to(x), (to(y) if y is not None else None)
        consts = []
        for li, L in enumerate(layers):
            t = L["type"]
            if t == "conv1x1":
                A64 = torch.as_tensor(np.asarray(L["A"], np.float64))
                consts.append((A64.to(dt), torch.linalg.inv(A64).to(dt)))
            elif t == "coupling":
                consts.append(R._Cnn(L["p"], dt))
            elif t.startswith("sdn"):
                ab = [R._scalar_pair(L, isos[b], cams[b]) for b in range(B)]
                consts.append((col([v[0] for v in ab]), col([v[1] for v in ab])))
            else:
                consts.append(col([R._gain(L, isos[b], n)[0] for b in range(B)]))

        def forward(li, z, ys, gsl, edge):
            """layer li applied to z (a whole image or a tile: ys / gsl / edge are the matching windows)."""
            t, c = layers[li]["type"], consts[li]
            if t == "conv1x1":
                return torch.einsum("bchw,ck->bkhw", z, c[0])
            if t == "coupling":
                g1, g2 = (gates[(li, k)][gsl].to(dt) for k in (1, 2))
                shift, raw = _cnn_on_tile(c, z[:, :2], g1, g2, edge)
                return torch.cat([z[:, :2], z[:, 2:] * torch.exp(c.sc * torch.tanh(raw)) + shift], 1)
            if t.startswith("sdn"):
                return z / torch.sqrt(c[0] * ys + c[1])
            return z / c

        def edge_of(oy, ox, hh, ww, tile_border):
            e = torch.zeros((1, 1, hh + 2, ww + 2), dtype=dt)
            R_ = torch.arange(-1, hh + 1).reshape(-1, 1) + oy
            C_ = torch.arange(-1, ww + 1).reshape(1, -1) + ox
            if tile_border:
                out = (R_ == oy - 1) | (R_ == oy + hh) | (C_ == ox - 1) | (C_ == ox + ww)
            else:
                out = (R_ == -1) | (R_ == H) | (C_ == -1) | (C_ == W)
            e[0, 0] = out.to(dt)
            return e

        # forward: the tensor in front of every segment (the forward launches are exact on their cores)
        whole = (slice(None), slice(None), slice(None), slice(None))
        e_img = edge_of(0, 0, H, W, False)
        zin, z = [], xt
        for lo, hi, _c in plan:
            zin.append(z)
            for li in range(lo, hi):
                z = forward(li, z, yt, whole, e_img)
        # backward, last segment first
        has_gy = yt is not None and any(L["type"].startswith("sdn") for L in layers)
        gy_img = torch.zeros_like(xt) if has_gy else None
        gy_written = False
        g_img = None
        for s in range(len(plan) - 1, -1, -1):
            lo, hi, c = plan[s]
            halo = 4 * c - (1 if (mutant == "short_halo" and c == 1) else 0)
            ny, oys, cy0, cy1 = _axis(H, halo)
            nx, oxs, cx0, cx1 = _axis(W, halo)
            if mutant == "core_shift":
                cy0 = [v + (1 if i else 0) for i, v in enumerate(cy0)]
                cy1 = [v + (1 if i < ny - 1 else 0) for i, v in enumerate(cy1)]
                cx0 = [v + (1 if i else 0) for i, v in enumerate(cx0)]
                cx1 = [v + (1 if i < nx - 1 else 0) for i, v in enumerate(cx1)]
            sdn = any(layers[li]["type"].startswith("sdn") for li in range(lo, hi))
            first_cpl = min([li for li in range(lo, hi) if layers[li]["type"] == "coupling"], default=hi)
            g_next = torch.full_like(xt, float("nan"))
            gy_seg = torch.zeros_like(xt) if has_gy else None
            for ty in range(ny):
                for tx in range(nx):
                    oy, ox = oys[ty], oxs[tx]
                    win = (slice(None), slice(None), slice(oy, oy + th), slice(ox, ox + tw))
                    ys = yt[win] if yt is not None else None
                    edge = edge_of(oy, ox, th, tw, mutant == "tile_edge")
                    z = zin[s][win]
                    outs = {}
                    for li in range(lo, hi):
                        z = forward(li, z, ys, win, edge)
                        if li < first_cpl:
                            outs[li] = z
                    g = z.clone() if s == len(plan) - 1 else g_img[win].clone()
                    gy_t = torch.zeros_like(z)
                    for li in range(hi - 1, lo - 1, -1):
                        t, k = layers[li]["type"], consts[li]
                        z_out = outs.get(li, z)
                        if t == "conv1x1":
                            z = torch.einsum("bkhw,kc->bchw", z_out, k[1])
                            g = torch.einsum("bkhw,ck->bchw", g, k[0])
                        elif t == "coupling":
                            g1, g2 = (gates[(li, q)][win].to(dt) for q in (1, 2))
                            z0 = z_out[:, :2]
                            shift, raw = _cnn_on_tile(k, z0, g1, g2, edge)
                            tnh = torch.tanh(raw)
                            ls = k.sc * tnh
                            e = torch.exp(ls)
                            z1 = (z_out[:, 2:] - shift) * torch.exp(-ls)
                            d_ls = g[:, 2:] * z1 * e - 1.0
                            d_z0 = k.transposed(g[:, 2:], k.sc * (1 - tnh * tnh) * d_ls, g1, g2)
                            g = torch.cat([g[:, :2] + d_z0, g[:, 2:] * e], 1)
                            z = torch.cat([z0, z1], 1)
                        elif t.startswith("sdn"):
                            s2 = k[0] * ys + k[1]
                            sq = torch.sqrt(s2)
                            gy_t = gy_t + 0.5 * k[0] / s2 * (1 - g * z_out)
                            g = g / sq
                            z = z_out * sq
                        else:
                            g = g / k
                            z = z_out * k
                    core = (slice(None), slice(None), slice(cy0[ty], cy1[ty]), slice(cx0[tx], cx1[tx]))
                    tcore = (slice(None), slice(None), slice(cy0[ty] - oy, cy1[ty] - oy), slice(cx0[tx] - ox, cx1[tx] - ox))
                    g_next[core] = g[tcore]
                    if has_gy:
                        gy_seg[core] = gy_t[tcore]
            g_img = g_next
            if has_gy and sdn:
                if not gy_written:
                    gy_img = gy_seg
                elif mutant != "gy_not_added":
                    gy_img = gy_img + gy_seg
                gy_written = True
        back = lambda v: v.permute(0, 2, 3, 1).double().numpy()   # noqa: E731
        return back(g_img), (back(gy_img) if has_gy else None)


# ---- the tiled arithmetic stays inside the bound --------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_tiled_sweep_is_autograd_and_inside_the_bound(shipped_variables, monkeypatch, label):
    ref, width, x, y, iso, cam, plan = _case(SPECS[LABELS.index(label)], shipped_variables, monkeypatch)
    e32 = R.reference_conditions(ref, width, x, y, iso, cam)
    _, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam)
    wx, wy = R.rule_weights(ref, y, iso, cam, x.shape)
    tensors = [("gx", gx64, wx)] + ([("gy", gy64, wy)] if gy64 is not None else [])
    got = tiled_sweep(ref, x, y, iso, cam, plan, np.float64)
    assert (gy64 is None) == (got[1] is None)
    for (name, r64, _), g in zip(tensors, got):
        d = float(R.patch_rel_err(g, r64).max())
        assert d <= 1e-12, (name, d)
    got = tiled_sweep(ref, x, y, iso, cam, plan, np.float32)
    misses = {}
    for (name, r64, w), g in zip(tensors, got):
        for tag, wt in (("", None), ("/w", w)):
            d = R.patch_rel_err(g, r64, wt)
            tol = np.maximum(R.REL_TOL, R.E32_FACTOR * e32[name + tag])
            print("%-24s segments %-26s %-5s %.2e (e32 %.2e)  %.2f of the bound"
                  % (label, [c for _, _, c in plan], name + tag, d.max(), e32[name + tag].max(), (d / tol).max()))
            if not np.all(d <= tol):
                misses[name + tag] = float((d / tol).max())
    assert not misses, misses


# ---- the mutants -----------------------------------------------------------------------------------------------------------------------
# (label, mutant) -> measured worst-element ratio to the combined bound: what the rule does not resolve on that case.
#   tile_edge, EVERY case, 6e-11 .. 6e-10 (fp64 round-off): an edge channel set at a tile border inside the image changes l_last's
#     output on the tile's outermost pixels only — the pixels whose zero padding is wrong anyway —, and what that does to the
#     gradient ends 2 pixels further in, inside the halo of 4 per coupling.  The kernel follows the image border as the narrower
#     widths' tiled kernel does; no test of core values can tell the two choices apart, and none claims to.
#   core_shift is a halo one pixel short on one side of a core, so it needs a core that ENDS at its halo: where an axis has two
#     tiles only, the second one's origin is clamped to the image (33: origin 1, 36: 4, 40: 8) and the overlap is wider than two
#     halos — nothing happens at all (1e-10), or, with 3 couplings in the segment, what happens is below the bound (0.01 .. 0.72).
#     Resolved on every case with a third tile along an axis: 9.8 (segments of 3, 3, 2) .. 3.3e3 (a segment of one coupling).
#   short_halo (segments of one coupling) and gy_not_added are resolved wherever they apply: 1.1e3 .. 9.1e3 and 37 .. 1.8e3.
DROPPED = {(label, "tile_edge"): 6e-10 for label in LABELS}
DROPPED.update({("w3 33x33", "core_shift"): 2.1e-10, ("w3 40x36", "core_shift"): 0.72, ("w3 4x40", "core_shift"): 0.079,
                ("w3 2x40", "core_shift"): 0.012, ("w3 40x36 S=1", "core_shift"): 0.72, ("w3 40x36 S=2", "core_shift"): 1.4e-10,
                ("w3 40x36 S=3", "core_shift"): 1.4e-10, ("vocab per-call", "core_shift"): 5.1e-10, ("vocab rows", "core_shift"): 3.7e-10,
                ("w17 40x36", "core_shift"): 0.0093})
DROPPED_LEAVES_AT = 4.0


def _applies(name, plan, H, W, ref):
    tiles = lambda c: _axis(H, 4 * c)[0] * _axis(W, 4 * c)[0]   # noqa: E731
    if name in ("short_halo", "core_shift", "tile_edge"):
        return any(tiles(c) > 1 for _, _, c in plan) and (name != "short_halo" or any(c == 1 and tiles(c) > 1 for _, _, c in plan))
    n_sdn_segs = sum(1 for lo, hi, _ in plan if any(ref.layers[li]["type"].startswith("sdn") for li in range(lo, hi)))
    return n_sdn_segs >= 2


@pytest.mark.parametrize("label", LABELS)
def test_mutants_exceed_twice_the_bound(shipped_variables, monkeypatch, label):
    ref, width, x, y, iso, cam, plan = _case(SPECS[LABELS.index(label)], shipped_variables, monkeypatch)
    _, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam)
    bound = R.combined_bound(ref, x, y, iso, cam)
    B, H, W, _ = x.shape
    failures = []
    for name in ("short_halo", "tile_edge", "gy_not_added", "core_shift"):
        if not _applies(name, plan, H, W, ref) or (name == "gy_not_added" and gy64 is None):
            continue
        got = tiled_sweep(ref, x, y, iso, cam, plan, np.float64, mutant=name)
        got = tuple(None if g is None else np.nan_to_num(g, nan=0.0) for g in got)
        ratio, raw = _ratios(bound, got, (gx64, gy64))
        dropped = (label, name) in DROPPED
        print("%-24s segments %-26s %-13s %9.3g x the combined bound;  the raw norm alone: %9.3g x%s"
              % (label, [c for _, _, c in plan], name, ratio, raw, "  DROPPED" if dropped else ""))
        if dropped:
            assert ratio < DROPPED_LEAVES_AT, (label, name, ratio)
        elif not ratio >= 2.0:
            failures.append((name, ratio))
    assert not failures, failures


def test_dropped_table():
    """Dropping is capped: never the short halo or the missing gy term, and every entry names a case that exists."""
    for (label, name), ratio in DROPPED.items():
        assert label in LABELS and name in ("tile_edge", "core_shift") and ratio < DROPPED_LEAVES_AT
