"""Reference for the vector-Jacobian product of sampling (helper, not a test).

``SampleVjpRef`` subclasses ``nll_grad_ref.PinnedRef`` and adds the SAMPLING graph as a torch function of (y, eps, temp), built from
``NoiseFlowOracle.layers`` with ``_cnn``, ``_scalar_pair`` and ``_gain`` of that module: z = eps temp, then the layers last to first,
each inverted.  The VJP is ``torch.autograd.grad((x * g).sum(), [y, eps, temp])`` with temp one value per patch, in float64 (the
reference) and in float32 on the float64 gates (the yardstick e32); kink reporting is the parent's.

THE RULE nf_sample_vjp is held to (``compare_with_kink_rule``), with the constants of nll_grad_ref and none of its own:
  gy, geps   per patch and tensor  max|got - g64| <= max(REL_TOL, E32_FACTOR e32) max|g64|, in the raw norm and in a whitened norm
             (got / w, g64 / w, e32 measured in that norm).  The weights (``rule_weights``) come from the model, y, ISO and cam alone:
             w_y = sum over the sdn-kind layers k of a_k / (2 s_k), w_eps = the product of the scales over the run of elementwise
             layers at the x end (1 if the model's first layer is a mixing or coupling layer);
  gtemp      per patch the same bound against sum|g_z eps|, g_z = d L / d (eps temp) in float64;
  x_out      conftest.close_elem at 1e-5 against ``NoiseFlowOracle.sample`` (the GPU file).
Preconditions (``reference_conditions``), asserted from the reference before a kernel's output is read: every pinned e32 <= E32_MAX,
at most 6 on-kink activations per patch.  A failing patch is excused only by ONE subset of at most MAX_EXCUSED_KINKS of its on-kink
gates whose inversion in the float64 reference makes every tensor pass in both norms.

The sweep (``backward_sweep``): the same VJP written out layer by layer in NLL order — the rules of csrc/nf_sample_grad.hip — in a
stored-activation flavour and in the REVERSIBLE one the kernel runs (every layer's input rebuilt from its output; the layers behind the
last coupling take their values forward from eps temp), with the mutants of tests/test_sample_vjp_rule_cpu.py.

In the shipped model y enters only the last sampling op (the leading sdn5), so gy never sees the couplings there: geps is held on every
case, and ``sdn5|unc|gain|unc|sdn3`` is the case where gy has teeth.
"""
import itertools

import numpy as np
import torch

from conftest import FULL_ARCH, trained_like_variables
from nll_grad_ref import (E32_FACTOR, E32_MAX, KINK_ULPS, MAX_EXCUSED_KINKS, REL_TOL, PinnedRef, _Cnn, _gain, _scalar_pair,  # noqa: F401
                          patch_rel_err)

WIDE_ARCH = "sdn5|unc|unc|gain4|unc"
VOCAB_ARCH = "sdn5|unc|gain|unc|sdn3"
TUPLES5 = [(100, 0), (400, 1), (800, 2), (1600, 3), (3200, 4)]
ISO, CAM = 800.0, 2.0
SHIPPED_TEMP = 0.6                                                   # the wrapper's default temperature
SHIPPED_CASES = [(32, 32), (9, 13), (64, 64), (1, 1), (1, 5)]        # seed 0
WIDTH_CASES = [(4, (16, 16)), (8, (16, 16)), (8, (48, 48)), (16, (16, 16)), (16, (32, 32)), (32, (16, 16)), (32, (24, 24))]   # temp 1, seed 0


def sampling_variables(arch, width, seed=0):
    """``conftest.trained_like_variables`` with l_2/W and l_last/W multiplied by sqrt(4 / width): as it stands that model is
    ill-conditioned in the sampling direction beyond width 4 (pinned e32 up to 1.5e-4 at width 16, 1.2e-4 at width 32)."""
    v = trained_like_variables(arch, width, seed)
    f = np.float32(np.sqrt(4.0 / width))
    for k in v:
        if k.endswith("l_2/W") or k.endswith("l_last/W"):
            v[k] = (v[k] * f).astype(np.float32)
    return v


def case_inputs(B, H, W, seed=0):
    """y = make_inputs(B, H, W, seed)[1]; eps, g = RandomState(seed + 77).randn, in that order (float32 [B, H, W, 4])."""
    from conftest import make_inputs
    y = make_inputs(B, H, W, seed)[1]
    rng = np.random.RandomState(seed + 77)
    eps = rng.randn(B, H, W, 4).astype(np.float32)
    g = rng.randn(B, H, W, 4).astype(np.float32)
    return y, eps, g


def _per_patch(v, B):
    return np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (B,)) if v is not None else [None] * B


class SampleVjpRef(PinnedRef):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._smemo = {}

    def sample(self, y, eps, temp, iso, cam, dt=torch.float64, flips=()):
        """y (or None), eps: torch [B, 4, H, W] of dtype dt; temp: torch [B, 1, 1, 1] → x [B, 4, H, W]."""
        self.kinks = []
        B, _, H, W = eps.shape
        n = 4 * H * W
        isos, cams = _per_patch(iso, B), _per_patch(cam, B)
        col = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dt).reshape(B, 1, 1, 1)   # noqa: E731
        z = eps * temp
        for li in range(len(self.layers) - 1, -1, -1):
            L = self.layers[li]
            t = L["type"]
            if t == "conv1x1":
                z = torch.einsum("bchw,ck->bkhw", z, torch.as_tensor(np.asarray(L["A_inv"], np.float64)).to(dt))
            elif t == "coupling":
                z0, z1 = z[:, :2], z[:, 2:]
                shift, raw = self._cnn(z0, L["p"], li, dt, flips)
                ls = float(L["p"]["rescaling_scale"]) * torch.tanh(raw)
                z = torch.cat([z0, (z1 - shift) * torch.exp(-ls)], 1)
            elif t.startswith("sdn"):
                ab = [_scalar_pair(L, isos[b], cams[b]) for b in range(B)]
                z = z * torch.sqrt(col([v[0] for v in ab]) * y + col([v[1] for v in ab]))
            else:
                z = z * col([_gain(L, isos[b], n)[0] for b in range(B)])
        return z

    def has_sdn(self):
        return any(L["type"].startswith("sdn") for L in self.layers)

    def _vjp(self, y, eps, g, temp, iso, cam, dtype, flips):
        dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        to = lambda a, rg: torch.as_tensor(np.asarray(a, np.float64)).to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(rg)   # noqa: E731
        B = eps.shape[0]
        needs_y = y is not None and self.has_sdn()
        yt = to(y, True) if needs_y else None
        et, gt = to(eps, True), to(g, False)
        tt = torch.full((B, 1, 1, 1), float(temp), dtype=dt, requires_grad=True)
        x = self.sample(yt, et, tt, iso, cam, dt, flips)
        grads = torch.autograd.grad((x * gt).sum(), ([yt] if needs_y else []) + [et, tt])
        back = lambda v: v.permute(0, 2, 3, 1).double().numpy()   # noqa: E731
        gy = back(grads[0]) if needs_y else None
        return back(x.detach()), gy, back(grads[-2]), grads[-1].double().numpy().reshape(B)

    def sample_vjp(self, y, eps, g, temp, iso=None, cam=None, dtype=np.float64, flips=()):
        """numpy [B, H, W, 4] in → (x, gy or None, geps, gtemp [B]) as float64 numpy, computed in `dtype` (float32: on the gates of the
        float64 evaluation); every (input, precision, flips) is evaluated once.  ``self.kinks`` afterwards lists the on-kink
        activations of the float64 evaluation of this input."""
        inp = (id(y), id(eps), id(g), float(temp), repr(iso), repr(cam))
        key = inp + (np.dtype(dtype).name, tuple(flips))
        if key not in self._smemo:
            f32 = np.dtype(dtype) == np.float32
            if f32:
                self.sample_vjp(y, eps, g, temp, iso, cam, np.float64)
            self._record = {} if (not f32 and not flips) else None
            self._pin = self._smemo[inp + ("float64", ())][2] if f32 else None
            try:
                out = self._vjp(y, eps, g, temp, iso, cam, dtype, flips)
            finally:
                gates, self._record, self._pin = self._record, None, None
            kinks = list(self.kinks) if not f32 else self._smemo[inp + ("float64", ())][1]
            self._smemo[key] = (out, kinks, gates, (y, eps, g))
        self.kinks = list(self._smemo[key][1])
        return self._smemo[key][0]

    def sample_gates(self, y, eps, g, temp, iso=None, cam=None):
        self.sample_vjp(y, eps, g, temp, iso, cam, np.float64)
        return self._smemo[(id(y), id(eps), id(g), float(temp), repr(iso), repr(cam), "float64", ())][2]


# ---- the cases of tests/test_sample_vjp_rule_cpu.py and tests/test_gpu_sample_vjp.py --------------------------------------------------
def case_model(name, shipped_variables):
    """→ (arch, variables, coupling width, {flow_permutation / decomp}) of one named case."""
    kind = name[0]
    if kind == "shipped":
        return FULL_ARCH, shipped_variables, 4, {}
    if kind == "width":
        width = name[1]
        return WIDE_ARCH, (trained_like_variables(WIDE_ARCH, 4) if width == 4 else sampling_variables(WIDE_ARCH, width)), width, {}
    if kind == "vocab":
        from test_gpu_nll_grad import _vocab_variables
        hps = {k: v for k, v in name[1].items() if k != "rows"}
        return VOCAB_ARCH, _vocab_variables(hps.get("decomp", "LU")), 4, hps
    assert kind == "nosdn"
    return "unc|gain4|unc", trained_like_variables("unc|gain4|unc", 4, seed=3), 4, {}


def _case(name, shipped_variables):
    """→ (ref, width, y, eps, g, temp, iso, cam) of one named case."""
    arch, v, width, hps = case_model(name, shipped_variables)
    ref = SampleVjpRef(arch, v, **hps)
    kind = name[0]
    if kind == "shipped":
        return (ref, width) + case_inputs(3, name[1][0], name[1][1], 0) + (SHIPPED_TEMP, ISO, CAM)
    if kind == "width":
        return (ref, width) + case_inputs(3, name[2][0], name[2][1], 0) + (1.0, ISO, CAM)
    if kind == "vocab":
        if name[1].get("rows"):
            return (ref, width) + case_inputs(5, 12, 12, 0) + (1.0, np.array([t[0] for t in TUPLES5], np.float64), np.array([t[1] for t in TUPLES5], np.float64))
        return (ref, width) + case_inputs(3, 12, 12, 0) + (1.0, 1600.0, 3.0)
    _, eps, g = case_inputs(3, 8, 8, 0)
    return ref, width, None, eps, g, 1.0, None, None


CASES = ([("shipped", hw) for hw in SHIPPED_CASES] + [("width", w, hw) for w, hw in WIDTH_CASES] +
         [("vocab", {}), ("vocab", {"rows": True}), ("vocab", {"flow_permutation": 0}), ("vocab", {"decomp": "NONE"}), ("nosdn",)])
_MEMO = {}


def get_case(name, shipped_variables):
    key = repr(name)
    if key not in _MEMO:
        _MEMO[key] = _case(name, shipped_variables)
    return _MEMO[key]


def oracle_sample(ref, y, eps, temp, iso, cam):
    B = eps.shape[0]
    if iso is None or np.ndim(iso) == 0:
        return ref.oracle.sample(eps, temp, y, iso, cam)
    return np.concatenate([ref.oracle.sample(eps[b:b + 1], temp, None if y is None else y[b:b + 1], float(iso[b]), float(cam[b])) for b in range(B)])


def rule_weights(ref, y, iso, cam, shape):
    """(w_y or None, w_eps) [B, H, W, 4] float64 — from the model, y, ISO and cam alone."""
    B = shape[0]
    n = 4 * shape[1] * shape[2]
    isos, cams = _per_patch(iso, B), _per_patch(cam, B)
    y64 = None if y is None else np.asarray(y, np.float64)
    we, wy, leading = np.ones(shape, np.float64), None, True
    for L in ref.layers:
        t = L["type"]
        if t.startswith("sdn"):
            ab = [_scalar_pair(L, isos[b], cams[b]) for b in range(B)]
            a, b_ = (np.asarray([v[k] for v in ab], np.float64).reshape(B, 1, 1, 1) for k in (0, 1))
            s = np.sqrt(a * y64 + b_)
            wy = (0.0 if wy is None else wy) + np.abs(a) / (2.0 * s)
            if leading:
                we = we * s
        elif t in ("conv1x1", "coupling"):
            leading = False
        elif leading:
            we = we * np.asarray([_gain(L, isos[b], n)[0] for b in range(B)], np.float64).reshape(B, 1, 1, 1)
    assert np.all(we > 0) and np.all(np.isfinite(we)) and (wy is None or (np.all(wy > 0) and np.all(np.isfinite(wy))))
    return wy, we


def kinks_per_patch(ref, width, y, eps, g, temp, iso, cam):
    ref.sample_vjp(y, eps, g, temp, iso, cam, np.float64)
    B, H, W, _ = eps.shape
    return [[(s, k) for s, k, _ in ref.kinks if k // (width * H * W) == b] for b in range(B)]


def distances(got, want, y, eps, temp, weights):
    """{"gy": [B], "gy/w", "geps", "geps/w", "gtemp"}: `got` = (gy or None, geps, gtemp) against `want` = the float64 (x, gy, geps, gtemp)."""
    wy, we = weights
    _, gy64, ge64, gt64 = want
    out = {}
    if gy64 is not None:
        out["gy"], out["gy/w"] = patch_rel_err(got[0], gy64), patch_rel_err(got[0], gy64, wy)
    out["geps"], out["geps/w"] = patch_rel_err(got[1], ge64), patch_rel_err(got[1], ge64, we)
    B = ge64.shape[0]
    scale = np.abs(ge64 / float(temp) * np.asarray(eps, np.float64)).reshape(B, -1).sum(axis=1)
    out["gtemp"] = np.abs(np.asarray(got[2], np.float64).reshape(B) - gt64) / scale
    return out


def reference_conditions(ref, width, y, eps, g, temp, iso, cam, max_on_kink=6, log=print):
    """The preconditions of a case, from the reference alone → {name: pinned e32 [B]}."""
    want = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float64)
    r32 = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float32)
    e32 = distances(r32[1:], want, y, eps, temp, rule_weights(ref, y, iso, cam, eps.shape))
    counts = [len(p) for p in kinks_per_patch(ref, width, y, eps, g, temp, iso, cam)]
    if log is not None:
        log("reference: on-kink %r  e32 %s" % (counts, "  ".join("%s %s" % (k, " ".join("%.2e" % v for v in e)) for k, e in e32.items())))
    assert all(np.all(e <= E32_MAX) for e in e32.values()), e32
    assert max(counts) <= max_on_kink, "kink condition: %r on-kink activations per patch" % counts
    return e32


def compare_with_kink_rule(ref, width, y, eps, g, temp, iso, cam, got, max_on_kink=6, log=None):
    """The rule of the module docstring: `got` = (gy or None, geps, gtemp) → {name: [(distance, e32) per patch]}."""
    assert isinstance(ref, SampleVjpRef)
    want = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float64)
    per_patch = kinks_per_patch(ref, width, y, eps, g, temp, iso, cam)
    assert max(len(p) for p in per_patch) <= max_on_kink, "kink condition: %r on-kink activations per patch" % [len(p) for p in per_patch]
    r32 = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float32)
    weights = rule_weights(ref, y, iso, cam, eps.shape)
    e32 = distances(r32[1:], want, y, eps, temp, weights)
    dist = distances(got, want, y, eps, temp, weights)
    tols = {k: np.maximum(REL_TOL, E32_FACTOR * e32[k]) for k in e32}
    failing = set()
    for k in dist:
        if log is not None:
            log("%s: kernel-to-fp64 %s   e32 %s" % (k, " ".join("%.2e" % v for v in dist[k]), " ".join("%.2e" % v for v in e32[k])))
        failing |= set(np.nonzero(~(dist[k] <= tols[k]))[0].tolist())
    for b in sorted(failing):
        cands = per_patch[b]
        assert cands, "patch %d: %r and no on-kink activation to excuse it" % (b, {k: (dist[k][b], tols[k][b]) for k in dist})
        ok = False
        for size in range(1, min(len(cands), MAX_EXCUSED_KINKS) + 1):
            for subset in itertools.combinations(cands, size):
                alt = ref.sample_vjp(y, eps, g, temp, iso, cam, np.float64, flips=subset)
                d = distances(got, alt, y, eps, temp, weights)
                ok = all(d[k][b] <= tols[k][b] for k in d)   # ONE subset has to explain every tensor in both norms
                if ok:
                    break
            if ok:
                break
        assert ok, "patch %d: %r not explained by inverting <= %d of its %d on-kink gates" % (
            b, {k: (dist[k][b], tols[k][b]) for k in dist}, MAX_EXCUSED_KINKS, len(cands))
    return {k: list(zip(dist[k].tolist(), e32[k].tolist())) for k in dist}


# ---- the hand-written sweep ----------------------------------------------------------------------------------------------------------
def backward_sweep(ref, y, eps, g, temp, iso=None, cam=None, dtype=np.float64, reversible=False, mutant=None):
    """(x, gy or None, geps, gtemp [B]) float64 numpy by the layer-by-layer rules of csrc/nf_sample_grad.hip, on the gates of the float64
    evaluation of the same input.

    Forward: z = eps temp, the layers last to first, each inverted.  Backward, the layers first to last; with v the output of a
    layer's inverse, u its input and g the cotangent of v:
      conv1x1   v = u Ainv: g <- g Ainv^T; u = v A
      coupling  v1 = (u1 - shift) exp(-ls): g1' = g1 exp(-ls), d shift = -g1', d ls = -g1 v1, d raw = S (1 - tanh^2) d ls,
                g0' = g0 + CNN^T(d shift, d raw) through the recorded gates; u1 = v1 exp(ls) + shift
      sdn       v = u s: gy += g v a / (2 s^2), g <- g s; u = v / s          gain   v = u c: g <- g c; u = v / c
      end       geps = temp g, gtemp_b = sum g eps.
    reversible=False: every v is the stored forward value.  reversible=True: only x is kept and every u is rebuilt as above in `dtype`;
    the layers behind the last coupling (the first ones sampling runs) take their v forward from eps temp.
    mutant: None or (name, layer index or None): "l1_tap" (as nll_grad_ref: l_1's transposed conv of that coupling drops the (-1, -1)
    tap along the last row), "no_dls_lastcol" (that coupling, or with None every coupling: d ls zeroed in the last column),
    "gy_not_added" (that sdn layer's part of gy is not added)."""
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    gates = ref.sample_gates(y, eps, g, temp, iso, cam)
    to = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dt).permute(0, 3, 1, 2).contiguous()   # noqa: E731
    layers = ref.layers
    B, H, W, _ = eps.shape
    n = 4 * H * W
    isos, cams = _per_patch(iso, B), _per_patch(cam, B)
    col = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dt).reshape(B, 1, 1, 1)   # noqa: E731
    mname, mlayer = mutant if mutant is not None else (None, None)
    with torch.no_grad():
        et, gt = to(eps), to(g)
        yt = to(y) if (y is not None and ref.has_sdn()) else None
        tmp = torch.as_tensor(float(temp), dtype=torch.float64).to(dt)
        last_cpl = max([i for i, L in enumerate(layers) if L["type"] == "coupling"], default=-1)
        consts = [None] * len(layers)
        outs = [None] * len(layers)
        z = et * tmp
        for li in range(len(layers) - 1, -1, -1):
            L = layers[li]
            t = L["type"]
            if t == "conv1x1":
                c = (torch.as_tensor(np.asarray(L["A"], np.float64)).to(dt), torch.as_tensor(np.asarray(L["A_inv"], np.float64)).to(dt))
                z = torch.einsum("bchw,ck->bkhw", z, c[1])
            elif t == "coupling":
                c = _Cnn(L["p"], dt)
                g1, g2 = (gates[(li, k)].to(dt) for k in (1, 2))
                shift, raw = c.forward(z[:, :2], g1, g2)
                z = torch.cat([z[:, :2], (z[:, 2:] - shift) * torch.exp(-c.sc * torch.tanh(raw))], 1)
            elif t.startswith("sdn"):
                ab = [_scalar_pair(L, isos[b], cams[b]) for b in range(B)]
                a = col([v[0] for v in ab])
                s2 = a * yt + col([v[1] for v in ab])
                c = (a, s2, torch.sqrt(s2))
                z = z * c[2]
            else:
                c = col([_gain(L, isos[b], n)[0] for b in range(B)])
                z = z * c
            consts[li] = c
            outs[li] = z if (not reversible or li > last_cpl) else None
        x = z
        gg = gt.clone()
        gy = torch.zeros_like(z) if yt is not None else None
        for li in range(len(layers)):
            t, c = layers[li]["type"], consts[li]
            v = outs[li] if outs[li] is not None else z
            if t == "conv1x1":
                gg = torch.einsum("bchw,kc->bkhw", gg, c[1])
                z = torch.einsum("bchw,ck->bkhw", v, c[0])
            elif t == "coupling":
                g1, g2 = (gates[(li, k)].to(dt) for k in (1, 2))
                shift, raw = c.forward(v[:, :2], g1, g2)
                th = torch.tanh(raw)
                ls = c.sc * th
                gu = gg[:, 2:] * torch.exp(-ls)
                d_ls = -gg[:, 2:] * v[:, 2:]
                if mname == "no_dls_lastcol" and mlayer in (None, li):
                    d_ls = d_ls.clone()
                    d_ls[:, :, :, -1] = 0
                d_z0 = c.transposed(-gu, c.sc * (1 - th * th) * d_ls, g1, g2, mname == "l1_tap" and mlayer == li)
                gg = torch.cat([gg[:, :2] + d_z0, gu], 1)
                z = torch.cat([v[:, :2], v[:, 2:] * torch.exp(ls) + shift], 1)
            elif t.startswith("sdn"):
                a, s2, s = c
                if not (mname == "gy_not_added" and mlayer == li):
                    gy = gy + gg * v * (0.5 * a / s2)
                gg = gg * s
                z = v / s
            else:
                gg = gg * c
                z = v / c
        back = lambda v: v.permute(0, 2, 3, 1).double().numpy()   # noqa: E731
        gtemp = (gg * et).sum(dim=(1, 2, 3)).double().numpy()
        return back(x), (back(gy) if gy is not None else None), back(gg * tmp), gtemp
