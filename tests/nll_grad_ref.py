"""Reference for the input gradients of the NLL (helper, not a test).

A torch-CPU restatement of the evaluation-mode NLL as a function of (x, y), built from ``NoiseFlowOracle(...).layers``: the
1x1 matrices, coupling parameters and log-dets are the oracle's, and every SDN / gain kind goes through the oracle's own scale
functions (an SDN scale is sqrt(a*y + b); a and b are read off the oracle's function at y = 0 and y = 1).  It runs in float64
(the reference) and in float32 (the yardstick: how far a plain fp32 evaluation with stored activations sits from fp64), gives
``torch.autograd.grad`` of ``nll.sum()`` — patches are independent in evaluation mode, so that is every patch's own gradient —
accepts a set of ReLU gates to invert, and reports per patch the activations that are "on their kink".

On-kink, exactly as ``oracle.nf_grad_oracle.GradOracle._relu`` but with the RUNNING mean: margin |h - mean| below
``KINK_ULPS`` = 32 units of u = 2^-24 * (sum |input| |weight| + |bias| + |mean|) + err_in, err_in = the round-off l_2's inputs
carry (l_1's u / sqrt(var + eps) pushed through |W2|).
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nf_oracle as O

KINK_ULPS = 32.0
MAX_EXCUSED_KINKS = 3        # conftest.MAX_EXCUSED_KINKS


def _scalar_pair(L, iso, cam):
    """fp64 (a, b) with scale^2 = a*y + b for an SDN kind — from the oracle's own scale function."""
    t, p = L["type"], L["p"]
    y = np.array([0.0, 1.0]).reshape(2, 1, 1, 1)
    if t == "sdn5":
        s = O.sdn_ex5_scale(y, p, iso, cam)
    elif t == "sdn4":
        s = O.sdn_ex4_scale(y, p, iso)
    elif t == "sdn":
        s = O.sdn_plain_scale(y, p)
    elif t == "sdn6":
        s = O.sdn_ex6_scale(y, p, iso, cam)
    else:
        s = O.sdn_ex123_scale(y, p, iso, t)
    s = np.asarray(s, np.float64).reshape(-1)
    return s[1] ** 2 - s[0] ** 2, s[0] ** 2


def _gain(L, iso, n):
    """fp64 (scale, log-det) of a gain kind, as NoiseFlowOracle.inverse writes them; n = H*W*C."""
    t = L["type"]
    if t == "gain4":
        g = float(np.asarray(L["gain_val"]).reshape(-1)[0])
        return g, -n * np.log(g)
    g = float(O.gain_plain_scale(L["p"], iso, np.float64) if t == "gain" else O.gain_ex123_scale(L["p"], iso, t, np.float64))
    return g, (-n if t == "gain2" else -1.0) * np.log(g)


class NllGradRef:
    def __init__(self, arch, variables, binding="loss_first", flow_permutation=1, decomp="LU"):
        self.oracle = O.NoiseFlowOracle(arch, variables, binding, np.float64, flow_permutation=flow_permutation, decomp=decomp)
        self.layers = self.oracle.layers
        self.kinks = []    # (site = (layer index, 1 | 2), flat index into [B, C, H, W], margin in units of u) of the latest call

    # -- ReLU as a constant gate; eval-mode kink report ------------------------------------------------------------------------
    def _relu(self, hn, h, mean, var, amp, site, flips, err_in=None):
        with torch.no_grad():
            gate = hn > 0
            u = 2.0 ** -24 * (amp + mean.abs()[None, :, None, None])
            if err_in is not None:
                u = u + err_in
            margin = (h - mean[None, :, None, None]).abs() / (u + 1e-300)
            for k in torch.nonzero(margin.reshape(-1) < KINK_ULPS).reshape(-1).tolist():
                self.kinks.append((site, k, float(margin.reshape(-1)[k])))
            if flips:
                flat = gate.reshape(-1).clone()
                for st, k in flips:
                    if st == site:
                        flat[k] = ~flat[k]
                gate = flat.reshape(gate.shape)
            err_out = u / torch.sqrt(var[None, :, None, None] + O.BN_EPS)
        return hn * gate.to(hn.dtype), err_out

    def _cnn(self, z0, p, li, dt, flips):
        g = lambda k: torch.as_tensor(np.asarray(p[k], np.float64)).to(dt)   # noqa: E731
        w1, b1 = g("l_1/W").permute(3, 2, 0, 1), g("l_1/b").reshape(-1)
        h = F.conv2d(z0, w1, b1, padding=1)
        with torch.no_grad():
            amp = F.conv2d(z0.abs(), w1.abs(), b1.abs(), padding=1)
        m1, v1 = g("bn1/mean").reshape(-1), g("bn1/var").reshape(-1)
        hn = (h - m1[None, :, None, None]) / torch.sqrt(v1[None, :, None, None] + O.BN_EPS)
        a1, err1 = self._relu(hn, h, m1, v1, amp, (li, 1), flips)
        w2 = g("l_2/W")
        w2 = w2.reshape(w2.shape[-2], w2.shape[-1]).t()[:, :, None, None]
        b2 = g("l_2/b").reshape(-1)
        h = F.conv2d(a1, w2, b2)
        with torch.no_grad():
            amp = F.conv2d(a1.abs(), w2.abs(), b2.abs())
            err2 = F.conv2d(err1, w2.abs())
        m2, v2 = g("bn2/mean").reshape(-1), g("bn2/var").reshape(-1)
        hn = (h - m2[None, :, None, None]) / torch.sqrt(v2[None, :, None, None] + O.BN_EPS)
        a2, _ = self._relu(hn, h, m2, v2, amp, (li, 2), flips, err2)
        hp = F.pad(a2, (1, 1, 1, 1))
        e = torch.zeros_like(hp[:, :1])
        e[:, :, 0, :] = 1
        e[:, :, -1, :] = 1
        e[:, :, :, 0] = 1
        e[:, :, :, -1] = 1
        o = F.conv2d(torch.cat([hp, e], 1), g("l_last/W").permute(3, 2, 0, 1), g("l_last/b").reshape(-1))
        o = o * torch.exp(g("l_last/logs").reshape(1, -1, 1, 1) * O.LOGSCALE_FACTOR)
        c2 = o.shape[1] // 2
        return o[:, :c2], o[:, c2:]

    def nll(self, x, y, iso, cam, dt=torch.float64, flips=()):
        """x, y: torch [B, 4, H, W] of dtype dt (y may be None); iso / cam: scalars or length-B sequences → nll [B]."""
        self.kinks = []
        B, _, H, W = x.shape
        n = 4 * H * W
        isos = np.broadcast_to(np.asarray(iso, np.float64).reshape(-1), (B,)) if iso is not None else [None] * B
        cams = np.broadcast_to(np.asarray(cam, np.float64).reshape(-1), (B,)) if cam is not None else [None] * B
        col = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dt).reshape(B, 1, 1, 1)   # noqa: E731
        z = x
        obj = torch.zeros((B,), dtype=dt)
        for li, L in enumerate(self.layers):
            t = L["type"]
            if t == "conv1x1":
                z = torch.einsum("bchw,ck->bkhw", z, torch.as_tensor(np.asarray(L["A"], np.float64)).to(dt))
                obj = obj + float(L["log_abs_det"]) * (H * W)
            elif t == "coupling":
                z0, z1 = z[:, :2], z[:, 2:]
                shift, raw = self._cnn(z0, L["p"], li, dt, flips)
                ls = float(L["p"]["rescaling_scale"]) * torch.tanh(raw)
                z = torch.cat([z0, z1 * torch.exp(ls) + shift], 1)
                obj = obj + ls.sum(dim=(1, 2, 3))
            elif t.startswith("sdn"):
                ab = [_scalar_pair(L, isos[b], cams[b]) for b in range(B)]
                s2 = col([v[0] for v in ab]) * y + col([v[1] for v in ab])
                z = z / torch.sqrt(s2)
                obj = obj - 0.5 * torch.log(s2).sum(dim=(1, 2, 3))
            else:
                gl = [_gain(L, isos[b], n) for b in range(B)]
                z = z / col([v[0] for v in gl])
                obj = obj + torch.as_tensor(np.asarray([v[1] for v in gl], np.float64)).to(dt)
        obj = obj + (-0.5 * (float(np.log(2 * np.pi)) + z * z)).sum(dim=(1, 2, 3))
        return -obj

    def oracle_nll(self, x, y, iso=None, cam=None):
        """``NoiseFlowOracle.nll`` (fp64) of every patch under its own (iso, cam): scalars or length-B sequences."""
        B = x.shape[0]
        if iso is None or (np.ndim(iso) == 0 and np.ndim(cam) == 0):
            return self.oracle.nll(x, y, iso, cam)[0]
        isos, cams = (np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (B,)) for v in (iso, cam))
        return np.concatenate([self.oracle.nll(x[b:b + 1], None if y is None else y[b:b + 1], float(isos[b]), float(cams[b]))[0]
                               for b in range(B)])

    def nll_and_grads(self, x, y, iso=None, cam=None, dtype=np.float64, flips=()):
        """x, y: numpy [B, H, W, 4] → (nll [B], gx [B, H, W, 4], gy or None) as float64 numpy, computed in `dtype`;
        ``self.kinks`` afterwards lists the on-kink activations of this input (meaningful for the float64 call)."""
        dt = torch.float64 if dtype == np.float64 else torch.float32
        xt = torch.as_tensor(np.asarray(x, np.float64)).to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        yt = None
        if y is not None:
            yt = torch.as_tensor(np.asarray(y, np.float64)).to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        nll = self.nll(xt, yt, iso, cam, dt, flips)
        needs_y = yt is not None and any(L["type"].startswith("sdn") for L in self.layers)
        grads = torch.autograd.grad(nll.sum(), [xt, yt] if needs_y else [xt])
        back = lambda g: g.permute(0, 2, 3, 1).double().numpy()   # noqa: E731
        return nll.detach().double().numpy(), back(grads[0]), (back(grads[1]) if needs_y else None)


def patch_rel_err(got, ref):
    """max|got - ref| / max|ref| per patch → [B]."""
    B = ref.shape[0]
    d = np.abs(np.asarray(got, np.float64) - ref).reshape(B, -1).max(axis=1)
    return d / np.abs(ref).reshape(B, -1).max(axis=1)


def compare_with_kink_rule(ref, width, x, y, iso, cam, got_gx, got_gy, max_on_kink=6, log=None):
    """The comparison and kink rules of tests/test_gpu_nll_grad.py.

    Per patch and tensor (gx, gy):  max|got - ref64| <= tol * max|ref64|,  tol = max(1e-5, 4 * e32), e32 = the float32 helper's
    own distance from the float64 helper on the same tensor and input.  A patch that fails is re-compared against the float64
    reference with a subset of at most MAX_EXCUSED_KINKS of THAT patch's on-kink gates inverted.  Asserts first that no patch
    has more than `max_on_kink` on-kink activations.  Returns per-tensor lists of (kernel distance, e32) per patch."""
    nll64, gx64, gy64 = ref.nll_and_grads(x, y, iso, cam, np.float64)
    kinks = list(ref.kinks)
    B, H, W, _ = x.shape
    per_patch = [[(s, k) for s, k, _ in kinks if k // (width * H * W) == b] for b in range(B)]
    assert max(len(p) for p in per_patch) <= max_on_kink, "kink condition: %r on-kink activations per patch" % [len(p) for p in per_patch]
    _, gx32, gy32 = ref.nll_and_grads(x, y, iso, cam, np.float32)
    ref.kinks = kinks
    out = {}
    failing = set()
    tensors = [("gx", got_gx, gx64, gx32)] + ([("gy", got_gy, gy64, gy32)] if gy64 is not None else [])
    tols = {}
    for name, got, r64, r32 in tensors:
        e32 = patch_rel_err(r32, r64)
        dist = patch_rel_err(got, r64)
        tols[name] = np.maximum(1e-5, 4.0 * e32)
        out[name] = list(zip(dist.tolist(), e32.tolist()))
        if log is not None:
            log("%s: kernel-to-fp64 %s   e32 %s" % (name, " ".join("%.2e" % v for v in dist), " ".join("%.2e" % v for v in e32)))
        failing |= set(np.nonzero(~(dist <= tols[name]))[0].tolist())
    for b in sorted(failing):
        cands = per_patch[b]
        assert cands, "patch %d: %r and no on-kink activation to excuse it" % (b, {n: out[n][b] for n in out})
        ok = False
        for size in range(1, min(len(cands), MAX_EXCUSED_KINKS) + 1):
            for subset in itertools.combinations(cands, size):
                _, ax, ay = ref.nll_and_grads(x, y, iso, cam, np.float64, flips=subset)
                ok = all(patch_rel_err(got[b:b + 1], alt[b:b + 1])[0] <= tols[name][b]
                         for (name, got, _, _), alt in zip(tensors, (ax, ay)))
                if ok:
                    break
            if ok:
                break
        assert ok, "patch %d: %r not explained by inverting <= %d of its %d on-kink gates" % (
            b, {n: out[n][b] for n in out}, MAX_EXCUSED_KINKS, len(cands))
    ref.kinks = kinks
    return nll64, out
