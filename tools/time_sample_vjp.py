"""nf_sample_vjp next to nf_sample and nf_nll_grad of the same handle: the shipped model at 32x32 and 64x64, B = 1 024, same box,
same process.

    python tools/time_sample_vjp.py [--launches 200] [--out FILE.json]

The protocol of tools/time_nll_grad.py: every figure is the mean over a window of `--launches` (at least 200) back-to-back launches
between two device events, after a warm-up of a quarter of that; three windows per entry, all three are printed and their median is
reported.  nf_sample is the forward direction alone (one coupling-CNN evaluation per coupling, on the flow kernel); nf_nll_grad does what
nf_sample_vjp does in the other direction — three CNN evaluations per coupling: forward sweep, recomputation, transposed products —
on the same scalar gradient block.  nf_sample_vjp is timed with all four outputs and with x_out = NULL (the backward pass of
sample_torch).  ms per launch, patches/s and the ratios.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("NF_TOOL_LIB"):   # A/B a differently-built library (this tool only)
    from noise_flow_amd import _lib as _nf_lib
    _nf_lib.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 200:
        raise SystemExit("--launches must be at least 200")
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    from noise_flow_amd.ckpt import load_checkpoint
    torch.cuda.set_device(0)
    v = load_checkpoint(os.path.join(ROOT, "models", "NoiseFlow", "ckpt", "model.ckpt.best"))
    B, temp = 1024, 0.6
    cond = _lib.nf_cond(100.0, 2.0, 0.0, 0.0)

    def timed(fn):
        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        window(max(a.launches // 4, 10))
        w = sorted(window(a.launches) for _ in range(3))
        return w[1], w

    res = {"B": B, "temp": temp, "launches_per_window": a.launches, "shapes": {}}
    for side in (32, 64):
        m = NoiseFlow([side, side, 4], False, default_hps(), variables=v, device=0)
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        eps, g = (torch.as_tensor(rng.randn(B, side, side, 4).astype(np.float32)).cuda() for _ in range(2))
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        nll, gt = (torch.empty((B,), device="cuda") for _ in range(2))
        o1, o2, o3 = (torch.empty_like(y) for _ in range(3))
        lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
        t_s, w_s = timed(lambda: _lib.check(lib.nf_sample(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), o1.data_ptr(), st)))
        t_g, w_g = timed(lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                            o1.data_ptr(), o2.data_ptr(), st)))
        t_v, w_v = timed(lambda: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None, g.data_ptr(),
                                                              o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), gt.data_ptr(), st)))
        t_b, w_b = timed(lambda: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None, g.data_ptr(),
                                                              None, o2.data_ptr(), o3.data_ptr(), gt.data_ptr(), st)))
        r = {"sample_ms": t_s, "nll_grad_ms": t_g, "vjp_ms": t_v, "vjp_no_x_ms": t_b,
             "windows": {"sample": w_s, "nll_grad": w_g, "vjp": w_v, "vjp_no_x": w_b},
             "sample_patches_per_s": B / t_s * 1e3, "nll_grad_patches_per_s": B / t_g * 1e3, "vjp_patches_per_s": B / t_v * 1e3,
             "vjp_over_sample": t_v / t_s, "vjp_over_nll_grad": t_v / t_g}
        res["shapes"]["%dx%d" % (side, side)] = r
        fmt = lambda w: "/".join("%.4f" % q for q in w)   # noqa: E731
        print("%dx%d  nf_sample %.4f ms [%s] (%.3e patches/s)   nf_nll_grad %.4f ms [%s] (%.3e patches/s)\n"
              "       nf_sample_vjp %.4f ms [%s] (%.3e patches/s), x_out = NULL %.4f ms [%s]   vjp / sample %.2f   vjp / nll_grad %.2f"
              % (side, side, t_s, fmt(w_s), r["sample_patches_per_s"], t_g, fmt(w_g), r["nll_grad_patches_per_s"], t_v, fmt(w_v),
                 r["vjp_patches_per_s"], t_b, fmt(w_b), r["vjp_over_sample"], r["vjp_over_nll_grad"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
