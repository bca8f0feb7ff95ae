"""nf_nll_grad next to nf_nll: the shipped model at 32x32 and 64x64, B = 1 024, same box, same process.

    python tools/time_nll_grad.py [--launches 200] [--out FILE.json]

Every figure is the mean over a window of `--launches` (at least 200) back-to-back launches between two device events, after
a warm-up of a quarter of that; three windows per entry, their median is reported.  The yardstick is nf_nll (the forward
kernel, which the gradient kernel does not touch): ms per launch, patches/s and the ratio grad / nll.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    B = 1024
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
        return sorted(window(a.launches) for _ in range(3))[1]

    res = {"B": B, "launches_per_window": a.launches, "shapes": {}}
    for side in (32, 64):
        m = NoiseFlow([side, side, 4], False, default_hps(), variables=v, device=0)
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        nll, sd, ld = (torch.empty((B,), device="cuda") for _ in range(3))
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
        t_nll = timed(lambda: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                    ld.data_ptr(), None, None, 0, st)))
        t_grad = timed(lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                          gx.data_ptr(), gy.data_ptr(), st)))
        r = {"nll_ms": t_nll, "grad_ms": t_grad, "nll_patches_per_s": B / t_nll * 1e3, "grad_patches_per_s": B / t_grad * 1e3,
             "grad_over_nll": t_grad / t_nll}
        res["shapes"]["%dx%d" % (side, side)] = r
        print("%dx%d  nf_nll %.4f ms (%.3e patches/s)   nf_nll_grad %.4f ms (%.3e patches/s)   ratio %.2f"
              % (side, side, t_nll, r["nll_patches_per_s"], t_grad, r["grad_patches_per_s"], r["grad_over_nll"]), flush=True)
    print("RESULT " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
