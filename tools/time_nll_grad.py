"""nf_nll_grad next to nf_nll: the shipped model at 32x32 and 64x64, and the paper-scale model (width 32, 8 couplings) on the
matrix-core gradient kernel, B = 1 024, same box, same process.

    python tools/time_nll_grad.py [--launches 200] [--legs shipped,wide,tiled,tiled_wide,gemm,tiled_gemm] [--out FILE.json]

Every figure is the mean over a window of `--launches` (at least 200) back-to-back launches between two device events, after
a warm-up of a quarter of that; three windows per entry, their median is reported.  The yardstick is nf_nll (the forward
kernel, which the gradient kernel does not touch): ms per launch, patches/s and the ratio grad / nll.

Legs `wide` (the full architecture at width 32; variables: paper_like_variables below, the model of the deep GPU tests):
  A/B at 24x24, the largest 8-coupling shape both gradient kernels hold: a handle with grad_kernel="mfma" (csrc/nf_grad_wide.hip)
      against one without (the scalar kernel, csrc/nf_grad.hip), the arms alternated `--reps` (at least 4) times in one process.
      Reported per arm: the median of its repetitions and its spread (max - min); the matrix-core kernel counts as faster when the
      difference of the medians exceeds twice the larger spread.
      `--ab-sides 8,16,24` adds other shapes both kernels hold.
  32x32: the matrix-core gradient kernel next to nf_nll of the same model (NF_PATH_WIDE32), as for the shipped model.

Leg `tiled` (not in the default set): whole images through the tiled gradient (grad_tiles=True, NF_CFG_GRAD_TILED), the shipped
model at 256x256 x 16 and 1024x1024 x 1.  One handle per segment count S = 8 / 4 / 3 (NF_GRAD_TILE_SEGMENTS, read at nf_create),
the arms alternated `--reps` times in one process, same window protocol; per arm the median and spread of its repetitions,
pixels/s, and the ratio to nf_nll of the same images (median of as many repetitions).  Beside every arm the terms of the
planner's cost model (csrc/nf_host.hip, plan_tile_segments): sum over segments of tiles x couplings, of tiles, and the segment
boundaries x image pixels — what the planner's constants are fitted to.

Leg `tiled_wide` (not in the default set): the same at coupling width 32 (grad_kernel="mfma", grad_tiles=True: NF_CFG_GRAD_TILED_WIDE,
tiles of csrc/nf_grad_wide.hip), FULL_ARCH / paper_like_variables on 64x64 x 1 024 and 256x256 x 16 (`--tw-shapes`).  Arms: the
planner's own choice and S = 8 / 4 / 3, alternated; beside them nf_nll of the same handle and the whole-patch matrix-core kernel at
32x32 x 1 024, per pixel.  Tile-couplings, tiles and boundary pixels are those of the whole launch here (x images).  At the end the least-squares fit of (ms) over (tile-couplings, tiles) of the forced arms of all shapes:
ns per tile-coupling, ns per tile, and their ratio — the per-tile constant of the planner's rule (csrc/nf_host.hip, kGradWideSegs).

Leg `gemm` (not in the default set): the GEMM gradient kernel (grad_kernel="gemm", NF_CFG_GRAD_GEMM, csrc/nf_grad_gemm.hip) at coupling
widths 64, 128 and 512, FULL_ARCH / paper_like_variables on 32x32; width 512 at B = 512, the others at B = 1 024.  Same window
protocol; per width nf_nll of the same handle, the gradient's three window means (median and spread), patches/s, the ratio to nf_nll
and the fraction of the fp32 matrix peak (157.3 TFLOP/s), counting THREE coupling-CNN evaluations per coupling — forward sweep,
recomputation, transposed products: the gates are stored, not recomputed.

Leg `tiled_gemm` (not in the default set): whole images at coupling widths 64, 128 and 512 (`--tg-widths`) through tiles of the GEMM
gradient kernel (grad_kernel="gemm", grad_tiles=True: NF_CFG_GRAD_TILED_GEMM), FULL_ARCH / paper_like_variables on 64x64 x 256 and
256x256 x 16 (`--tg-shapes`).  Arms: the planner's own choice and every feasible forced count S = 8 .. 3, alternated `--reps` times;
beside them nf_nll of the same handle and the whole-patch GEMM gradient kernel at 32x32, per pixel.  A call takes 10 ms .. 1 s here,
so a window is as many back-to-back calls as fill `--tg-window-ms` (at least 3) behind one warm-up call, one window per repetition:
per arm the median and the spread (max - min) of its repetitions.  Beside every arm the planner's terms (tile-couplings, tiles,
boundary pixels of the whole launch; at the end of a width the least-squares fits of the forced arms over them, tiled_gemm_fit: the
per-tile constant of csrc/nf_host.hip, kGradGemmSegs) and the halo recomputation factor it implies, tile pixels evaluated per image pixel and
coupling: sum over segments of couplings x tiles x 1024 / (all couplings x image pixels).
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
    ap.add_argument("--legs", default="shipped,wide")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--ab-sides", default="24", help="patch sides of the A/B legs (both gradient kernels must hold them)")
    ap.add_argument("--tw-shapes", default="64x1024,256x16", help="side x images of the tiled_wide leg")
    ap.add_argument("--tg-widths", default="64,128,512", help="coupling widths of the tiled_gemm leg")
    ap.add_argument("--tg-shapes", default="64x256,256x16", help="side x images of the tiled_gemm leg")
    ap.add_argument("--tg-window-ms", type=float, default=300.0, help="least duration of a timing window of the tiled_gemm leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.legs.split(",")
    if a.reps < 4:
        raise SystemExit("--reps must be at least 4")
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
    for side in (32, 64) if "shipped" in legs else ():
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
    if "wide" in legs:
        res["wide32"] = wide_legs(a, timed, B)
    if "tiled" in legs:
        res["tiled"] = tiled_legs(a, timed, v)
    if "tiled_wide" in legs:
        res["tiled_wide"] = tiled_wide_legs(a, timed)
    if "gemm" in legs:
        res["gemm"] = gemm_legs(a)
    if "tiled_gemm" in legs:
        res["tiled_gemm"] = tiled_gemm_legs(a)
    print("RESULT " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


FULL_ARCH = "sdn5|unc|unc|unc|unc|gain4|unc|unc|unc|unc"


def paper_like_variables(arch, width, seed=0):
    """Fresh variables perturbed so that every term of the stack is exercised, the per-layer gain held independent of the width
    (l_2 by sqrt(4 / w), l_last by sqrt(5 / (w + 1))) — the same construction, value for value, as the model of
    tests/test_gpu_nll_grad_wide.py, restated here so that the tool stands without the test modules."""
    import numpy as np
    from noise_flow_amd import params
    rng = np.random.RandomState(seed + 1000)
    v = params.init_variables(arch, width, 4, seed)
    for k in list(v):
        a = v[k]
        if k.endswith("l_1/W"):
            v[k] = (rng.randn(*a.shape) * 0.4).astype(np.float32)
        elif k.endswith("l_2/W"):
            v[k] = ((rng.randn(*a.shape) * 0.4).astype(np.float32) * np.sqrt(4.0 / width)).astype(np.float32)
        elif k.endswith("l_last/W"):
            v[k] = ((rng.randn(*a.shape) * 0.15).astype(np.float32) * np.sqrt(5.0 / (width + 1))).astype(np.float32)
        elif k.endswith("/b") or k.endswith("l_last/logs"):
            v[k] = (rng.randn(*a.shape) * 0.1).astype(np.float32)
        elif k.endswith("/mean"):
            v[k] = (rng.randn(*a.shape) * 0.2).astype(np.float32)
        elif k.endswith("/var"):
            v[k] = (0.5 + rng.rand(*a.shape)).astype(np.float32)
        elif "rescaling_scale" in k:
            v[k] = np.float32(0.3 + 0.6 * rng.rand())
        elif "log_S" in k or "L_vec" in k or "U_vec" in k:
            v[k] = (a + rng.randn(*a.shape).astype(np.float32) * 0.1).astype(np.float32)
        elif k.endswith("gain_val"):
            v[k] = np.asarray([1.3], np.float32)
    return v


def wide_legs(a, timed, B):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    v = paper_like_variables(FULL_ARCH, 32)
    cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
    out = {}

    def setup(side, grad_kernel):
        m = NoiseFlow([side, side, 4], False, default_hps(arch=FULL_ARCH, width=32), variables=v, device=0, grad_kernel=grad_kernel)
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        bufs = (x, y, torch.empty((B,), device="cuda"), torch.empty_like(x), torch.empty_like(y))
        lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
        grad = lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, bufs[2].data_ptr(),   # noqa: E731
                                                  bufs[3].data_ptr(), bufs[4].data_ptr(), st))
        return m, bufs, grad

    # A/B at 24x24 (and any other side asked for)
    med = lambda t: float(np.median(t))   # noqa: E731
    for side in [int(v) for v in a.ab_sides.split(",") if v]:
        ma, ba, ga = setup(side, "mfma")
        mb, bb, gb = setup(side, "scalar")
        assert ma._flow.lib.nf_grad_path(ma._flow.ptr) == _lib.NF_GRAD_PATH_WIDE32
        assert mb._flow.lib.nf_grad_path(mb._flow.ptr) == _lib.NF_GRAD_PATH_SCALAR
        ta, tb = [], []
        for rep in range(a.reps):
            ta.append(timed(ga))
            tb.append(timed(gb))
            print("%dx%d rep %d  matrix-core %.4f ms   scalar %.4f ms" % (side, side, rep, ta[-1], tb[-1]), flush=True)
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        r = {"mfma_ms": ta, "scalar_ms": tb, "mfma_median_ms": med(ta), "scalar_median_ms": med(tb), "larger_spread_ms": spread,
             "scalar_over_mfma": med(tb) / med(ta), "faster_by_the_rule": bool(med(tb) - med(ta) > 2.0 * spread)}
        out["%dx%d" % (side, side)] = r
        print("%dx%d  matrix-core %.4f ms (%.3e patches/s)   scalar %.4f ms (%.3e patches/s)   scalar / matrix-core %.2f   "
              "difference %.4f ms vs 2 x larger in-arm spread %.4f ms: %s"
              % (side, side, med(ta), B / med(ta) * 1e3, med(tb), B / med(tb) * 1e3, med(tb) / med(ta), med(tb) - med(ta), 2.0 * spread,
                 "faster" if r["faster_by_the_rule"] else "NOT faster by the rule"), flush=True)
        del ma, mb, ba, bb
    # 32x32 next to nf_nll
    m, (x, y, nll, gx, gy), grad = setup(32, "mfma")
    sd, ld = torch.empty((B,), device="cuda"), torch.empty((B,), device="cuda")
    lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
    assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_WIDE32 and lib.nf_kernel_path(h, 0) == _lib.NF_PATH_WIDE32
    t_nll = timed(lambda: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                ld.data_ptr(), None, None, 0, st)))
    t_grad = timed(grad)
    out["32x32"] = {"nll_ms": t_nll, "grad_ms": t_grad, "nll_patches_per_s": B / t_nll * 1e3, "grad_patches_per_s": B / t_grad * 1e3,
                    "grad_over_nll": t_grad / t_nll}
    print("width 32, 32x32  nf_nll %.4f ms (%.3e patches/s)   nf_nll_grad (matrix-core) %.4f ms (%.3e patches/s)   ratio %.2f"
          % (t_nll, B / t_nll * 1e3, t_grad, B / t_grad * 1e3, t_grad / t_nll), flush=True)
    return out


def tiled_legs(a, timed, v):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    cond = _lib.nf_cond(100.0, 2.0, 0.0, 0.0)
    med = lambda t: float(np.median(t))   # noqa: E731
    out = {}
    for side, B in ((256, 16), (1024, 1)):
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        nll, sd, ld = (torch.empty((B,), device="cuda") for _ in range(3))
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        arms = {}
        for S in (8, 4, 3):
            os.environ["NF_GRAD_TILE_SEGMENTS"] = str(S)
            m = NoiseFlow([side, side, 4], False, default_hps(), variables=v, device=0, grad_tiles=True)
            os.environ.pop("NF_GRAD_TILE_SEGMENTS")
            lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
            assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_TILED
            _lib.check(lib.nf_reserve_grad_workspace(h, B, 1))
            cfg, descs, flat = m._flow._model_args
            seg = (C.c_int32 * 80)()
            os.environ["NF_GRAD_TILE_SEGMENTS"] = str(S)
            n = lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, seg, 16)
            os.environ.pop("NF_GRAD_TILE_SEGMENTS")
            assert n == S
            rows = [tuple(seg[5 * i:5 * i + 5]) for i in range(n)]
            plan = {"segments": n, "tile_couplings": sum(r[3] * r[4] * (r[2] // 4) for r in rows), "tiles": sum(r[3] * r[4] for r in rows),
                    "boundary_pixels": (n - 1) * side * side}
            grad = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                                          gx.data_ptr(), gy.data_ptr(), st)))
            fwd = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                                    ld.data_ptr(), None, None, 0, st)))
            arms[S] = {"model": m, "grad": grad, "fwd": fwd, "plan": plan, "ms": []}
        t_nll = []
        for rep in range(a.reps):
            t_nll.append(timed(arms[8]["fwd"]))
            for S in (8, 4, 3):
                arms[S]["ms"].append(timed(arms[S]["grad"]))
            print("%dx%d x %d rep %d  nf_nll %.4f ms   nf_nll_grad S=8 %.4f  S=4 %.4f  S=3 %.4f ms"
                  % (side, side, B, rep, t_nll[-1], arms[8]["ms"][-1], arms[4]["ms"][-1], arms[3]["ms"][-1]), flush=True)
        px = float(B) * side * side
        r = {"B": B, "nll_ms": t_nll, "nll_median_ms": med(t_nll), "nll_pixels_per_s": px / med(t_nll) * 1e3, "arms": {}}
        for S in (8, 4, 3):
            t = arms[S]["ms"]
            r["arms"]["S=%d" % S] = dict(arms[S]["plan"], ms=t, median_ms=med(t), spread_ms=max(t) - min(t), pixels_per_s=px / med(t) * 1e3,
                                        grad_over_nll=med(t) / med(t_nll))
            print("%dx%d x %d  S=%d  %.4f ms (spread %.4f)  %.3e pixels/s  grad / nll %.2f   tile-couplings %d  tiles %d  boundary pixels %d"
                  % (side, side, B, S, med(t), max(t) - min(t), px / med(t) * 1e3, med(t) / med(t_nll), arms[S]["plan"]["tile_couplings"],
                     arms[S]["plan"]["tiles"], arms[S]["plan"]["boundary_pixels"]), flush=True)
        out["%dx%d" % (side, side)] = r
        del arms
    return out


def tiled_wide_legs(a, timed):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    v = paper_like_variables(FULL_ARCH, 32)
    cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
    med = lambda t: float(np.median(t))   # noqa: E731
    out = {}

    def with_forced(S, fn):
        if S:
            os.environ["NF_GRAD_TILE_SEGMENTS"] = str(S)
        try:
            return fn()
        finally:
            os.environ.pop("NF_GRAD_TILE_SEGMENTS", None)

    def tensors(B, side):
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        return x, y, torch.empty((B,), device="cuda"), torch.empty_like(x), torch.empty_like(y)

    # the whole-patch matrix-core kernel at 32x32, per pixel
    B32 = 1024
    m32 = NoiseFlow([32, 32, 4], False, default_hps(arch=FULL_ARCH, width=32), variables=v, device=0, grad_kernel="mfma", grad_tiles=True)
    x, y, nll, gx, gy = tensors(B32, 32)
    lib, h, st = m32._flow.lib, m32._flow.ptr, m32._dev.stream_ptr()
    assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_WIDE32
    t32 = timed(lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B32, C.byref(cond), None, nll.data_ptr(), gx.data_ptr(),
                                                   gy.data_ptr(), st)))
    whole_pps = B32 * 1024.0 / t32 * 1e3
    out["32x32"] = {"B": B32, "grad_ms": t32, "pixels_per_s": whole_pps}
    print("width 32, 32x32 x %d whole-patch matrix-core kernel  %.4f ms  %.3e pixels/s" % (B32, t32, whole_pps), flush=True)
    del m32, x, y, nll, gx, gy

    fit_rows = []
    for side, B in [tuple(int(q) for q in w.split("x")) for w in a.tw_shapes.split(",") if w]:
        x, y, nll, gx, gy = tensors(B, side)
        sd, ld = torch.empty((B,), device="cuda"), torch.empty((B,), device="cuda")
        arms = {}
        for S in (0, 8, 4, 3):     # 0: the planner's choice
            m = with_forced(S, lambda: NoiseFlow([side, side, 4], False, default_hps(arch=FULL_ARCH, width=32), variables=v, device=0,
                                                 grad_kernel="mfma", grad_tiles=True))
            lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
            assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_TILED_WIDE32
            _lib.check(lib.nf_reserve_grad_workspace(h, B, 1))
            cfg, descs, flat = m._flow._model_args
            seg = (C.c_int32 * 80)()
            n = with_forced(S, lambda: lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, seg, 16))
            assert n > 0 and (not S or n == S)
            rows = [tuple(seg[5 * i:5 * i + 5]) for i in range(n)]
            plan = {"segments": n, "tile_couplings": B * sum(r[3] * r[4] * (r[2] // 4) for r in rows), "tiles": B * sum(r[3] * r[4] for r in rows),
                    "boundary_pixels": (n - 1) * B * side * side}
            grad = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                                          gx.data_ptr(), gy.data_ptr(), st)))
            fwd = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                                    ld.data_ptr(), None, None, 0, st)))
            arms[S] = {"model": m, "grad": grad, "fwd": fwd, "plan": plan, "ms": []}
        t_nll = []
        for rep in range(a.reps):
            t_nll.append(timed(arms[0]["fwd"]))
            for S in (0, 8, 4, 3):
                arms[S]["ms"].append(timed(arms[S]["grad"]))
            print("%dx%d x %d rep %d  nf_nll %.4f ms   nf_nll_grad unforced (S=%d) %.4f  S=8 %.4f  S=4 %.4f  S=3 %.4f ms"
                  % (side, side, B, rep, t_nll[-1], arms[0]["plan"]["segments"], arms[0]["ms"][-1], arms[8]["ms"][-1], arms[4]["ms"][-1],
                     arms[3]["ms"][-1]), flush=True)
        px = float(B) * side * side
        r = {"B": B, "nll_ms": t_nll, "nll_median_ms": med(t_nll), "nll_pixels_per_s": px / med(t_nll) * 1e3, "arms": {}}
        for S in (0, 8, 4, 3):
            t = arms[S]["ms"]
            name = "S=%d" % S if S else "unforced"
            r["arms"][name] = dict(arms[S]["plan"], ms=t, median_ms=med(t), spread_ms=max(t) - min(t), pixels_per_s=px / med(t) * 1e3,
                                   grad_over_nll=med(t) / med(t_nll), whole_patch_over_this=whole_pps / (px / med(t) * 1e3))
            print("%dx%d x %d  %-8s (S=%d)  %.4f ms (spread %.4f)  %.3e pixels/s  grad / nll %.2f  32x32 whole-patch pixels/s over this %.2f   "
                  "tile-couplings %d  tiles %d  boundary pixels %d"
                  % (side, side, B, name, arms[S]["plan"]["segments"], med(t), max(t) - min(t), px / med(t) * 1e3, med(t) / med(t_nll),
                     whole_pps / (px / med(t) * 1e3), arms[S]["plan"]["tile_couplings"], arms[S]["plan"]["tiles"], arms[S]["plan"]["boundary_pixels"]),
                  flush=True)
            if S:
                fit_rows.append((arms[S]["plan"]["tile_couplings"], arms[S]["plan"]["tiles"], med(t)))
        out["%dx%d" % (side, side)] = r
        del arms
    if len(fit_rows) >= 2:
        A = np.array([[r[0], r[1]] for r in fit_rows], np.float64)
        t = np.array([r[2] for r in fit_rows], np.float64) * 1e6      # ns
        coef = np.linalg.lstsq(A, t, rcond=None)[0]
        resid = (A @ coef - t) / t
        out["fit"] = {"ns_per_tile_coupling": float(coef[0]), "ns_per_tile": float(coef[1]), "per_tile_in_tile_couplings": float(coef[1] / coef[0]),
                      "largest_relative_residual": float(np.abs(resid).max()), "rows": len(fit_rows)}
        print("fit over %d forced arms: %.1f ns per tile-coupling, %.1f ns per tile: a tile costs its couplings + %.2f (largest residual %.1f %%)"
              % (len(fit_rows), coef[0], coef[1], coef[1] / coef[0], 100.0 * np.abs(resid).max()), flush=True)
    return out


def gemm_legs(a):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
    PEAK = 157.3e12   # fp32 matrix peak of an MI355X, FLOP/s
    EVALS = 3         # coupling-CNN evaluations per coupling: forward sweep, recomputation, transposed products
    out = {}

    def windows(fn):   # the window protocol of `timed`, all three window means kept
        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        window(max(a.launches // 4, 10))
        return sorted(window(a.launches) for _ in range(3))

    for width, B in ((64, 1024), (128, 1024), (512, 512)):
        v = paper_like_variables(FULL_ARCH, width)
        m = NoiseFlow([32, 32, 4], False, default_hps(arch=FULL_ARCH, width=width), variables=v, device=0, grad_kernel="gemm")
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, 32, 32, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, 32, 32, 4) * 0.02).astype(np.float32)).cuda()
        nll, sd, ld = (torch.empty((B,), device="cuda") for _ in range(3))
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
        assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_GEMM and lib.nf_kernel_path(h, 0) == _lib.NF_PATH_GEMM
        _lib.check(lib.nf_reserve_grad_workspace(h, B, 1))
        t_nll = windows(lambda: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                      ld.data_ptr(), None, None, 0, st)))
        t_grad = windows(lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                            gx.data_ptr(), gy.data_ptr(), st)))
        n_cpl = FULL_ARCH.split("|").count("unc")
        flop = 2.0 * (18 * width + width * width + 36 * width) * 1024 * n_cpl * B   # one coupling-CNN evaluation of every coupling and patch
        r = {"B": B, "nll_ms": t_nll, "grad_ms": t_grad, "nll_median_ms": t_nll[1], "grad_median_ms": t_grad[1],
             "grad_spread_ms": t_grad[2] - t_grad[0], "nll_spread_ms": t_nll[2] - t_nll[0], "grad_patches_per_s": B / t_grad[1] * 1e3,
             "nll_patches_per_s": B / t_nll[1] * 1e3, "grad_over_nll": t_grad[1] / t_nll[1],
             "grad_fraction_of_fp32_matrix_peak": EVALS * flop / (t_grad[1] * 1e-3) / PEAK, "nll_fraction_of_fp32_matrix_peak": flop / (t_nll[1] * 1e-3) / PEAK,
             "workspace_bytes": int(lib.nf_workspace_bytes(h, 2, B))}
        out["w%d" % width] = r
        print("width %d, 32x32 x %d  nf_nll %.4f ms (spread %.4f, %.3f of peak)   nf_nll_grad (GEMM) %.4f ms (spread %.4f)  %.3e patches/s   "
              "ratio %.2f   %.3f of the fp32 matrix peak at %d evaluations per coupling   gate scratch %.1f MiB"
              % (width, B, t_nll[1], r["nll_spread_ms"], r["nll_fraction_of_fp32_matrix_peak"], t_grad[1], r["grad_spread_ms"], r["grad_patches_per_s"],
                 r["grad_over_nll"], r["grad_fraction_of_fp32_matrix_peak"], EVALS, r["workspace_bytes"] / 2.0 ** 20), flush=True)
        del m, x, y, gx, gy
    return out


def tiled_gemm_fit(width, res, n_cpl):
    """Least squares of the forced arms' medians (ns) of one width, all shapes of `res` together, over (tile-couplings, tiles) and over
    (tile-couplings, tiles, boundary pixels): the per-tile constant of the planner's rule (csrc/nf_host.hip, kGradGemmSegs) is the ratio
    of the first fit's two coefficients.  Beside them the whole-patch kernel's time per 32x32 patch and coupling."""
    import numpy as np
    rows = [(arm["tile_couplings"], arm["tiles"], arm["boundary_pixels"], arm["median_ms"])
            for shape, r in res.items() if shape != "32x32" for name, arm in r["arms"].items() if name != "unforced"]
    fit = {"rows": len(rows), "whole_patch_ns_per_tile_coupling": res["32x32"]["grad_ms"][1] * 1e6 / (res["32x32"]["B"] * n_cpl)}
    if len(rows) >= 3:
        t = np.array([r[3] for r in rows], np.float64) * 1e6      # ns
        for terms in (2, 3):
            A = np.array([r[:terms] for r in rows], np.float64)
            coef = np.linalg.lstsq(A, t, rcond=None)[0]
            fit["%d_terms" % terms] = {"ns_per_tile_coupling": float(coef[0]), "ns_per_tile": float(coef[1]),
                                       "ns_per_boundary_pixel": float(coef[2]) if terms == 3 else None,
                                       "per_tile_in_tile_couplings": float(coef[1] / coef[0]),
                                       "largest_relative_residual": float(np.abs((A @ coef - t) / t).max())}
        f2, f3 = fit["2_terms"], fit["3_terms"]
        print("width %d  fit over %d forced arms: %.1f ns per tile-coupling, %.1f ns per tile: a tile costs its couplings + %.2f (largest residual %.1f %%)"
              % (width, len(rows), f2["ns_per_tile_coupling"], f2["ns_per_tile"], f2["per_tile_in_tile_couplings"], 100.0 * f2["largest_relative_residual"]),
              flush=True)
        print("width %d  fit with a third term: %.1f ns per tile-coupling, %.1f ns per tile, %.4f ns per boundary pixel (largest residual %.1f %%)"
              % (width, f3["ns_per_tile_coupling"], f3["ns_per_tile"], f3["ns_per_boundary_pixel"], 100.0 * f3["largest_relative_residual"]), flush=True)
    print("width %d  whole-patch kernel: %.1f ns per 32x32 patch and coupling" % (width, fit["whole_patch_ns_per_tile_coupling"]), flush=True)
    return fit


def tiled_gemm_legs(a):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
    med = lambda t: float(np.median(t))   # noqa: E731
    n_cpl = FULL_ARCH.split("|").count("unc")
    out = {}

    def window(fn):
        """ms per call over one window: a warm-up call (timed, to size the window), then max(3, window / call) calls between two events."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        n = max(3, int(np.ceil(a.tg_window_ms / max(e0.elapsed_time(e1), 1e-3))))
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def with_forced(S, fn):
        if S:
            os.environ["NF_GRAD_TILE_SEGMENTS"] = str(S)
        try:
            return fn()
        finally:
            os.environ.pop("NF_GRAD_TILE_SEGMENTS", None)

    def tensors(B, side):
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        return x, y, torch.empty((B,), device="cuda"), torch.empty_like(x), torch.empty_like(y)

    forced = [S for S in range(n_cpl, 0, -1) if -(-n_cpl // S) <= 3]     # at most 3 couplings per segment: 8 .. 3
    for width in [int(w) for w in a.tg_widths.split(",") if w]:
        v = paper_like_variables(FULL_ARCH, width)
        hps = lambda: default_hps(arch=FULL_ARCH, width=width)   # noqa: E731
        res = {}
        # the whole-patch GEMM gradient kernel at 32x32, per pixel
        B32 = 512 if width > 128 else 1024
        m32 = NoiseFlow([32, 32, 4], False, hps(), variables=v, device=0, grad_kernel="gemm", grad_tiles=True)
        x, y, nll, gx, gy = tensors(B32, 32)
        lib, h, st = m32._flow.lib, m32._flow.ptr, m32._dev.stream_ptr()
        assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_GEMM
        _lib.check(lib.nf_reserve_grad_workspace(h, B32, 1))
        t32 = sorted(window(lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B32, C.byref(cond), None, nll.data_ptr(), gx.data_ptr(),
                                                               gy.data_ptr(), st))) for _ in range(3))
        whole_pps = B32 * 1024.0 / t32[1] * 1e3
        res["32x32"] = {"B": B32, "grad_ms": t32, "pixels_per_s": whole_pps, "patches_per_s": B32 / t32[1] * 1e3}
        print("width %d, 32x32 x %d whole-patch GEMM gradient kernel  %.4f ms (spread %.4f)  %.3e patches/s  %.3e pixels/s"
              % (width, B32, t32[1], t32[2] - t32[0], B32 / t32[1] * 1e3, whole_pps), flush=True)
        del m32, x, y, nll, gx, gy
        for side, B in [tuple(int(q) for q in w.split("x")) for w in a.tg_shapes.split(",") if w]:
            x, y, nll, gx, gy = tensors(B, side)
            sd, ld = torch.empty((B,), device="cuda"), torch.empty((B,), device="cuda")
            arms = {}
            for S in [0] + forced:     # 0: the planner's choice
                m = with_forced(S, lambda: NoiseFlow([side, side, 4], False, hps(), variables=v, device=0, grad_kernel="gemm", grad_tiles=True))
                lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
                assert lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_TILED_GEMM
                _lib.check(lib.nf_reserve_grad_workspace(h, B, 1))
                cfg, descs, flat = m._flow._model_args
                seg = (C.c_int32 * 80)()
                n = with_forced(S, lambda: lib.nf_grad_tile_segments(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, seg, 16))
                assert n > 0 and (not S or n == S)
                rows = [tuple(seg[5 * i:5 * i + 5]) for i in range(n)]
                tc = sum(r[3] * r[4] * (r[2] // 4) for r in rows)
                plan = {"segments": n, "couplings_per_segment": [r[2] // 4 for r in rows], "tile_couplings": B * tc, "tiles": B * sum(r[3] * r[4] for r in rows),
                        "boundary_pixels": (n - 1) * B * side * side, "halo_recomputation": tc * 1024.0 / (n_cpl * side * side),
                        "workspace_bytes": int(lib.nf_workspace_bytes(h, 2, B))}
                grad = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                                              gx.data_ptr(), gy.data_ptr(), st)))
                fwd = (lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                                        ld.data_ptr(), None, None, 0, st)))
                arms[S] = {"model": m, "grad": grad, "fwd": fwd, "plan": plan, "ms": []}
            t_nll = []
            for r_ in range(a.reps):
                t_nll.append(window(arms[0]["fwd"]))
                for S in arms:
                    arms[S]["ms"].append(window(arms[S]["grad"]))
                print("width %d  %dx%d x %d rep %d  nf_nll %.4f ms   nf_nll_grad unforced (S=%d) %.4f  %s ms"
                      % (width, side, side, B, r_, t_nll[-1], arms[0]["plan"]["segments"], arms[0]["ms"][-1],
                         "  ".join("S=%d %.4f" % (S, arms[S]["ms"][-1]) for S in forced)), flush=True)
            px = float(B) * side * side
            r = {"B": B, "nll_ms": t_nll, "nll_median_ms": med(t_nll), "nll_spread_ms": max(t_nll) - min(t_nll), "nll_pixels_per_s": px / med(t_nll) * 1e3,
                 "arms": {}}
            for S in arms:
                t = arms[S]["ms"]
                name = "S=%d" % S if S else "unforced"
                r["arms"][name] = dict(arms[S]["plan"], ms=t, median_ms=med(t), spread_ms=max(t) - min(t), pixels_per_s=px / med(t) * 1e3,
                                       grad_over_nll=med(t) / med(t_nll), fraction_of_whole_patch_pixel_rate=(px / med(t) * 1e3) / whole_pps)
                print("width %d  %dx%d x %d  %-8s (S=%d %r)  %.4f ms (spread %.4f)  %.3e pixels/s  grad / nll %.2f  %.3f of the 32x32 whole-patch pixel rate   "
                      "halo recomputation %.2f   tile-couplings %d  tiles %d  boundary pixels %d  workspace %.1f MiB"
                      % (width, side, side, B, name, arms[S]["plan"]["segments"], arms[S]["plan"]["couplings_per_segment"], med(t), max(t) - min(t),
                         px / med(t) * 1e3, med(t) / med(t_nll), (px / med(t) * 1e3) / whole_pps, arms[S]["plan"]["halo_recomputation"],
                         arms[S]["plan"]["tile_couplings"], arms[S]["plan"]["tiles"], arms[S]["plan"]["boundary_pixels"],
                         arms[S]["plan"]["workspace_bytes"] / 2.0 ** 20), flush=True)
            best = min((k for k in r["arms"] if k != "unforced"), key=lambda k: r["arms"][k]["median_ms"])
            r["fastest_forced_arm"] = best
            r["unforced_over_fastest"] = r["arms"]["unforced"]["median_ms"] / r["arms"][best]["median_ms"]
            print("width %d  %dx%d x %d  nf_nll %.4f ms (spread %.4f)   fastest forced arm %s; unforced / fastest %.4f"
                  % (width, side, side, B, med(t_nll), max(t_nll) - min(t_nll), best, r["unforced_over_fastest"]), flush=True)
            res["%dx%d" % (side, side)] = r
            del arms, x, y, nll, gx, gy
        res["fit"] = tiled_gemm_fit(width, res, n_cpl)
        out["w%d" % width] = res
    return out


if __name__ == "__main__":
    sys.exit(main())
