"""nf_sample_vjp next to nf_sample and nf_nll_grad of the same handle: the shipped model at 32x32 and 64x64, B = 1 024, same box,
same process.

    python tools/time_sample_vjp.py [--launches 200] [--out FILE.json]

The protocol of tools/time_nll_grad.py: every figure is the mean over a window of `--launches` (at least 200) back-to-back launches
between two device events, after a warm-up of a quarter of that; three windows per entry, all three are printed and their median is
reported.  nf_sample is the forward direction alone (one coupling-CNN evaluation per coupling, on the flow kernel); nf_nll_grad does what
nf_sample_vjp does in the other direction — three CNN evaluations per coupling: forward sweep, recomputation, transposed products —
on the same scalar gradient block.  nf_sample_vjp is timed with all four outputs and with x_out = NULL (the backward pass of
sample_torch).  ms per launch, patches/s and the ratios.

    python tools/time_sample_vjp.py --width 32 --kernel mfma [--reps 4] [--ab-sides 24,16]

The matrix-core kernel (csrc/nf_sample_grad_wide.hip, sample_vjp_kernel="mfma") on the deep model at width 32 (deep_variables below),
B = 1 024, temp 0.6, the same windows.  32x32: nf_sample_vjp (all outputs, and x_out = NULL) against nf_nll_grad (NF_GRAD_PATH_WIDE32:
the same three CNN evaluations per coupling) and nf_sample of the same handle.  `--ab-sides`: the new kernel against the scalar
nf_sample_vjp of a handle without the flag, arms alternated `--reps` times; per arm the median and the spread (max - min) of its
`--reps` medians, and the difference read against twice the larger spread.

    python tools/time_sample_vjp.py --kernel gemm [--widths 64,128,512] [--reps 3] [--launches 20] [--batch 1024]

The GEMM kernel (csrc/nf_sample_grad_gemm.hip, sample_vjp_kernel="gemm", NF_SVJP_PATH_GEMM) on FULL_ARCH (8 couplings) at each width,
32x32, temp 0.6, weights of `default_hps` initialisation.  nf_sample_vjp (all outputs), nf_nll_grad (NF_GRAD_PATH_GEMM: the same three CNN
evaluations per coupling) and nf_sample of the same handle, ALTERNATED: `--reps` rounds, one window of `--launches` launches per call
and round after a warm-up window; per call the median of its windows and their spread (max - min), the two ratios, and the fraction
of the fp32 matrix peak (157.3 TFLOP/s) at three CNN evaluations per coupling.  The workspace is reserved first.  (`--launches` may be
below 200 here: a launch is 5 .. 120 ms.)

    python tools/time_sample_vjp.py --legs tiled [--reps 3]

The tile mode (sample_vjp_tiles=True, NF_SVJP_PATH_TILED) on the shipped model at 256x256 x 16 and 1024x1024 x 1, temp 0.6, under the
plans NF_GRAD_TILE_SEGMENTS = 8 / 4 / 3 (one handle per plan; the switch is read when a handle is made).  Per plan: nf_sample_vjp with
all outputs and with x_out = NULL, the tiled nf_sample and the tiled nf_nll_grad of the same handle and images.  The arms are alternated
in one process: `--reps` rounds over the three handles, one window of `--launches` launches per call and round; the median of a call's
windows is reported, all windows are printed.  The workspace is reserved first, so no window contains an allocation.
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


def gemm_legs(a):
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps
    torch.cuda.set_device(0)
    B, temp, side = a.batch, 0.6, 32
    reps = a.reps or 3
    cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
    res = {"B": B, "temp": temp, "launches_per_window": a.launches, "reps": reps, "widths": {}}
    rng = np.random.RandomState(0)
    y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
    eps, g = (torch.as_tensor(rng.randn(B, side, side, 4).astype(np.float32)).cuda() for _ in range(2))
    x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
    nll, gt = (torch.empty((B,), device="cuda") for _ in range(2))
    o1, o2, o3 = (torch.empty_like(y) for _ in range(3))

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for width in [int(q) for q in a.widths.split(",") if q]:
        m = NoiseFlow([side, side, 4], False, default_hps(arch=FULL_ARCH, width=width), device=0, sample_vjp_kernel="gemm")
        lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
        assert lib.nf_sample_vjp_path(h) == _lib.NF_SVJP_PATH_GEMM and lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_GEMM
        _lib.check(lib.nf_reserve_sample_vjp_workspace(h, B, 1))
        calls = {
            "sample": lambda: _lib.check(lib.nf_sample(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), o1.data_ptr(), st)),
            "nll_grad": lambda: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(), o1.data_ptr(),
                                                           o2.data_ptr(), st)),
            "vjp": lambda: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None, g.data_ptr(),
                                                        o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), gt.data_ptr(), st)),
        }
        for fn in calls.values():
            window(fn, max(a.launches // 4, 2))
        wins = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                wins[k].append(window(fn, a.launches))
        med = {k: sorted(w)[len(w) // 2] for k, w in wins.items()}
        wp = 64 if width <= 64 else 128 if width <= 128 else 256 if width <= 256 else 512
        flop = 3.0 * 8 * B * side * side * 2.0 * (18 * wp + wp * wp + 36 * wp)   # three CNN evaluations per coupling, padded width
        r = {"ms": med, "windows": wins, "spread_ms": {k: max(w) - min(w) for k, w in wins.items()},
             "vjp_over_nll_grad": med["vjp"] / med["nll_grad"], "vjp_over_sample": med["vjp"] / med["sample"],
             "vjp_peak_fraction": flop / (med["vjp"] * 1e-3) / 157.3e12, "nll_grad_peak_fraction": flop / (med["nll_grad"] * 1e-3) / 157.3e12}
        res["widths"][str(width)] = r
        fmt = lambda w: "/".join("%.3f" % q for q in w)   # noqa: E731
        print("width %d  nf_sample %.3f ms [%s]   nf_nll_grad %.3f ms [%s]   nf_sample_vjp %.3f ms [%s]\n"
              "          vjp / nll_grad %.3f   vjp / sample %.2f   of the fp32 matrix peak: vjp %.2f, nll_grad %.2f"
              % (width, med["sample"], fmt(wins["sample"]), med["nll_grad"], fmt(wins["nll_grad"]), med["vjp"], fmt(wins["vjp"]),
                 r["vjp_over_nll_grad"], r["vjp_over_sample"], r["vjp_peak_fraction"], r["nll_grad_peak_fraction"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=4, help="4: the shipped model (default); 32: the deep model at width 32")
    ap.add_argument("--kernel", default="scalar", help="with --width 32: 'mfma' = sample_vjp_kernel='mfma'")
    ap.add_argument("--reps", type=int, default=None, help="rounds of alternated arms (default 4; --legs tiled: 3)")
    ap.add_argument("--ab-sides", default="24,16")
    ap.add_argument("--legs", default="whole", help="'whole' (default): the whole-patch kernels; 'tiled': the tile mode on 256x256 x 16 and 1024x1024 x 1")
    ap.add_argument("--widths", default="64,128,512", help="--kernel gemm: the coupling widths")
    ap.add_argument("--batch", type=int, default=1024, help="--kernel gemm: patches per launch")
    a = ap.parse_args()
    if a.kernel == "gemm":
        return gemm_legs(a)
    if a.reps is None:
        a.reps = 3 if a.legs == "tiled" else 4
    if a.legs not in ("whole", "tiled"):
        raise SystemExit("--legs whole or --legs tiled")
    if (a.width, a.kernel) not in ((4, "scalar"), (32, "mfma")):
        raise SystemExit("--width 4 [--kernel scalar] or --width 32 --kernel mfma")
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

    if a.legs == "tiled":
        if (a.width, a.kernel) != (4, "scalar"):
            raise SystemExit("--legs tiled times the shipped model")
        res = tiled_legs(a, v, cond, temp)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return

    res = {"B": B, "temp": temp, "launches_per_window": a.launches, "shapes": {}}
    wide = a.width == 32
    if wide:
        v = deep_variables(32)
        cond = _lib.nf_cond(800.0, 2.0, 0.0, 0.0)
        res["model"] = "deep_variables(32)"
    for side in ((32,) if wide else (32, 64)):
        if wide:
            m = NoiseFlow([side, side, 4], False, default_hps(arch=FULL_ARCH, width=32), variables=v, device=0, sample_vjp_kernel="mfma")
            assert m._flow.lib.nf_sample_vjp_path(m._flow.ptr) == _lib.NF_SVJP_PATH_WIDE32
            assert m._flow.lib.nf_grad_path(m._flow.ptr) == _lib.NF_GRAD_PATH_WIDE32
        else:
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
    # the matrix-core kernel against the scalar one where both hold the shape: arms alternated, differences against the spread
    for side in ([int(q) for q in a.ab_sides.split(",") if q] if wide else []):
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        eps, g = (torch.as_tensor(rng.randn(B, side, side, 4).astype(np.float32)).cuda() for _ in range(2))
        gt = torch.empty((B,), device="cuda")
        o1, o2, o3 = (torch.empty_like(y) for _ in range(3))
        arms = {}
        for name in ("mfma", "scalar"):
            m = NoiseFlow([side, side, 4], False, default_hps(arch=FULL_ARCH, width=32), variables=v, device=0, sample_vjp_kernel=name)
            assert m._flow.lib.nf_sample_vjp_path(m._flow.ptr) == (_lib.NF_SVJP_PATH_WIDE32 if name == "mfma" else _lib.NF_SVJP_PATH_SCALAR)
            arms[name] = m
        med = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, m in arms.items():
                lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
                med[name].append(timed(lambda: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None,
                                                                            g.data_ptr(), o1.data_ptr(), o2.data_ptr(), o3.data_ptr(),
                                                                            gt.data_ptr(), st)))[0])
        mid = {name: sorted(w)[len(w) // 2] for name, w in med.items()}
        spread = {name: max(w) - min(w) for name, w in med.items()}
        diff, noise = mid["mfma"] - mid["scalar"], 2.0 * max(spread.values())
        res["shapes"]["ab %dx%d" % (side, side)] = {"medians_ms": med, "median_ms": mid, "spread_ms": spread, "mfma_minus_scalar_ms": diff,
                                                    "twice_spread_ms": noise, "mfma_over_scalar": mid["mfma"] / mid["scalar"]}
        print("%dx%d  nf_sample_vjp  mfma %.4f ms [%s]   scalar %.4f ms [%s]   mfma - scalar %+.4f ms (2 x spread %.4f: %s)   mfma / scalar %.3f"
              % (side, side, mid["mfma"], "/".join("%.4f" % q for q in med["mfma"]), mid["scalar"], "/".join("%.4f" % q for q in med["scalar"]),
                 diff, noise, "a difference" if abs(diff) > noise else "inside the noise", mid["mfma"] / mid["scalar"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def tiled_legs(a, v, cond, temp):
    """--legs tiled (module docstring) → the result record."""
    import numpy as np
    import torch
    from noise_flow_amd import NoiseFlow, _lib, default_hps

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    res = {"temp": temp, "launches_per_window": a.launches, "rounds": a.reps, "shapes": {}}
    keep = os.environ.get("NF_GRAD_TILE_SEGMENTS")
    for side, B in ((256, 16), (1024, 1)):
        rng = np.random.RandomState(0)
        y = torch.as_tensor(rng.rand(B, side, side, 4).astype(np.float32)).cuda()
        eps, g = (torch.as_tensor(rng.randn(B, side, side, 4).astype(np.float32)).cuda() for _ in range(2))
        x = torch.as_tensor((rng.randn(B, side, side, 4) * 0.02).astype(np.float32)).cuda()
        nll, gt = (torch.empty((B,), device="cuda") for _ in range(2))
        o1, o2, o3 = (torch.empty_like(y) for _ in range(3))
        arms = {}
        for S in (8, 4, 3):
            os.environ["NF_GRAD_TILE_SEGMENTS"] = str(S)
            m = NoiseFlow([side, side, 4], False, default_hps(), variables=v, device=0, sample_vjp_tiles=True)
            lib, h, st = m._flow.lib, m._flow.ptr, m._dev.stream_ptr()
            assert lib.nf_sample_vjp_path(h) == _lib.NF_SVJP_PATH_TILED and lib.nf_grad_path(h) == _lib.NF_GRAD_PATH_TILED
            _lib.check(lib.nf_reserve_workspace(h, B, 1))
            _lib.check(lib.nf_reserve_grad_workspace(h, B, 1))
            _lib.check(lib.nf_reserve_sample_vjp_workspace(h, B, 1))
            calls = {
                "sample": lambda lib=lib, h=h, st=st: _lib.check(lib.nf_sample(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond),
                                                                               o1.data_ptr(), st)),
                "nll_grad": lambda lib=lib, h=h, st=st: _lib.check(lib.nf_nll_grad(h, x.data_ptr(), y.data_ptr(), B, C.byref(cond), None, nll.data_ptr(),
                                                                                   o1.data_ptr(), o2.data_ptr(), st)),
                "vjp": lambda lib=lib, h=h, st=st: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None,
                                                                                g.data_ptr(), o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), gt.data_ptr(), st)),
                "vjp_no_x": lambda lib=lib, h=h, st=st: _lib.check(lib.nf_sample_vjp(h, y.data_ptr(), eps.data_ptr(), 0, 0, temp, B, C.byref(cond), None,
                                                                                     g.data_ptr(), None, o2.data_ptr(), o3.data_ptr(), gt.data_ptr(), st)),
            }
            for fn in calls.values():
                window(fn, max(a.launches // 4, 10))
            arms[S] = (m, calls, {k: [] for k in calls})
        for _ in range(a.reps):      # the arms alternated
            for S, (m, calls, w) in arms.items():
                for k, fn in calls.items():
                    w[k].append(window(fn, a.launches))
        shape = {}
        for S, (m, calls, w) in arms.items():
            med = {k: sorted(q)[len(q) // 2] for k, q in w.items()}
            shape["S=%d" % S] = {"median_ms": med, "windows_ms": w, "vjp_over_nll_grad": med["vjp"] / med["nll_grad"],
                                 "vjp_no_x_over_nll_grad": med["vjp_no_x"] / med["nll_grad"], "vjp_over_sample": med["vjp"] / med["sample"],
                                 "pixels_per_s": B * side * side / med["vjp"] * 1e3}
            fmt = lambda q: "/".join("%.4f" % t for t in q)   # noqa: E731
            print("%dx%d x %d  S = %d  nf_sample %.4f ms [%s]   nf_nll_grad %.4f ms [%s]\n"
                  "       nf_sample_vjp %.4f ms [%s] (%.3e pixels/s), x_out = NULL %.4f ms [%s]   vjp / nll_grad %.3f   x_out = NULL / nll_grad %.3f   "
                  "vjp / sample %.2f" % (side, side, B, S, med["sample"], fmt(w["sample"]), med["nll_grad"], fmt(w["nll_grad"]), med["vjp"], fmt(w["vjp"]),
                                         shape["S=%d" % S]["pixels_per_s"], med["vjp_no_x"], fmt(w["vjp_no_x"]), shape["S=%d" % S]["vjp_over_nll_grad"],
                                         shape["S=%d" % S]["vjp_no_x_over_nll_grad"], shape["S=%d" % S]["vjp_over_sample"]), flush=True)
        res["shapes"]["%dx%d x %d" % (side, side, B)] = shape
    if keep is None:
        os.environ.pop("NF_GRAD_TILE_SEGMENTS", None)
    else:
        os.environ["NF_GRAD_TILE_SEGMENTS"] = keep
    return res


FULL_ARCH = "sdn5|unc|unc|unc|unc|gain4|unc|unc|unc|unc"


def deep_variables(width, seed=0):
    """The deep model of tests/sample_vjp_wide_cases.py, value for value (conftest.trained_like_variables with l_2/W and l_last/W
    multiplied by sqrt(4 / width), then by 0.5), restated here so that the tool stands without the test modules."""
    import numpy as np
    from noise_flow_amd import params
    rng = np.random.RandomState(seed + 1000)
    v = params.init_variables(FULL_ARCH, width, 4, seed)
    f = np.float32(np.sqrt(4.0 / width))
    for k in list(v):
        a = v[k]
        if k.endswith("l_1/W"):
            v[k] = (rng.randn(*a.shape) * 0.4).astype(np.float32)
        elif k.endswith("l_2/W"):
            v[k] = (((rng.randn(*a.shape) * 0.4).astype(np.float32) * f).astype(np.float32) * np.float32(0.5)).astype(np.float32)
        elif k.endswith("l_last/W"):
            v[k] = (((rng.randn(*a.shape) * 0.15).astype(np.float32) * f).astype(np.float32) * np.float32(0.5)).astype(np.float32)
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


if __name__ == "__main__":
    main()
