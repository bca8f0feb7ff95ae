"""Per-patch conditioning: what it costs the per-call path, and what it buys a mixed minibatch.

    python tools/time_percond.py [--base build/variants/lib_parent.so] [--repeats 3] [--launches 200] [--out FILE.json]

1. Per-call headline shapes (shipped model, 32x32: nf_nll at B = 1 024, nf_sample with the in-kernel draw at B = 4 096) on two
   builds of the library, ALTERNATED `--repeats` times (one fresh process per arm and repeat, so neither build keeps a warm
   device to itself): `--base`, the library as it was before the per-patch entries existed (built from the parent commit into
   build/variants/, see tools/build_variant.sh), and the product's csrc/libnoiseflow_hip.so.  The product passes when its median
   is inside the spread the base shows against itself across its repeats.
2. The product alone: nf_nll_percond at B = 1 024 with 25 (ISO, camera) tuples against nf_nll at B = 1 024 with one tuple, and
   against what a caller had to do before: 25 nf_nll launches of 41 patches each, one per tuple.

Every figure is the mean over a window of `--launches` back-to-back launches between two device events, after a warm-up of a
quarter of that; a process takes three windows and reports their median.  The arms bind the C ABI themselves (ctypes), because
the base library does not export the new entries.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRODUCT = os.path.join(ROOT, "noise_flow_amd", "csrc", "libnoiseflow_hip.so")
ISOS, CAMS = (100, 400, 800, 1600, 3200), (0, 1, 2, 3, 4)


def child(lib_path, launches, percond):
    import numpy as np
    import torch
    from noise_flow_amd import _lib as L, params
    from noise_flow_amd.ckpt import load_checkpoint
    from noise_flow_amd.noise_flow_model import default_hps
    lib = C.CDLL(lib_path)
    vp, i64, u32, u64, f32 = C.c_void_p, C.c_int64, C.c_uint32, C.c_uint64, C.c_float
    lib.nf_create.argtypes = [C.POINTER(L.nf_config), C.POINTER(L.nf_layer_desc), C.POINTER(C.c_float), C.c_size_t, C.POINTER(vp)]
    lib.nf_nll.argtypes = [vp, vp, vp, i64, C.POINTER(L.nf_cond), vp, vp, vp, vp, vp, u32, vp]
    lib.nf_sample.argtypes = [vp, vp, vp, u64, i64, f32, i64, C.POINTER(L.nf_cond), vp, vp]
    lib.nf_destroy.argtypes = [vp]
    lib.nf_last_error.restype = C.c_char_p
    hps = default_hps()
    v = load_checkpoint(os.path.join(ROOT, "models", "NoiseFlow", "ckpt", "model.ckpt.best"))
    layers, descs, flat = params.pack(hps.arch, v, hps.width, "loss_first")
    cfg = L.nf_config(32, 32, 4, len(layers), 0, 0)
    fp = flat.ctypes.data_as(C.POINTER(C.c_float))
    h = vp()
    assert lib.nf_create(C.byref(cfg), descs, fp, flat.size, C.byref(h)) == 0, lib.nf_last_error()
    torch.cuda.set_device(0)
    st = int(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(0)
    BN, BS = 1024, 4096
    y = torch.as_tensor(rng.rand(BS, 32, 32, 4).astype(np.float32)).cuda()
    x = torch.as_tensor((rng.randn(1025, 32, 32, 4) * 0.02).astype(np.float32)).cuda()
    nll, sd, ld = (torch.empty((1025,), device="cuda") for _ in range(3))
    out = torch.empty_like(y)
    cond = L.nf_cond(100.0, 2.0, 0.0, 0.0)

    def ok(rc):
        assert rc == 0, lib.nf_last_error()

    def timed(fn):
        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        window(max(launches // 4, 10))
        return sorted(window(launches) for _ in range(3))[1]

    res = {"lib": lib_path}
    res["nll_1024_ms"] = timed(lambda: ok(lib.nf_nll(h, x.data_ptr(), y.data_ptr(), BN, C.byref(cond), nll.data_ptr(), sd.data_ptr(),
                                                     ld.data_ptr(), None, None, 0, st)))
    res["sample_4096_ms"] = timed(lambda: ok(lib.nf_sample(h, y.data_ptr(), None, 7, 0, 1.0, BS, C.byref(cond), out.data_ptr(), st)))
    if percond:
        lib.nf_cond_rows.argtypes = [C.POINTER(L.nf_config), C.POINTER(L.nf_layer_desc), C.POINTER(C.c_float), C.c_size_t, C.c_int32,
                                     C.POINTER(L.nf_cond), i64, C.POINTER(L.nf_cond_row)]
        lib.nf_nll_percond.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, u32, vp]
        tuples = [(i, c) for i in ISOS for c in CAMS]
        conds = (L.nf_cond * 25)(*[L.nf_cond(float(i), float(c), 0.0, 0.0) for i, c in tuples])
        rows25 = (L.nf_cond_row * 25)()
        ok(lib.nf_cond_rows(C.byref(cfg), descs, fp, flat.size, 0, conds, 25, rows25))
        r = np.frombuffer(rows25, np.uint8).reshape(25, 48)
        rows = torch.as_tensor(r[np.arange(BN) % 25].copy()).cuda()
        res["percond_1024x25_ms"] = timed(lambda: ok(lib.nf_nll_percond(h, x.data_ptr(), y.data_ptr(), BN, rows.data_ptr(), nll.data_ptr(),
                                                                        sd.data_ptr(), ld.data_ptr(), None, None, 0, st)))

        def grouped():   # what a mixed minibatch cost before: one launch per (ISO, camera) group, 25 x 41 patches
            for k in range(25):
                o = 41 * k
                ok(lib.nf_nll(h, x[o:].data_ptr(), y[o:].data_ptr(), 41, C.byref(conds[k]), nll[o:].data_ptr(), sd[o:].data_ptr(),
                              ld[o:].data_ptr(), None, None, 0, st))
        res["grouped_25x41_ms"] = timed(grouped)
    torch.cuda.synchronize()
    lib.nf_destroy(h)
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib_path, launches, percond):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path, "--launches", str(launches)] + (["--percond"] if percond else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("arm %s failed (exit %d):\n%s\n%s" % (lib_path, p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=os.path.join(ROOT, "build", "variants", "lib_parent.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--percond", action="store_true")
    a = ap.parse_args()
    if a.launches < 200 and not a.child:
        raise SystemExit("--launches must be at least 200")
    if a.child:
        return child(a.child, a.launches, a.percond)
    if not os.path.exists(a.base):
        raise SystemExit("%s is missing: build the parent commit's library there first (tools/build_variant.sh)" % a.base)
    arms = {"base": [], "product": []}
    for rep in range(max(a.repeats, 3)):      # a fault in one arm ends the run: run_child raises on a non-zero exit
        for arm, path in (("base", a.base), ("product", PRODUCT)):
            r = run_child(path, a.launches, arm == "product")
            arms[arm].append(r)
            print("%s rep %d: %s" % (arm, rep, json.dumps({k: round(v, 5) for k, v in r.items() if k != "lib"})), flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    summary = {"launches_per_window": a.launches, "repeats": max(a.repeats, 3), "arms": arms, "per_call": {}}
    for key in ("nll_1024_ms", "sample_4096_ms"):
        b = [r[key] for r in arms["base"]]
        p = [r[key] for r in arms["product"]]
        summary["per_call"][key] = {"base_min": min(b), "base_max": max(b), "base_spread_rel": (max(b) - min(b)) / med(b),
                                    "product_median": med(p), "product_vs_base_median": med(p) / med(b),
                                    "inside_base_spread": med(p) <= max(b)}
    pc, one, grp = (med([r[k] for r in arms["product"]]) for k in ("percond_1024x25_ms", "nll_1024_ms", "grouped_25x41_ms"))
    summary["mixed_batch"] = {"percond_1024x25_ms": pc, "per_call_1024x1_ms": one, "grouped_25x41_ms": grp,
                              "percond_patches_per_s": 1024 / pc * 1e3, "per_call_patches_per_s": 1024 / one * 1e3,
                              "grouped_patches_per_s": 1025 / grp * 1e3, "percond_over_per_call_time": pc / one,
                              "grouped_over_percond_time_per_patch": (grp / 1025) / (pc / 1024)}
    print(json.dumps({k: v for k, v in summary.items() if k != "arms"}, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
