"""Which kernel family a handle launches, per direction, over a grid of widths x patch shapes x nf_config.flags x switches.

tests/golden/kernel_path_table.json holds nf_kernel_path(h, 0) and nf_kernel_path(h, 1) — the value of the one function the
launches themselves dispatch on (csrc/nf_host.hip: select_path) — for handles created over the grid, or nf_create's return code
where it refuses the model.  Recorded on an MI355X from the build of the commit BEFORE the three hand-written copies of the
decision were merged (the file names it), by

    python tests/test_gpu_kernel_path_table.py --record <commit>

Only nf_create / nf_kernel_path / nf_destroy are called: no kernel is launched.  NF_KERNEL=valu is read once per process, so
that column is computed (recorded and checked) in one fresh child process.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "kernel_path_table.json")
SWITCHES = ("NF_GEMM", "NF_GEMM16", "NF_H16", "NF_TILE_SEGMENTS")


def grid():
    """(width, H, W, flags, env): the widths, shapes and flags of tests/test_fold_layout_digests_cpu.py plus 200x64 (tiled in one
    dimension only), and the three switches on the cases each touches."""
    from test_fold_layout_digests_cpu import SHAPES, WIDTHS, _flags
    f0, f16, fex = _flags()
    out = [(w, H, W, fl, "") for w in WIDTHS for (H, W) in SHAPES + ((200, 64),) for fl in (f0, f16, fex)]
    for w in (40, 96):
        for hw in ((16, 16), (32, 32), (64, 64), (128, 128)):
            out.append((w,) + hw + (f0, "NF_GEMM=a"))
            out.append((w,) + hw + (f16, "NF_GEMM16=a"))
    for w in (3, 4):
        for hw in ((5, 9), (32, 32), (64, 64), (128, 128), (200, 64)):
            out.append((w,) + hw + (f16, "NF_H16=4x4"))
    return out


def compute_column():
    """{case: [path of direction 0, path of direction 1]} or {case: [nf_create's return code]} in THIS process's NF_KERNEL mode."""
    from noise_flow_amd import _lib
    from test_fold_layout_digests_cpu import MAIN, model
    lib = _lib.load()
    keep = {k: os.environ.pop(k, None) for k in SWITCHES}
    out = {}
    try:
        for w, H, W, fl, env in grid():
            descs, flat = model(*MAIN, w)
            cfg = _lib.nf_config(H, W, 4, len(descs), -1, fl)
            if env:
                name, value = env.split("=")
                os.environ[name] = value
            try:
                h = C.c_void_p()
                rc = lib.nf_create(C.byref(cfg), descs, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size, C.byref(h))
            finally:
                if env:
                    del os.environ[name]
            key = "w%d;%dx%d;f%d;%s" % (w, H, W, fl, env)
            if rc != 0:
                out[key] = [rc]
                continue
            out[key] = [lib.nf_kernel_path(h, 0), lib.nf_kernel_path(h, 1)]
            assert lib.nf_destroy(h) == 0
    finally:
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    return out


def child_column(nf_kernel):
    """The column of a fresh process started with NF_KERNEL=<nf_kernel>; nothing further runs if the child dies."""
    env = dict(os.environ, NF_KERNEL=nf_kernel)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--column"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child exited with %d\n%s%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def _compare(got, want, recorded_from):
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, "%d of %d handles choose another kernel path than %s: (got, recorded) %r" % (
        len(bad), len(got), recorded_from, dict(list(bad.items())[:8]))


@pytest.mark.gpu
def test_kernel_path_of_every_handle_of_the_grid():
    assert "NF_KERNEL" not in os.environ, "this column is the default (matrix-core) mode"
    with open(GOLDEN) as f:
        g = json.load(f)
    got = compute_column()
    _compare(got, g["default"], g["recorded_from"])
    assert {p for v in got.values() if len(v) == 2 for p in v} == set(range(9)), "the grid must reach all nine families"


@pytest.mark.gpu
def test_kernel_path_of_every_handle_of_the_grid_under_nf_kernel_valu():
    with open(GOLDEN) as f:
        g = json.load(f)
    _compare(child_column("valu"), g["valu"], g["recorded_from"])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    if sys.argv[1:2] == ["--column"]:
        print(json.dumps(compute_column(), separators=(",", ":"), sort_keys=True))
    elif sys.argv[1:2] == ["--record"] and len(sys.argv) >= 3:
        out = sys.argv[3] if len(sys.argv) > 3 else GOLDEN
        os.environ.pop("NF_KERNEL", None)
        table = {"recorded_from": sys.argv[2], "default": compute_column(), "valu": child_column("valu")}
        with open(out, "w") as f:
            json.dump(table, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print("wrote %s (%d bytes, %d handles per column)" % (out, os.path.getsize(out), len(table["default"])))
    else:
        sys.exit(__doc__)
