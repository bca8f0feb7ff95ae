"""Kernel launches of the batch-statistics calls, per case, for comparing two builds of the host code.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/batchstats_launches.py run     (a run of its own, no counters)
    NF_KERNEL=valu rocprofv3 ... -d <dir_valu> -- python tools/batchstats_launches.py run                (the cases of that mode)
    python tools/batchstats_launches.py list <dir> [<dir_valu>] > launches.txt

`run` makes, once each, the four calls of every case of tests/test_gpu_batchstats_bits.py and one NLL call of every row of
tests/test_gpu_batchstats_route.py whose NF_KERNEL mode is this process's (NF_TOOL_LIB selects another build of the library).  In
front of each it launches a separator — nf_sample_eps for one patch of one pixel — so that `list` can cut the trace into cases
without a second tracing mode.  `list` prints, per case and in dispatch order, kernel | grid | workgroup of every launch that is
not PyTorch's own (at::...), with runs of one launch folded into a count; two builds launch the same if the two outputs are
equal (diff)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def jobs(kernel):
    """[(title, function)] of this NF_KERNEL mode, in a fixed order."""
    import test_gpu_batchstats_bits as bits
    import test_gpu_batchstats_route as route
    from test_gpu_trainer_bits import _env
    out = []
    for case in bits.CASES:
        if case["kernel"] == kernel:
            def f(case=case):
                with _env(case["env"]):
                    bits._run(case, {})
            out.append(("bits case %s: %s, width %d, %dx%d, B = %d: nll, inverse, sample(eps), sample(seed)" % (
                case["id"], case["arch"], case["width"], case["hw"][0], case["hw"][1], case["B"]), f))
    for row in route.ROWS:
        if row[4] == kernel:
            def g(row=row):
                from conftest import make_inputs
                w, H, W, env, _, _ = row
                x, y = make_inputs(2, H, W, seed=3)
                m = route.make_model(w, H, W)
                with _env(env):
                    m._loss(x, y, [0.0], [0.0], [400], [1])
            out.append(("route row %s (%s, B = 2): nll; expected route %s" % (route.row_key(row), route.ARCH,
                                                                               ("MFMA4", "SCALAR", "TRAINER")[row[5]]), g))
    return out


def run():
    import torch
    from noise_flow_amd import _lib
    if os.environ.get("NF_TOOL_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])
    lib = _lib.load()
    sep = torch.zeros(4, device="cuda")
    for title, f in jobs(os.environ.get("NF_KERNEL") or None):
        torch.cuda.synchronize()
        _lib.check(lib.nf_sample_eps(1, 0, 1, 1, 1, sep.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        try:
            f()
            print(title, flush=True)
        except _lib.NoiseFlowLibError as e:      # a refusal of the library is a result; anything else ends the run
            print("%s: REFUSED: %s" % (title, e), flush=True)
    torch.cuda.synchronize()


def _rows(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, "expected one kernel trace under %s, found %r" % (d, files)
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "")
        if "at::" in name or name.startswith("__amd_rocclr"):
            continue
        name = name.split("(")[0].replace(" [clone .kd]", "").replace(".kd", "")
        dims = lambda p: "x".join(r[p + s] for s in ("_X", "_Y", "_Z")) if (p + "_X") in r else r[p]
        out.append("%s | grid %s | wg %s" % (name, dims("Grid_Size"), dims("Workgroup_Size")))
    return out


def listing(dirs):
    for d, kernel in zip(dirs, (None, "valu")):
        rows = _rows(d)
        sep = rows[0]      # the first launch of the library is the first separator
        chunks = []
        for r in rows:
            if r == sep:
                chunks.append([])
            else:
                chunks[-1].append(r)
        titles = [t for t, _ in jobs(kernel)]
        assert len(chunks) == len(titles), "%d separators (%s) for %d cases" % (len(chunks), sep, len(titles))
        for title, chunk in zip(titles, chunks):
            print("== %s%s: %d launches" % ("NF_KERNEL=valu, " if kernel else "", title, len(chunk)))
            i = 0
            while i < len(chunk):
                j = i
                while j < len(chunk) and chunk[j] == chunk[i]:
                    j += 1
                print("  %3d x %s" % (j - i, chunk[i]))
                i = j


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) in (3, 4):
        listing(sys.argv[2:])
    else:
        sys.exit(__doc__)
