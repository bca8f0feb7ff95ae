"""Record tests/golden/batchstats_host_bits.npz: the bits nf_nll_batchstats / nf_sample_batchstats give on the cases of
tests/test_gpu_batchstats_bits.py (an MI355X is needed).

    [NF_TOOL_LIB=build/variants/lib_<parent>.so] python tools/make_golden_batchstats_bits.py [out.npz] [--compare other.npz]

The fixture pins the calls across rewrites of their host code that keep every launch and operand, so it is recorded from the build
of the commit BEFORE such a rewrite (NF_TOOL_LIB; the test module names the commit) and never from the code under test; the
library needs no nf_batchstats_route.  Every case is run twice, in two processes, and has to give the same bits both times.  A case
whose bits are fixed by construction (the test module's docstring) that differs fails the recording; a `generic` case that differs is
left out of the fixture and named — take it out of the test's table with that reason.  --compare: hold the new file against
another one (recorded from another build) and fail on any differing bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record_all(out):
    """This process: every case of the table once (a case of another NF_KERNEL mode in its own child)."""
    from test_gpu_batchstats_bits import CASES, case_outputs
    arrays = {}
    for case in CASES:
        res, route = case_outputs(case)
        arrays.update(res)
        print("%s: %d arrays%s" % (case["id"], len(res), "" if route is None else ", route %d" % route), flush=True)
        assert route is None or route == case["route"], (case["id"], route)
    np.savez(out, **arrays)


def main():
    if os.environ.get("NF_TOOL_LIB"):
        from noise_flow_amd import _lib
        _lib.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])
    args = sys.argv[1:]
    if args[:1] == ["--one-pass"]:
        return record_all(args[1])
    from test_gpu_batchstats_bits import CASES, GOLDEN, differing
    compare = None
    if "--compare" in args:
        i = args.index("--compare")
        compare = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k in range(2):      # two processes; nothing further runs on the GPU if one of them dies
            p = os.path.join(d, "pass%d.npz" % k)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one-pass", p], check=True, timeout=900)
            with np.load(p) as f:
                runs.append({key: f[key] for key in f.files})
    bad = differing(runs[1], runs[0])
    dropped = sorted({key.split("__")[0] for key in bad})
    generic = {c["id"] for c in CASES if c["generic"]}
    assert set(dropped) <= generic, "cases that are reproducible by construction differ between two processes: %r" % bad
    arrays = {key: a for key, a in runs[0].items() if key.split("__")[0] not in dropped}
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s (%d bytes, %d arrays, %d of %d cases)" % (out, size, len(arrays), len(CASES) - len(dropped), len(CASES)))
    print("left out (two recordings of one build differ): %s" % (", ".join(dropped) or "none"))
    assert size < 512 * 1024, "the fixture has to stay under 512 KiB"
    if compare:
        with np.load(compare) as f:
            other = {key: f[key] for key in f.files}
        bad = differing(arrays, other)
        assert not bad, "differs from %s in %r" % (compare, bad)
        print("identical to %s" % compare)


if __name__ == "__main__":
    main()
