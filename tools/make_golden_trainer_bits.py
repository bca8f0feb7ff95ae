"""Record tests/golden/trainer_host_bits.npz: the bits the training step and the batch-statistics evaluator give on the cases of
tests/test_gpu_trainer_bits.py (an MI355X is needed: the grids depend on the CU count).

    python tools/make_golden_trainer_bits.py [out.npz] [--compare other.npz] [--only PREFIX --into old.npz]

The fixture pins the trainer across rewrites of its host orchestration that keep every launch, grid and operand, so it is recorded
from the build of the commit BEFORE such a rewrite and never from the code under test (the test module names the commit).  Every
case is run twice and has to give the same bits both times before anything is written; no case is dropped.  --compare: after
recording, hold the new file against another one (a fixture recorded from another build) and fail on any differing bit.
--only PREFIX --into old.npz: record only the cases whose id starts with PREFIX and write them together with the arrays of old.npz,
which are taken over as they are (cases added later are recorded from THEIR parent commit; the earlier ones keep theirs)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from test_gpu_trainer_bits import CASES, GOLDEN, case_outputs, differing
    args = sys.argv[1:]
    compare = None
    if "--compare" in args:
        i = args.index("--compare")
        compare = args[i + 1]
        del args[i:i + 2]
    only, arrays = "", {}
    if "--only" in args:
        i = args.index("--only")
        only = args[i + 1]
        del args[i:i + 2]
        i = args.index("--into")
        with np.load(args[i + 1]) as f:
            arrays = {k: f[k] for k in f.files}
        del args[i:i + 2]
        assert not [k for k in arrays if k.startswith(only)], "%s already holds cases that start with %r" % ("old.npz", only)
    out = args[0] if args else GOLDEN
    cases = [c for c in CASES if c["id"].startswith(only)]
    unstable = []
    for case in cases:
        first, second = case_outputs(case), case_outputs(case)
        bad = differing(second, first)
        unstable += bad
        arrays.update(first)
        print("%s: %d arrays, %s" % (case["id"], len(first), "two runs DIFFER in %r" % bad if bad else "the same bits twice"), flush=True)
    assert not unstable, "two runs of the same build differ in %r" % unstable
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s (%d bytes, %d arrays, %d cases)" % (out, size, len(arrays), len(cases)))
    assert size < 512 * 1024, "the fixture has to stay under 512 KiB"
    if compare:
        with np.load(compare) as f:
            other = {k: f[k] for k in f.files}
        bad = differing(arrays, other)
        assert not bad, "differs from %s in %r" % (compare, bad)
        print("identical to %s" % compare)


if __name__ == "__main__":
    main()
