"""Record tests/golden/trainer_host_bits.npz: the bits the training step and the batch-statistics evaluator give on the cases of
tests/test_gpu_trainer_bits.py (an MI355X is needed: the grids depend on the CU count).

    python tools/make_golden_trainer_bits.py [out.npz] [--compare other.npz]

The fixture pins the trainer across rewrites of its host orchestration that keep every launch, grid and operand, so it is recorded
from the build of the commit BEFORE such a rewrite and never from the code under test (the test module names the commit).  Every
case is run twice and has to give the same bits both times before anything is written; no case is dropped.  --compare: after
recording, hold the new file against another one (a fixture recorded from another build) and fail on any differing bit."""
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
    out = args[0] if args else GOLDEN
    arrays, unstable = {}, []
    for case in CASES:
        first, second = case_outputs(case), case_outputs(case)
        bad = differing(second, first)
        unstable += bad
        arrays.update(first)
        print("%s: %d arrays, %s" % (case["id"], len(first), "two runs DIFFER in %r" % bad if bad else "the same bits twice"), flush=True)
    assert not unstable, "two runs of the same build differ in %r" % unstable
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s (%d bytes, %d arrays, %d cases)" % (out, size, len(arrays), len(CASES)))
    assert size < 512 * 1024, "the fixture has to stay under 512 KiB"
    if compare:
        with np.load(compare) as f:
            other = {k: f[k] for k in f.files}
        bad = differing(arrays, other)
        assert not bad, "differs from %s in %r" % (compare, bad)
        print("identical to %s" % compare)


if __name__ == "__main__":
    main()
