"""Record tests/golden/split_bf16_runs.npz: the bits the split-bf16 flow kernel gives today on the cases of
tests/test_gpu_split_bf16_runs.py (an MI355X is needed).

    python tools/make_golden_split_bf16_runs.py [out.npz]

The fixture pins the kernel's outputs across rewrites that change addressing and scheduling only, so it is recorded from the
build of the commit BEFORE such a rewrite and never from the code under test (the test module names the commit)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from test_gpu_split_bf16_runs import GOLDEN, compute_outputs
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = compute_outputs()
    np.savez_compressed(out, **arrays)
    print("wrote %s (%d bytes): %s" % (out, os.path.getsize(out), ", ".join("%s %s" % (k, v.shape) for k, v in arrays.items())))


if __name__ == "__main__":
    main()
