"""Record tests/golden/wide_family_bits.npz: the bits the width-16 / 32 matrix-core kernels (csrc/nf_wide.hip, nf_wide16.hip) give
today on the cases of tests/test_gpu_wide_bits.py (an MI355X is needed).

    python tools/make_golden_wide_bits.py [out.npz]

The fixture pins the kernels' per-patch outputs across rewrites that move code without changing a product, an addition order or
a rounding point, so it is recorded from the build of the commit BEFORE such a rewrite and never from the code under test (the
test module names the commit)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from test_gpu_wide_bits import GOLDEN, compute_outputs
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = compute_outputs()
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s (%d bytes, %d arrays)" % (out, size, len(arrays)))
    assert size < 512 * 1024, "the fixture has to stay under 512 KiB"


if __name__ == "__main__":
    main()
