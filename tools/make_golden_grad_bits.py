"""Record tests/golden/grad_family_bits.npz: the bits the four gradient kernels (csrc/nf_grad.hip, nf_grad_wide.hip, nf_grad_gemm.hip,
nf_sample_grad.hip) give today on the cases of tests/test_gpu_grad_bits.py (an MI355X is needed).

    [NF_TOOL_LIB=/path/to/libnoiseflow_hip.so] python tools/make_golden_grad_bits.py [out.npz] [--compare other.npz]

The fixture pins the kernels' per-patch outputs across rewrites that move code without changing a product, an addition order, a
rounding point or a launch, so it is recorded from the build of the commit BEFORE such a rewrite (NF_TOOL_LIB selects that build's
library) and never from the code under test (the test module names the commit).  Every case is run twice and has to give the same
bits both times.  --compare: say whether every array has the bytes of that file's (the parent's build against the fixture, or
two builds against each other); exit status 1 if one differs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if os.environ.get("NF_TOOL_LIB"):
        from noise_flow_amd import _lib
        _lib.LIB_PATH = os.path.abspath(os.environ["NF_TOOL_LIB"])
    from test_gpu_grad_bits import GOLDEN, compute_outputs
    args = sys.argv[1:]
    other = None
    if "--compare" in args:
        i = args.index("--compare")
        other = args[i + 1]
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    arrays, again = compute_outputs(), compute_outputs()
    assert sorted(arrays) == sorted(again)
    unstable = [k for k in arrays if arrays[k].tobytes() != again[k].tobytes()]
    assert not unstable, "two runs disagree: %s" % unstable
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s (%d bytes, %d arrays), two runs with the same bits" % (out, size, len(arrays)))
    assert size < 512 * 1024, "the fixture has to stay under 512 KiB"
    if other:
        ref = np.load(other)
        differs = [k for k in arrays if k not in ref.files or arrays[k].tobytes() != ref[k].tobytes()] + [k for k in ref.files if k not in arrays]
        print("against %s: %d arrays, %d differ %s" % (other, len(arrays), len(differs), differs[:8]))
        sys.exit(1 if differs else 0)


if __name__ == "__main__":
    main()
