"""Record tests/golden/fold_layout_digests.json: digests of every program and parameter block the host program builder makes on
the grid of tests/test_fold_layout_digests_cpu.py (no GPU needed).

    python tools/make_golden_fold_digests.py <commit the library was built from> [out.json]

The fixture pins the builder's output across rewrites that move code without changing a float, so it is recorded from the build
of the commit BEFORE such a rewrite and never from the code under test; the commit is written into the file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from test_fold_layout_digests_cpu import GOLDEN, N_PATHS, compute_all
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    cases = compute_all()
    with open(out, "w") as f:
        json.dump({"recorded_from": sys.argv[1], "cases": cases}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    blocks = [sum(isinstance(v, str) for c in cases.values() for d in c.values() for v in d["paths"][p:p + 1]) for p in range(N_PATHS)]
    print("wrote %s (%d bytes, %d cases, blocks per path %s)" % (out, os.path.getsize(out), len(cases), blocks))
    assert os.path.getsize(out) < 512 * 1024, "the fixture has to stay under 512 KiB"


if __name__ == "__main__":
    main()
