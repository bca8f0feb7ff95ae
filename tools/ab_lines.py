"""Two arms of an A/B session, line by line:   python tools/ab_lines.py <name A> <logs of A ...> -- <name B> <logs of B ...>

Every log is the output of one run of a timing tool that prints `<label>  <x> ms/call ...` lines (tools/time_batchstats.py,
tools/time_batchstats_width.py), the runs of the two arms alternated in one session.  Per label: each arm's figures, mean and spread
(max - min over its runs), and the verdict of the project's rule — B is slower only if its mean exceeds A's by more than twice
the larger in-arm spread.  Exit status 1 if any line is slower."""
import re
import sys


def read(paths):
    out = {}
    for p in paths:
        for line in open(p):
            m = re.match(r"(.*?)\s+([0-9.]+) ms/call", line)
            if m:
                out.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
    return out


def main():
    args = sys.argv[1:]
    cut = args.index("--")
    (na, *pa), (nb, *pb) = args[:cut], args[cut + 1:]
    A, B = read(pa), read(pb)
    assert list(A) == list(B) and len(pa) == len(pb), "the two arms hold different lines or run counts"
    slower = 0
    print("ms/call; %d runs per arm, alternated; spread = max - min of an arm's runs" % len(pa))
    for label in A:
        a, b = A[label], B[label]
        ma, mb = sum(a) / len(a), sum(b) / len(b)
        sa, sb = max(a) - min(a), max(b) - min(b)
        bad = mb - ma > 2 * max(sa, sb)
        slower += bad
        print("%s\n    %-8s %s  mean %.4f  spread %.4f\n    %-8s %s  mean %.4f  spread %.4f\n    %s - %s = %+.4f ms against 2 x %.4f: %s" % (
            label, na, " ".join("%.3f" % v for v in a), ma, sa, nb, " ".join("%.3f" % v for v in b), mb, sb, nb, na, mb - ma,
            max(sa, sb), "SLOWER" if bad else "not slower"))
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
