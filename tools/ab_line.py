"""One line of an A/B log from a bench.py result:   python tools/ab_line.py <arm> <rep> <bench.json>
(`value`, step and kernel time of the headline; with a --full result also the sampling and sharded_1m sections)."""
import json
import sys

arm, rep, path = sys.argv[1:4]
r = json.loads([l for l in open(path) if l.startswith("{")][-1])
print("%s rep%s value %.6e patches/s  ms_per_step %.5f  kernel_ms %.5f" % (arm, rep, r["value"], r["ms_per_step"], r["roofline"]["kernel_ms"]))
for sec in ("sampling", "sharded_1m"):
    s = r.get(sec)
    if isinstance(s, dict) and "value" in s:
        print("%s %s %s value %.6e  ms_per_step %.5f" % (arm, rep, sec, s["value"], s.get("ms_per_step", float("nan"))))
