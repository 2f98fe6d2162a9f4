"""Compare two loop-body dumps of iter_trace.py: python3 tools/cmp_body_trace.py A B

A dump merges the hardware queues by start time, so where queues run side by side its line order
moves from run to run.  What a build fixes is the launch sequence of each queue and which launches
share a queue; queue ids are the runtime's labels and are matched here by content.  Exit status 0
when those agree."""
import sys


def load(path):
    out = []
    for ln in open(path):
        f = ln.split(None, 3)
        out.append((f[2], f[3].rstrip("\n")))
    return out


def per_queue(trace):
    d = {}
    for q, name in trace:
        d.setdefault(q, []).append(name)
    return sorted(d.values())


a, b = load(sys.argv[1]), load(sys.argv[2])
print("%d and %d launches" % (len(a), len(b)))
first = next((i + 1 for i, (x, y) in enumerate(zip(a, b)) if x[1] != y[1]), None)
print("merged order: " + ("identical" if first is None and len(a) == len(b)
                           else "differs from line %s" % first))
same = per_queue(a) == per_queue(b)
print("per-queue launch sequences and queue membership: " + ("identical" if same else "DIFFERENT"))
sys.exit(0 if same else 1)
