#!/usr/bin/env python3
"""Kernel summary of a `rocprofv3 --kernel-trace --stats` run as CSV, plus how much the launches overlap.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python bench.py --only-headline --no-parity --no-cpu-baseline
    python tools/rocprof_overlap.py OUT/run_results.db > profiles/NAME.csv

One row per kernel (calls, total / average / min / max duration in us, share of the summed kernel time) and, for the
step kernel, the figures that show what the pipelined rollout driver (include/bpp_pipeline.h) does: the summed duration
of its launches against the time during which at least one of them was running.  On one stream the two are equal; with
G chains a launch lasts longer, because it shares the chip, and the sum exceeds the busy time by the overlap."""
import csv
import sqlite3
import sys


def busy_ns(spans):
    """length of the union of [start, end) intervals"""
    total, cur_s, cur_e = 0, None, None
    for s, e in sorted(spans):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                total += cur_e - cur_s
            cur_s, cur_e = s, e
        elif e > cur_e:
            cur_e = e
    return total + (cur_e - cur_s if cur_e is not None else 0)


def main(path, out=sys.stdout):
    db = sqlite3.connect(path)
    rows = db.execute("select name, start, end, stream_id, queue_id from kernels").fetchall()
    by = {}
    for name, s, e, stream, queue in rows:
        by.setdefault(name, []).append((s, e, stream, queue))
    all_ns = sum(e - s for v in by.values() for s, e, _, _ in v)
    w = csv.writer(out)
    w.writerow(["name", "calls", "total_us", "average_us", "min_us", "max_us", "percent_of_kernel_time", "streams", "queues",
                "busy_us", "overlap_factor"])
    for name, v in sorted(by.items(), key=lambda kv: -sum(e - s for s, e, _, _ in kv[1])):
        d = [e - s for s, e, _, _ in v]
        busy = busy_ns([(s, e) for s, e, _, _ in v])
        w.writerow([name, len(v), "%.3f" % (sum(d) / 1e3), "%.3f" % (sum(d) / len(d) / 1e3), "%.3f" % (min(d) / 1e3),
                    "%.3f" % (max(d) / 1e3), "%.3f" % (100.0 * sum(d) / all_ns), len({x[2] for x in v}), len({x[3] for x in v}),
                    "%.3f" % (busy / 1e3), "%.4f" % (sum(d) / busy)])


if __name__ == "__main__":
    main(sys.argv[1])
