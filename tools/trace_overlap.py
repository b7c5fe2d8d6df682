"""How many tracing-kernel launches run side by side, from a rocprofv3 --kernel-trace CSV (kt_kernel_trace.csv).

    python tools/trace_overlap.py <kernel_trace.csv> [--kernel path_pool_kernel] [--skip N]

Prints one JSON object: the launches counted (after skipping the first N: warm-up), their grid sizes and hardware queues, the
histogram of launches open at each launch's midpoint, the time-weighted histogram of launches open between the first start and
the last end, and the longest stretch with fewer than two open.
"""
import argparse
import csv
import json
from collections import Counter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--kernel", default="path_pool_kernel")
    ap.add_argument("--skip", type=int, default=0)
    a = ap.parse_args()
    rows = [r for r in csv.DictReader(open(a.csv)) if a.kernel in r["Kernel_Name"]]
    spans = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"],
                    int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)) for r in rows)[a.skip:]
    at_mid = Counter()
    for s, e, _, _ in spans:
        m = (s + e) // 2
        at_mid[sum(1 for b, c, _, _ in spans if b <= m < c)] += 1
    edges = sorted([(s, 1) for s, _, _, _ in spans] + [(e, -1) for _, e, _, _ in spans])
    open_ns, n_open, last, longest_thin, thin_since = Counter(), 0, edges[0][0], 0, None
    for t, d in edges:
        open_ns[n_open] += t - last
        if n_open < 2 and thin_since is None:
            thin_since = last
        last = t
        n_open += d
        if n_open >= 2 and thin_since is not None:
            longest_thin = max(longest_thin, t - thin_since)
            thin_since = None
    if thin_since is not None:
        longest_thin = max(longest_thin, last - thin_since)
    total = max(edges[-1][0] - edges[0][0], 1)
    dur = [e - s for s, e, _, _ in spans]
    gaps = [spans[i + 1][0] - spans[i][0] for i in range(len(spans) - 1)]
    print(json.dumps({
        "launches": len(spans), "workgroups": dict(Counter(g for _, _, _, g in spans)), "hardware_queues": dict(Counter(q for _, _, q, _ in spans)),
        "mean_span_ms": round(sum(dur) / len(dur) / 1e6, 3), "mean_start_to_start_ms": round(sum(gaps) / max(len(gaps), 1) / 1e6, 3),
        "open_at_launch_midpoint": {str(k): v for k, v in sorted(at_mid.items())},
        "time_share_by_launches_open": {str(k): round(v / total, 3) for k, v in sorted(open_ns.items()) if v},
        "longest_stretch_with_fewer_than_two_open_ms": round(longest_thin / 1e6, 3)}))


if __name__ == "__main__":
    main()
