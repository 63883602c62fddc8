"""medians of scratch/pair_host_time.py lines by library:   python scratch/pair_host_time_summary.py FILE.jsonl"""
import json, statistics, sys
runs = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
libs = sorted({r["lib"] for r in runs})
for key, field in (("pairs_59", "wall_ms_median"), ("pairs_59", "call_ms_median"), ("pairs_1", "wall_ms_median"), ("pairs_1", "call_ms_median"), ("bf_match", "ms_median"), ("select_grid", "ms_median")):
    for lib in libs:
        v = [r[key][field] for r in runs if r["lib"] == lib]
        print("%-12s %-15s %-40s median %.4f  min %.4f  max %.4f  n %d" % (key, field, lib[-40:], statistics.median(v), min(v), max(v), len(v)))
print("records equal:", len({r["pairs_59"]["records_sha1"] for r in runs}) == 1 and len({r["pairs_1"]["records_sha1"] for r in runs}) == 1)
