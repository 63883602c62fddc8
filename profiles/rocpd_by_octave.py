#!/usr/bin/env python3
"""rocprofv3 rocpd kernel trace of a serial SIFT pass (one work area in flight) -> pyramid kernel time per octave.
A batch's pyramid launches arrive in plan order: the base blur (the BGR variant) opens a batch, every extrema launch closes an octave.
usage: rocpd_by_octave.py <results.db> [batches per group, comma separated: 3,3,3 -> one table per group; default: all in one]
Per group: one row per (octave, kernel, radius, grid) from `first` (default 2) on with calls and us per launch, then the sum per batch."""
import re
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
groups = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 and sys.argv[2] else None
first = int(sys.argv[3]) if len(sys.argv) > 3 else 2
pat = re.compile(r"(blur16_stream|blur16_tile|downsample16|extrema_stream|extrema_kernel)(?:<(\d+), (true|false))?")
batches = []      # per batch: list of (octave, kernel, radius, grid, ns)
octave = None
for name, gx, gy, gz, t0, t1 in db.execute("select name, grid_x, grid_y, grid_z, start, end from kernels order by start"):
    m = pat.search(name)
    if not m:
        continue
    kern, rad, bgr = m.group(1), m.group(2), m.group(3)
    if bgr == "true":
        batches.append([]); octave = 0
    if octave is None:
        continue
    batches[-1].append((octave, kern, int(rad) if rad else 0, "%dx%dx%d" % (gx, gy, gz), t1 - t0))
    if kern.startswith("extrema"):
        octave += 1
if groups is None:
    groups = [len(batches)]
at = 0
for gi, nb in enumerate(groups):
    part = batches[at:at + nb]; at += nb
    if not part:
        break
    rows = {}
    for b in part:
        for o, kern, rad, grid, ns in b:
            if o >= first:
                c = rows.setdefault((o, kern, rad, grid), [0, 0]); c[0] += 1; c[1] += ns
    print("group %d: %d batches" % (gi, len(part)))
    print("  %-3s %-15s %3s %-14s %6s %10s" % ("oct", "kernel", "R", "grid", "calls", "us/launch"))
    per_oct = {}
    for (o, kern, rad, grid), (n, ns) in sorted(rows.items(), key=lambda kv: (kv[0][0], kv[0][1], -kv[0][2])):
        print("  %-3d %-15s %3d %-14s %6d %10.1f" % (o, kern, rad, grid, n, ns / 1e3 / n))
        per_oct[o] = per_oct.get(o, 0) + ns
    tot = sum(per_oct.values())
    print("  per batch, us: " + "  ".join("octave %d: %.1f" % (o, v / 1e3 / len(part)) for o, v in sorted(per_oct.items())) + "  | octaves >= %d: %.1f" % (first, tot / 1e3 / len(part)))
