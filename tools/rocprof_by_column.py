#!/usr/bin/env python3
"""Per-block-column durations of a kernel that is launched once per block column, from a rocprofv3 results .db:
rocprof_by_column.py <results.db> <name-filter> <launches per factorisation>.  Launches are taken in start order on each stream and
numbered modulo the period (potrf_kernel: nblk, trsm4_kernel and panel_kernel: nblk - 1 when every factorisation of the run has the
same nblk, as config C's), so row k is block column k."""
import sqlite3
import sys

con = sqlite3.connect(sys.argv[1])
cur = con.cursor()
flt, period = sys.argv[2], int(sys.argv[3])
cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
qcol = [c for c in cols if c.lower() in ("queue_id", "stream_id", "queue")]
qcol = qcol[0] if qcol else "0"
rows = cur.execute(f"select name, {qcol}, start, end from kernels order by start").fetchall()
seen, acc = {}, {}
for name, q, s, e in rows:
    if flt not in name.split("(")[0]:
        continue
    k = seen.get(q, 0)
    seen[q] = k + 1
    acc.setdefault(k % period, []).append((e - s) / 1e3)
for k in sorted(acc):
    v = acc[k]
    print(f"{flt:16s} column {k:3d} calls {len(v):5d} avg {sum(v)/len(v):9.2f} us  min {min(v):9.2f} us")
