#!/usr/bin/env python3
"""The ordered kernel-name list of every stream of a rocprofv3 kernel trace, as one line per stream: launches, SHA-256 of the names
(full names, template arguments included, one per line in launch order), first and last name.  Streams are listed by length and hash,
not by id, so two runs of the same program compare with diff.  With speculative trials in flight the order ACROSS streams is the
hardware's; the order inside a stream is the program's.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/c2_probe.py
    python tools/stream_kernel_lists.py <dir or kernel_trace.csv> [--names]     (--names: the lists themselves)"""
import csv
import glob
import hashlib
import os
import sys

src = sys.argv[1]
if os.path.isdir(src):
    found = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
    if len(found) != 1:
        sys.exit("expected one *kernel_trace.csv under %s, found %d" % (src, len(found)))
    src = found[0]
rows = list(csv.DictReader(open(src)))
key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
if key != "Stream_Id":
    print("# no Stream_Id column: split by Queue_Id (streams that share a hardware queue are merged)")
rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
streams = {}
for r in rows:
    streams.setdefault(r[key], []).append(r["Kernel_Name"])
out = []
for names in streams.values():
    out.append((len(names), hashlib.sha256("\n".join(names).encode()).hexdigest(), names))
out.sort(key=lambda t: (-t[0], t[1]))
print("# %d launches on %d streams" % (len(rows), len(out)))
for n, h, names in out:
    print("%6d %s  %s ... %s" % (n, h, names[0].split("(")[0][:60], names[-1].split("(")[0][:60]))
    if "--names" in sys.argv:
        for x in names:
            print("       " + x)
