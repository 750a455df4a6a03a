"""The last optimize(5) of a resident BA window split by LM trial, from a rocprofv3 kernel trace (tools/c2_probe.py under
rocprofv3 --kernel-trace).  A PCG trial starts at its k_trial_setup and ends with the last k_finalize before the next trial or
linearisation; per trial: start and end (us from the step's first lineariser launch), operator launches before its first
evaluation (the first peek batch) and in all, evaluations, kernel-busy time, and the gap to the next trial.  Trials that overlap
(speculative trials on streams of their own) show a negative gap.

    python tools/trial_timeline.py <kernel_trace.csv> [accepted flags, e.g. FFFFFTTTTT]
"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
nm = [r['Kernel_Name'].split('(')[0].replace('void nrs::', '').replace('nrs::', '').split('<')[0] for r in rows]
st = [int(r['Start_Timestamp']) for r in rows]
en = [int(r['End_Timestamp']) for r in rows]
lin = [i for i, n in enumerate(nm) if n == 'k_lin_plain']
i0 = lin[-5]
t0 = st[i0]
idx = list(range(i0, len(rows)))
span = max(en[i] for i in idx) - t0
setups = [i for i in idx if nm[i] == 'k_trial_setup']
# a trial owns the launches from its set-up up to the next set-up or lineariser launch, in launch order of its own stream: with
# speculative trials several run at once, so launches are assigned to the trial whose stream (rocprofv3 Stream_Id) they ran on
sid = [r.get('Stream_Id', '0') for r in rows]
trials = []
for k, s in enumerate(setups):
    own = [s]
    for i in range(s + 1, len(rows)):
        if nm[i] in ('k_trial_setup', 'k_lin_plain') and sid[i] == sid[s]:
            break
        if sid[i] == sid[s]:
            own.append(i)
    fin = [i for i in own if nm[i] == 'k_finalize']
    if fin:
        own = [i for i in own if st[i] <= st[fin[-1]]]
    trials.append(own)
acc = sys.argv[2] if len(sys.argv) > 2 else ''
print("step span %.1f us (first lineariser launch to last kernel end), %d trials" % (span / 1e3, len(trials)))
print("%-5s %-4s %9s %9s %9s %8s %6s %6s %5s %9s" % ("trial", "acc", "start_us", "end_us", "dur_us", "busy_us", "spmv1", "spmv", "evals", "gap_us"))
ends = []
for k, own in enumerate(trials):
    a, b = st[own[0]], max(en[i] for i in own)
    ends.append(b)
    fin = [i for i in own if nm[i] == 'k_finalize']
    sp1 = sum(1 for i in own if nm[i] == 'k_spmv_f' and (not fin or st[i] < st[fin[0]]))
    sp = sum(1 for i in own if nm[i] == 'k_spmv_f')
    busy = sum(en[i] - st[i] for i in own)
    nxt = st[trials[k + 1][0]] - b if k + 1 < len(trials) else float('nan')
    print("%-5d %-4s %9.1f %9.1f %9.1f %8.1f %6d %6d %5d %9.1f" % (k, acc[k] if k < len(acc) else '?', (a - t0) / 1e3, (b - t0) / 1e3,
                                                                  (b - a) / 1e3, busy / 1e3, sp1, sp, len(fin), nxt / 1e3))
if len(acc) >= len(trials) and 'T' in acc:
    first_acc = acc.index('T')
    if first_acc > 0:
        run = st[trials[first_acc][0]] - st[trials[0][0]]
        print("rejected run of LM iteration 0 (trials 0..%d): set-up of trial 0 to set-up of trial %d = %.1f us = %.1f %% of the step"
              % (first_acc - 1, first_acc, run / 1e3, 100.0 * run / span))
