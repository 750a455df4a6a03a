"""PCG launches of a resident BA window that do no work, from a rocprofv3 kernel trace of tools/c2_probe.py and the probe's own
output (the LM trace of the last optimize(5): one dict per trial with 'inner', 'early', 'accepted').

Every k_spmv_f / k_pcg_update launch of the last step falls into one of three classes:
  useful             the solve it belongs to was still running when it started
  behind a finished  queued behind a solve that had converged (flags[0] set): every workgroup starts, reads the flag and returns
  aborted follower   of a speculative trial the host discarded (it never shows in the LM trace)
A device trial is the launches of one stream from a k_trial_setup to the next one (tools/trial_timeline.py).  Device trials are
matched to the LM trace in start order: a device trial stands for the next trace entry if it holds at least the launches that
entry needed (inner + 1 for a solve that ran to convergence -- the launch pair that finds it converged does the work of an
iteration -- and inner for one rejected at a peek); otherwise it is a discarded follower.  Launches of a matched trial beyond
what it needed are 'behind a finished solve'.  As a check on the matching the table also counts, per class, the launches no longer
than 1.5 x the shortest launch of that kernel in the step (a no-op is a launch floor).

On the critical path: for a matched trial, the no-op launches between its last useful launch and the k_apply that follows them on
the same stream hold that evaluation up by their summed duration (the host waits for the evaluation).  For discarded followers:
the time by which their last kernel ends after the accepted trial's last k_finalize, which is what the next lineariser waits for.
Fill dispatches (__amd_rocclr_fillBufferAligned) of the step are counted with their stream.

    python tools/wasted_launches.py <kernel_trace.csv> <probe_stdout.txt>
"""
import ast
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
nm = [r['Kernel_Name'].split('(')[0].replace('void nrs::', '').replace('nrs::', '').split('<')[0] for r in rows]
st = [int(r['Start_Timestamp']) for r in rows]
en = [int(r['End_Timestamp']) for r in rows]
sid = [r.get('Stream_Id', '0') for r in rows]
host = []
for line in open(sys.argv[2]):
    line = line.strip()
    if line.startswith('{') and "'inner'" in line:
        host.append(ast.literal_eval(line))
lin = [i for i, n in enumerate(nm) if n == 'k_lin_plain']
i0 = lin[-5]
t0 = st[i0]
idx = list(range(i0, len(rows)))
main = sid[i0]
span = max(en[i] for i in idx) - t0
PCG = ('k_spmv_f', 'k_pcg_update')
floor = {k: min(en[i] - st[i] for i in idx if nm[i] == k) for k in PCG}

trials = []
for s in [i for i in idx if nm[i] == 'k_trial_setup']:
    own = [s]
    for i in range(s + 1, len(rows)):
        if sid[i] != sid[s]:
            continue
        if nm[i] in ('k_trial_setup', 'k_lin_plain'):
            break
        own.append(i)
    trials.append(own)

cls = {}                                 # launch index -> class
crit = {'behind': 0, 'aborted': 0}
hi = 0
match = []
last_fin_main = None
for own in trials:
    ops = [i for i in own if nm[i] == 'k_spmv_f']
    ups = [i for i in own if nm[i] == 'k_pcg_update']
    need = None
    if hi < len(host):
        h = host[hi]
        need = h['inner'] + (0 if h['early'] else 1)
    if need is not None and len(ops) >= need:
        hi += 1
        match.append((own, h, need))
        for lst in (ops, ups):
            for k, i in enumerate(lst):
                cls[i] = 'useful' if k < need else 'behind'
        # no-ops in front of an evaluation of this trial: runs of 'behind' launches directly followed (same stream) by k_apply
        run = 0
        for i in own:
            if cls.get(i) == 'behind':
                run += en[i] - st[i]
            elif nm[i] == 'k_apply':
                crit['behind'] += run
                run = 0
            elif nm[i] in PCG:
                run = 0
    else:
        match.append((own, None, 0))
        for i in ops + ups:
            cls[i] = 'aborted'

# discarded followers against the lineariser that waits for them
for li in [i for i in lin if i > i0] + [None]:
    before = [t for t in match if li is None or st[t[0][0]] < st[li]]
    acc = [t for t in before if t[1] is not None and t[1]['accepted']]
    if not acc:
        continue
    fin = [i for i in acc[-1][0] if nm[i] == 'k_finalize']
    if not fin:
        continue
    t_acc = en[fin[-1]]
    tail = [en[i] for t in before if t[1] is None for i in t[0] if en[i] > t_acc and (li is None or en[i] <= st[li] + 1)]
    if tail:
        crit['aborted'] += max(tail) - t_acc
    match = [t for t in match if t not in before]

print("step span %.1f us, %d device trials, %d in the LM trace (%d matched)" % (span / 1e3, len(trials), len(host), hi))
print("launch floors in this step: k_spmv_f %.2f us, k_pcg_update %.2f us" % (floor['k_spmv_f'] / 1e3, floor['k_pcg_update'] / 1e3))
print("%-22s %-14s %7s %11s %9s %12s" % ("class", "kernel", "count", "sum_us", "mean_us", "at_floor"))
tot = {}
for c in ('useful', 'behind', 'aborted'):
    for k in PCG:
        sel = [i for i in cls if cls[i] == c and nm[i] == k]
        d = sum(en[i] - st[i] for i in sel)
        nf = sum(1 for i in sel if en[i] - st[i] <= 1.5 * floor[k])
        tot[c] = tot.get(c, 0) + d
        label = {'useful': 'useful', 'behind': 'behind a finished solve', 'aborted': 'aborted follower'}[c]
        print("%-22s %-14s %7d %11.1f %9.2f %12d" % (label[:22], k, len(sel), d / 1e3, d / 1e3 / max(1, len(sel)), nf))
fills = [i for i in idx if nm[i] == '__amd_rocclr_fillBufferAligned']
fm = [i for i in fills if sid[i] == main]
print("fill dispatches: %d (%.1f us), of them on the context's stream %d (%.1f us)"
      % (len(fills), sum(en[i] - st[i] for i in fills) / 1e3, len(fm), sum(en[i] - st[i] for i in fm) / 1e3))
ab = [i for t in trials for i in t if all(cls.get(j) == 'aborted' or nm[j] not in PCG for j in t) and any(cls.get(j) == 'aborted' for j in t) and nm[i] not in PCG]
print("other kernels of discarded followers (set-up, apply, evaluation): %d, %.1f us" % (len(ab), sum(en[i] - st[i] for i in ab) / 1e3))
n_pcg = sum(1 for i in idx if nm[i] in PCG)
print("launches per step: k_spmv_f + k_pcg_update %d, fills %d, all kernels %d" % (n_pcg, len(fills), len(idx)))
print("on the critical path: no-ops in front of an evaluation the host waits for %.1f us (%.2f %% of the step); "
      "discarded followers holding the next lineariser %.1f us (%.2f %%)"
      % (crit['behind'] / 1e3, 100.0 * crit['behind'] / span, crit['aborted'] / 1e3, 100.0 * crit['aborted'] / span))
