#!/usr/bin/env python3
"""Per-step summary of a rocprofv3 kernel trace (SQLite output) of a training loop: wall time per step between the last
steps' Adam launches, the GPU's busy time (union of kernel intervals) and idle time in that window, kernels per step,
the heaviest kernels and the contrastive loss kernels.

    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/bench_contrastive.py --bs 128 ...
    python tools/trace_step_summary.py <dir>/run_results.db [...]
"""
import sqlite3, sys, collections
def summary(path, steps=100):
    db = sqlite3.connect(path)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    adam = [r for r in rows if 'adam' in r[0].lower()]
    adam = adam[-(steps + 1):]
    t0, t1 = adam[0][2], adam[-1][2]
    win = [r for r in rows if r[1] >= t0 and r[2] <= t1]
    # busy time: union of the kernels' intervals
    busy, cur_s, cur_e = 0, None, None
    for _, s, e in sorted((r for r in win), key=lambda r: r[1]):
        if cur_e is None or s > cur_e:
            if cur_e is not None: busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += cur_e - cur_s
    per = collections.defaultdict(lambda: [0, 0])
    for n, s, e in win:
        k = n.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0].split('<')[0]
        per[k][0] += 1; per[k][1] += e - s
    n = len(adam) - 1
    wall = (t1 - t0) / n / 1e3
    print("%s: %d steps, wall %.1f us/step, GPU busy %.1f us/step, idle %.1f us/step, %.1f kernels/step"
          % (path.split('/')[-2], n, wall, busy / n / 1e3, wall - busy / n / 1e3, len(win) / n))
    for k, (c, d) in sorted(per.items(), key=lambda kv: -kv[1][1])[:12]:
        print("   %-50s %5.2f/step %8.1f us/step" % (k[:50], c / n, d / n / 1e3))
    for k, (c, d) in per.items():
        if 'infonce' in k or 'ebm' in k:
            print("   loss kernel %-38s %5.2f/step %8.1f us/step (%.2f %% of wall)" % (k, c / n, d / n / 1e3, 100 * d / n / 1e3 / wall))
for p in sys.argv[1:]:
    summary(p)
