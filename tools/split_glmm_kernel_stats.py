"""Kernel statistics of one `rocprofv3 --kernel-trace --output-format csv -- python tools/time_glmm_poisson.py` run, from its
kernel trace: the table rocprofv3's --stats writes, with a median, and with the dispatches of the mixed-model kernels over the rows
(`glmm_slopes_*` / `glmm_poisson_*` rows, infl_rows, infl_gsum) split by dispatch order into `[K = 1]` (the first half of a
kernel's dispatches) and `[K = 4]` -- BY POSITION: the trace does not record K; the timing script runs K = 1 before K = 4 with
the same number of calls, and an odd number of dispatches is an error.

    python tools/split_glmm_kernel_stats.py <..._kernel_trace.csv> > profiles/<name>.csv

With `--reps R` (the REPS of the timing tool the trace is of; 4 for time_glmm_slopes.py and time_glmm_influence.py) the trace may
be of ANY `tools/time_glmm_*.py`: only the kernels that walk the rows through a likelihood policy are kept (rows, infl_rows,
infl_gsum, predict_rows, disp_rows), and the dispatches of each are cut BY POSITION into the n equal runs of consecutive dispatches
that the tool made at one family, K and censored share -- n the largest divisor of the count not above count / R -- named
`[1/n]` .. `[n/n]`.

    python tools/split_glmm_kernel_stats.py --reps 5 <..._kernel_trace.csv> > profiles/<name>.csv
"""
import csv
import re
import statistics
import sys

SPLIT = re.compile(r'glmm_(slopes|poisson)_(rows|infl_rows|infl_gsum)_kernel')
WALKS = re.compile(r'glmm_\w*(rows|infl_rows|infl_gsum|predict_rows|disp_rows)_kernel')
reps = 0
if sys.argv[1] == '--reps':
    reps = int(sys.argv[2])
    del sys.argv[1:3]
runs = {}
with open(sys.argv[1], newline='') as f:
    for r in sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp'])):
        runs.setdefault(r['Kernel_Name'], []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
rows = {}
for name, d in runs.items():
    if reps:
        if not WALKS.search(name) or 'schur_rows' in name:
            continue
        n = max(len(d) // reps, 1)
        while len(d) % n:
            n -= 1
        for i in range(n):
            rows['%s [%d/%d]' % (name, i + 1, n)] = d[i * (len(d) // n):(i + 1) * (len(d) // n)]
    elif SPLIT.search(name):                                              # by position only: the trace does not record K
        if len(d) % 2:
            sys.exit('%s: %d dispatches cannot be halved into K = 1 and K = 4' % (name, len(d)))
        rows[name + ' [K = 1]'], rows[name + ' [K = 4]'] = d[:len(d) // 2], d[len(d) // 2:]
    else:
        rows[name] = d
total = sum(map(sum, rows.values()))
out = csv.writer(sys.stdout, quoting=csv.QUOTE_NONNUMERIC)
out.writerow(['Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage', 'MinNs', 'MaxNs', 'StdDev', 'MedianNs'])
for name, d in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
    out.writerow([name, len(d), sum(d), round(sum(d) / len(d), 6), round(100.0 * sum(d) / total, 4), min(d), max(d),
                  round(statistics.pstdev(d), 6), statistics.median(d)])
