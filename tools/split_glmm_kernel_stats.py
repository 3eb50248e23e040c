"""Kernel statistics of one `rocprofv3 --kernel-trace --output-format csv -- python tools/time_glmm_poisson.py` run, from its
kernel trace: the table rocprofv3's --stats writes, with a median, and with the dispatches of the mixed-model kernels over the rows
(`glmm_slopes_*` / `glmm_poisson_*` rows, infl_rows, infl_gsum) split by dispatch order into `[K = 1]` (the first half of a
kernel's dispatches) and `[K = 4]` -- BY POSITION: the trace does not record K; the timing script runs K = 1 before K = 4 with
the same number of calls, and an odd number of dispatches is an error.

    python tools/split_glmm_kernel_stats.py <..._kernel_trace.csv> > profiles/<name>.csv
"""
import csv
import re
import statistics
import sys

SPLIT = re.compile(r'glmm_(slopes|poisson)_(rows|infl_rows|infl_gsum)_kernel')
runs = {}
with open(sys.argv[1], newline='') as f:
    for r in sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp'])):
        runs.setdefault(r['Kernel_Name'], []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
rows = {}
for name, d in runs.items():
    if SPLIT.search(name):                                              # by position only: the trace does not record K
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
