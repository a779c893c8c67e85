#!/usr/bin/env python3
"""Prints per-wavefront instruction counts and activity of k_chain_fused from gpurun_out/pmc_<tag> (tools/pmc_quick.sh)."""
# The chain's pixel stage is up to three kernels per call (k_chain_fused, k_chain_fused_rim, k_chain_fused_over; or
# k_chain_fused_whole alone): their counters are summed per call.  A call launches each member once at most, so the member
# with the most dispatches counts the calls.
import csv, glob, os, re, sys, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1]
acc = collections.defaultdict(float)
calls = collections.defaultdict(lambda: collections.defaultdict(int))     # key -> member kernel -> dispatches
for path in sorted(glob.glob(os.path.join(ROOT, 'gpurun_out', f'pmc_{tag}', 'p*', '**', '*counter_collection.csv'), recursive=True)):
    for r in csv.DictReader(open(path)):
        if 'k_chain_fused' in r['Kernel_Name']:
            ns = 'ns_' + os.path.basename(os.path.dirname(path))[:2]
            acc[r['Counter_Name']] += float(r['Counter_Value'])
            acc[ns] += int(r['End_Timestamp']) - int(r['Start_Timestamp'])
            member = re.search(r'k_chain_fused[a-z_]*', r['Kernel_Name']).group(0)
            calls[r['Counter_Name']][member] += 1
            calls[ns][member] += 1
m = {k: v / max(calls[k].values()) for k, v in acc.items()}
w = m.get('SQ_WAVES', 1)
for k in sorted(m):
    print(f'{k:24s} {m[k]:14.6g}  per wave {m[k] / w:10.2f}')
