"""Per-launch timeline of the keypoint stage of the last bench step, from a rocprofv3 kernel trace and (optionally) the HIP API
trace of the SAME run: for every launch of the affine, patch and descriptor kernels its start, end and hardware queue, and - with the
API trace - the moment the host submitted it (matched by correlation id).  A launch that the host submitted long before it started
waited on the device; one that started as it was submitted waited for the host.
usage: group_timeline.py <kernel_trace.csv> [<hip_api_trace.csv>] [--slow-ms 0.2]"""
import csv, sys

args = [a for a in sys.argv[1:] if not a.startswith('--')]
slow_ms = float(sys.argv[sys.argv.index('--slow-ms') + 1]) if '--slow-ms' in sys.argv else 0.2
rows = list(csv.DictReader(open(args[0])))
ks = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].split('(')[0].replace('void ', ''), r.get('Queue_Id', ''),
       r.get('Correlation_Id', '')) for r in rows]
ks.sort()
# the last step: from its first pyramid launch (the blur that converts the source: the only k_blur_hess_march instantiation whose
# last template argument, SRC, is not 0) to its k_pack
starts = [k[0] for k in ks if k[2].startswith('k_gray') or (k[2].startswith('k_blur_hess_march') and not k[2].rstrip().endswith(', 0>'))]
t0 = max(starts)
ks = [k for k in ks if k[0] >= t0]
ends = [k[1] for k in ks if k[2].startswith('k_pack')]
t1 = min(ends) if ends else max(k[1] for k in ks)
ks = [k for k in ks if k[0] < t1]

submit = {}
api = []
if len(args) > 1:
    for r in csv.DictReader(open(args[1])):
        s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
        api.append((s, e, r['Function'], r.get('Correlation_Id', '')))
        if 'Launch' in r['Function']:
            submit[r.get('Correlation_Id', '')] = s

SHORT = (('k_patch_extract_small<0', 'small0'), ('k_patch_extract_small<1', 'small1'), ('k_patch_mid<128', 'mid128'), ('k_patch_mid<512', 'mid512'),
         ('k_patch_large_rows', 'lrows'), ('k_patch_large_finish', 'lfinish'), ('k_large_prefix', 'lprefix'), ('k_sift_grad', 'grad'), ('k_sift_hist', 'hist'),
         ('k_sift_meanvar', 'meanvar'), ('k_sift_quant', 'quant'), ('k_affine', 'affine'), ('k_prepare_patch', 'prep'))
def short(n):
    for key, f in SHORT:
        if n.startswith(key): return f
    return None

qids = sorted({k[3] for k in ks if short(k[2])})
print('step span %.2f ms; keypoint-stage launches by start time (ms from the step\'s first kernel); queues %s' % ((t1 - t0) / 1e6, ' '.join(qids)))
print('%9s %9s %8s  %-5s %-8s %10s %9s' % ('start', 'end', 'ms', 'queue', 'kernel', 'submitted', 'waited'))
count = {}
for s, e, n, q, cid in ks:
    f = short(n)
    if not f: continue
    count[f] = count.get(f, 0) + 1
    sub = submit.get(cid)
    print('%9.3f %9.3f %8.3f  %-5s %-8s %10s %9s' % ((s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6, q, '%s#%d' % (f, count[f] - 1),
                                                      '%.3f' % ((sub - t0) / 1e6) if sub else '-', '%.3f' % ((s - sub) / 1e6) if sub else '-'))
if api:
    # host calls inside the step that took long: where the submitting thread stood still
    print('\nHIP API calls of the step that lasted more than %.2f ms (start, ms, function):' % slow_ms)
    first_sub = min([v for v in submit.values() if v >= t0 - 50e6] or [t0])
    for s, e, fn, cid in sorted(api):
        if s >= first_sub - 5e6 and s < t1 and (e - s) / 1e6 > slow_ms:
            print('%9.3f %8.3f  %s' % ((s - t0) / 1e6, (e - s) / 1e6, fn))
    inwin = [(s, e, fn) for s, e, fn, cid in api if s >= first_sub and s < t1]
    tot = {}
    for s, e, fn in inwin:
        a = tot.setdefault(fn, [0, 0.0]); a[0] += 1; a[1] += (e - s) / 1e6
    print('\nHIP API calls from the step\'s first launch to its k_pack: count, total ms')
    for fn, (c, ms) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        print('%-28s %6d %9.3f' % (fn, c, ms))
