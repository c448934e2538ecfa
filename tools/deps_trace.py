#!/usr/bin/env python
"""Per-module schedule figures of the HRNet forward program from one rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python bench.py --traffic-child --batch 64
    python tools/deps_trace.py OUT [--batch 64] [--passes 3] > profiles/deps_trace_<which>.txt

The trace has no op tags, so the program is recorded again here (recording needs no GPU; set EGONET_AMD_DEPS as the
traced run had it) and its launches are laid over the trace in dispatch order: one kernel per op, and behind every pass
the one-block ticket check (egn_ticket_errors_kernel) that marks where a pass ends.  Kernel names must repeat from pass
to pass at every position, else the alignment is refused.

Per stage module (tags stageS.K.branches.* / .fuse_layers.* / .fuseI), median over the passes, in microseconds:
  wall     first branch kernel start -> last fuse kernel end
  cu_time  sum over its kernels of duration x min(blocks, CUs) / CUs: what the module would take on a full chip
  fill     cu_time / wall
  gap      end of the FIRST lane to finish its branch chain -> start of the first fuse-phase kernel
  barrier  end of the LAST lane to finish its branch chain -> start of the first fuse-phase kernel (negative: fuse-phase
           kernels already ran beside the slowest branch)
  tail     first lane's end -> last lane's end
"""
import argparse
import csv
import glob
import os
import re
import statistics
import sys

os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS = 256
TICKET_KERNEL = 'egn_ticket_errors_kernel'
TAG = re.compile(r'^(stage\d+\.\d+)\.(branches\.(\d+)|fuse_layers\.(\d+)\.(\d+)|fuse(\d+))')


def load_kernels(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('no *kernel_trace.csv under %s' % path)
    rows = []
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                blocks = 1
                for d in 'XYZ':
                    g, w = int(row.get('Grid_Size_' + d, 1) or 1), int(row.get('Workgroup_Size_' + d, 1) or 1)
                    blocks *= max(1, (g + w - 1) // max(w, 1))
                rows.append(dict(name=row['Kernel_Name'], start=int(row['Start_Timestamp']), end=int(row['End_Timestamp']),
                                 blocks=blocks, did=int(row.get('Dispatch_Id', 0) or 0)))
    rows.sort(key=lambda r: (r['did'], r['start']))
    return rows


def recorded_ops(batch, head):
    from egonet_amd import configs
    from egonet_amd.engine import HRNetEngine
    from egonet_amd.model.heatmapModel import hrnet
    net = hrnet.get_pose_net(configs.w48_config(head), is_train=False).eval()
    rec, _, _ = HRNetEngine(net)._record(batch, 3, 256, 256, 1 if head == 'heatmap' else None)
    return [(kind, op) for kind, op in rec.ops if kind not in ('fork', 'join')]


def split_passes(rows, nops, passes):
    marks = [i for i, r in enumerate(rows) if TICKET_KERNEL in r['name']]
    out = []
    if len(marks) >= passes:
        for m in marks[-passes:]:
            out.append(rows[m - nops:m])
    else:
        tail = rows[len(rows) - passes * nops:]
        out = [tail[k * nops:(k + 1) * nops] for k in range(passes)]
    for k in range(nops):
        names = {p[k]['name'] for p in out}
        if len(names) != 1 or any(len(p) != nops for p in out):
            raise SystemExit('the passes do not line up at op %d: %s' % (k, sorted(names)))
    return out


def module_figures(ops, rows):
    mods = {}
    for (kind, op), r in zip(ops, rows):
        m = TAG.match(op.get('tag', ''))
        if not m:
            continue
        d = mods.setdefault(m.group(1), dict(branch={}, fuse=[], all=[]))
        d['all'].append(r)
        if m.group(3) is not None:
            d['branch'].setdefault(int(m.group(3)), []).append(r)
        else:
            d['fuse'].append(r)
    out = {}
    for name, d in mods.items():
        if not d['fuse'] or not d['branch']:
            continue
        ends = [max(r['end'] for r in rs) for rs in d['branch'].values()]
        t0 = min(r['start'] for rs in d['branch'].values() for r in rs)
        f0 = min(r['start'] for r in d['fuse'])
        wall = max(r['end'] for r in d['all']) - t0
        cu = sum((r['end'] - r['start']) * min(r['blocks'], CUS) / float(CUS) for r in d['all'])
        out[name] = dict(wall=wall / 1e3, cu_time=cu / 1e3, fill=cu / wall, gap=(f0 - min(ends)) / 1e3,
                         barrier=(f0 - max(ends)) / 1e3, tail=(max(ends) - min(ends)) / 1e3, kernels=len(d['all']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--head', default='heatmap')
    a = ap.parse_args()
    ops = recorded_ops(a.batch, a.head)
    passes = split_passes(load_kernels(a.trace), len(ops), a.passes)
    figs = [module_figures(ops, p) for p in passes]
    spans = [(p[-1]['end'] - p[0]['start']) / 1e3 for p in passes]
    ends = [(max(r['end'] for r in p) - min(r['start'] for r in p)) / 1e3 for p in passes]
    print('# EGONET_AMD_DEPS=%s  batch %d  %d launches per pass, %d passes' %
          (os.environ.get('EGONET_AMD_DEPS', '(unset)'), a.batch, len(ops), a.passes))
    print('# forward, first kernel start -> last kernel end, per pass [us]: %s' % ' '.join('%.1f' % e for e in ends))
    print('# (first launch start -> last launch end: %s)' % ' '.join('%.1f' % s for s in spans))
    cols = ('wall', 'cu_time', 'fill', 'gap', 'barrier', 'tail')
    print('%-10s %4s ' % ('module', 'k') + ' '.join('%9s' % c for c in cols))
    tot = dict.fromkeys(cols, 0.0)
    for name in figs[0]:
        med = {c: statistics.median(f[name][c] for f in figs) for c in cols}
        for c in cols:
            tot[c] += med[c]
        print('%-10s %4d ' % (name, figs[0][name]['kernels']) +
              ' '.join(('%9.3f' if c == 'fill' else '%9.1f') % med[c] for c in cols))
    tot['fill'] = tot['cu_time'] / tot['wall'] if tot['wall'] else 0.0
    print('%-10s %4s ' % ('sum', '') + ' '.join(('%9.3f' if c == 'fill' else '%9.1f') % tot[c] for c in cols))
    for k, f in enumerate(figs):
        print('# pass %d: sum of gaps %.1f us, sum of barriers %.1f us, sum of walls %.1f us' %
              (k, sum(v['gap'] for v in f.values()), sum(v['barrier'] for v in f.values()),
               sum(v['wall'] for v in f.values())))


if __name__ == '__main__':
    main()
