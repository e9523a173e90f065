#!/usr/bin/env python3
"""Per-kernel register table of csrc files (all of csrc/*.hip when none is
named) from -Rpass-analysis=kernel-resource-usage, one sorted line per kernel:
file, kernel (mangled template id, anonymous namespace and argument list
stripped), VGPRs/AGPRs, scratch, LDS, occupancy.
`--compare A B`: every kernel of table A must be in B with no more
VGPRs/AGPRs/scratch and no less occupancy (exit status 1 otherwise).
usage: python tools/kres_all.py [igemm.hip halo_conv.hip ...] > table.txt
       python tools/kres_all.py --compare before.txt after.txt"""
import concurrent.futures as cf
import glob
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'uncertainty-model_amd', 'csrc')
KEYS = (('vgpr', 'VGPRs'), ('agpr', 'AGPRs'), ('scratch', 'ScratchSize [bytes/lane]'),
        ('lds', 'LDS Size [bytes/block]'), ('occ', 'Occupancy [waves/SIMD]'))


def short(name):
    name = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', name)
    i = name.rfind('EEv')  # end of the template arguments of a void kernel
    return name[:i + 2] if i >= 0 else name


def one(src):
    with tempfile.TemporaryDirectory() as td:
        cmd = ['/opt/rocm/bin/hipcc', '-O3', '-fPIC', '-std=c++17', '--offload-arch=gfx950',
               '-I', os.path.join(REPO, 'include'), '-I', CSRC, '-c', src,
               '-o', os.path.join(td, 'k.o'), '-Rpass-analysis=kernel-resource-usage']
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-3000:])
    cur, rows = None, []
    for line in r.stderr.splitlines():
        m = re.search(r'remark: (.*?) \[-Rpass', line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith('Function Name:'):
            cur = {'name': short(t.split(':', 1)[1].strip())}
            rows.append(cur)
        elif cur is not None and ':' in t:
            k, v = t.split(':', 1)
            cur[k.strip()] = v.strip()
    base = os.path.basename(src)
    return sorted(' '.join([base, d['name']] + [f'{a} {d.get(b, "?")}' for a, b in KEYS])
                  for d in rows)


def table(files):
    srcs = sorted(os.path.join(CSRC, f) for f in files) or \
        sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    with cf.ThreadPoolExecutor(max_workers=min(16, len(srcs))) as ex:
        for rows in ex.map(one, srcs):
            print('\n'.join(rows))


def parse(path):
    with open(path) as fh:
        rows = [line.split() for line in fh if line.strip()]
    return {(p[0], p[1]): {p[i]: int(p[i + 1]) for i in range(2, len(p) - 1, 2)} for p in rows}


def compare(a, b):
    A, B = parse(a), parse(b)
    bad = 0
    for k, va in A.items():
        vb = B.get(k)
        if vb is None or vb['vgpr'] > va['vgpr'] or vb['agpr'] > va['agpr'] or \
                vb['scratch'] > va['scratch'] or vb['occ'] < va['occ']:
            print('regressed:' if vb else 'missing:', *k, va, '->', vb)
            bad += 1
    print(f'{len(A)} kernels before, {len(B)} after, {bad} regressed or missing')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ['--compare'] else table(sys.argv[1:]))
