#!/usr/bin/env python
"""Static instruction statistics of gfx950 kernels from a device-only
assembly listing:
    hipcc --offload-arch=gfx950 --cuda-device-only -S -O3 ... -o conv.s
    python scripts/isastats.py conv.s [substring-of-kernel-name ...]
Per kernel: instructions, VALU, MFMA, SALU, LDS, global, runtime integer
divides (v_rcp_iflag_f32), barriers, and for every loop that contains an
MFMA (label .. back-edge) the same counts of its body.
"""
import re
import sys


def classify(op):
    if op.startswith('v_mfma'):
        return 'mfma'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('s_'):
        return 'salu'
    return 'other'


def count(ops):
    c = {'n': len(ops), 'valu': 0, 'mfma': 0, 'salu': 0, 'lds': 0, 'vmem': 0,
         'other': 0, 'idiv': 0, 'barrier': 0}
    for op in ops:
        c[classify(op)] += 1
        if op.startswith('v_rcp_iflag'):
            c['idiv'] += 1
        if op == 's_barrier':
            c['barrier'] += 1
    return c


def fmt(c):
    return (f'instrs {c["n"]:5} VALU {c["valu"]:5} MFMA {c["mfma"]:3} '
            f'SALU {c["salu"]:4} LDS {c["lds"]:3} VMEM {c["vmem"]:3} '
            f'idiv {c["idiv"]:2} barriers {c["barrier"]}')


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    name, body = None, []
    kernels = {}
    for line in open(path):
        s = line.strip()
        m = re.match(r'^(_Z\w+):', s)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if s.startswith('.Lfunc_end'):
            kernels[name] = body
            name = None
            continue
        if not s or s.startswith((';', '.p2align', '.type', '.size')):
            continue
        m = re.match(r'^(\.LBB\w+):', s)
        if m:
            body.append(('label', m.group(1)))
        elif not s.startswith('.'):
            toks = s.split(';')[0].split()
            if toks:
                body.append(('op', toks[0], toks[1:] and toks[-1]))
    for kname, body in kernels.items():
        if pats and not any(p in kname for p in pats):
            continue
        ops = [b[1] for b in body if b[0] == 'op']
        print(kname)
        print('  total      ', fmt(count(ops)))
        labels = {b[1]: i for i, b in enumerate(body) if b[0] == 'label'}
        for i, b in enumerate(body):
            if b[0] == 'op' and b[1].startswith(('s_cbranch', 's_branch')) \
                    and b[2] in labels and labels[b[2]] < i:
                lops = [x[1] for x in body[labels[b[2]]:i + 1]
                        if x[0] == 'op']
                c = count(lops)
                if c['mfma']:
                    print(f'  loop {b[2]:10}', fmt(c))


if __name__ == '__main__':
    main()
