#!/usr/bin/env python
"""Per-shape A/B of the MFMA grouped conv: fwd, bwd-data, bwd-weight timed
separately with hip events.  Every native row is timed with one route
switch off and on, alternating, in one process; MIOpen (F.conv2d) is the
outside reference.  The switch is HETEROFL_CONV_RESIDENT (off = the staged
kernels) by default; `--toggle=tabled` alternates HETEROFL_CONV_TABLED
instead (off = the untabled gather kernels) with the resident switch left on.
Run on a GPU box:
    python scripts/convbench.py [iters] [reps] [--extra] [--toggle=tabled]
`--extra` appends large-window shapes that sit near the resident LDS cap
(sweep the cap itself with HETEROFL_CONV_RESIDENT_LDS=<bytes>).
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, '.')
from heterofl_amd.ops import require_native  # noqa: E402

SHAPES = [
    # (name, G, N, Cin, H, Cout, k, stride, pad)
    ('stem', 5, 10, 3, 32, 64, 3, 1, 1),
    ('L1', 5, 10, 64, 32, 64, 3, 1, 1),
    ('L2d', 5, 10, 64, 32, 128, 3, 2, 1),
    ('L2', 5, 10, 128, 16, 128, 3, 1, 1),
    ('L3d', 5, 10, 128, 16, 256, 3, 2, 1),
    ('L3', 5, 10, 256, 8, 256, 3, 1, 1),
    ('L4d', 5, 10, 256, 8, 512, 3, 2, 1),
    ('L4', 5, 10, 512, 4, 512, 3, 1, 1),
    ('sc2', 5, 10, 64, 32, 128, 1, 2, 0),
    ('sc3', 5, 10, 128, 16, 256, 1, 2, 0),
    ('sc4', 5, 10, 256, 8, 512, 1, 2, 0),
]
# unsplit slices whose window + tiles need about 53 KB / 64 KB of LDS
EXTRA = [
    ('X96', 5, 10, 96, 32, 96, 3, 1, 1),
    ('X128', 5, 10, 128, 32, 128, 3, 1, 1),
]


def timeit(fn, iters):
    s = torch.cuda.Event(True)
    e = torch.cuda.Event(True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000  # us


TOGGLES = {'resident': 'HETEROFL_CONV_RESIDENT',
           'tabled': 'HETEROFL_CONV_TABLED'}


def timeit_toggle(fn, iters, reps, var):
    """off/on alternating; returns the two lists of per-rep times (us)"""
    off, on = [], []
    for _ in range(reps):
        os.environ[var] = '0'
        off.append(timeit(fn, iters))
        os.environ[var] = '1'
        on.append(timeit(fn, iters))
    del os.environ[var]
    return off, on


def served(dname, H, OH, k, s):
    """rows whose geometry the staged, hence the resident-window, kernels
    take: 3x3, whole-row tiles inside one sample (64 pixels fwd/bwd-data,
    32 bwd-weight); bwd-data stride 1 only.  Slices over the LDS cap still
    fall back (X128 bwdD)."""
    if k != 3:
        return False
    if dname == 'fwd':
        return (OH * OH) % 64 == 0 and 64 % OH == 0
    if dname == 'bwdD':
        return s == 1 and (H * H) % 64 == 0 and 64 % H == 0
    return (OH * OH) % 32 == 0 and 32 % OH == 0


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    iters = int(args[0]) if len(args) > 0 else 50
    reps = int(args[1]) if len(args) > 1 else 5
    shapes = SHAPES + (EXTRA if '--extra' in sys.argv else [])
    toggle = 'resident'
    for a in sys.argv[1:]:
        if a.startswith('--toggle='):
            toggle = a.split('=', 1)[1]
    var = TOGGLES[toggle]
    from heterofl_amd.ops.fused import conv_plan
    ext = require_native()
    dt = torch.bfloat16
    print(f'toggle: {var}')
    print(f'{"shape":6} {"dir":5} {"off_us":>8} {"on_us":>8} {"on/off":>6} '
          f'{"off_spread":>10} {"on_spread":>9} {"res":>3} '
          f'{"miopen_us":>10} {"ratio":>6}  gflop')
    tot_n = tot_m = tot_off = 0.0
    srv_on = srv_off = 0.0
    gat_on = gat_off = gat_spread = 0.0
    for name, G, N, Cin, H, Cout, k, s, p in shapes:
        x = torch.randn(N, G * Cin, H, H, device='cuda', dtype=dt)
        w = torch.randn(G * Cout, Cin, k, k, device='cuda') * 0.1
        wb = w.to(dt)
        OH = (H + 2 * p - k) // s + 1
        dy = torch.randn(N, G * Cout, OH, OH, device='cuda', dtype=dt)
        gflop = 2.0 * N * G * Cout * Cin * k * k * OH * OH / 1e9
        rows = [
            ('fwd', 'fwd',
             lambda: ext.conv_fwd(x, w, torch.Tensor(), torch.Tensor(),
                                  G, s, p, 0),
             lambda: F.conv2d(x, wb, None, s, p, 1, G)),
            ('bwdD', 'bwd_data',
             lambda: ext.conv_bwd_data(dy, w, G, s, p, H, H, 0),
             lambda: torch.nn.grad.conv2d_input(
                 (N, G * Cin, H, H), wb, dy, (s, s), (p, p), (1, 1), G)),
            ('bwdW', 'bwd_weight',
             lambda: ext.conv_bwd_weight(dy, x, G, s, p, k, 0),
             lambda: torch.nn.grad.conv2d_weight(
                 x, (G * Cout, Cin, k, k), dy, (s, s), (p, p), (1, 1), G)),
        ]
        for dname, direction, fn_n, fn_m in rows:
            off, on = timeit_toggle(fn_n, iters, reps, var)
            gat = conv_plan(direction, G, N, Cin, H, H, Cout, k, s, p, 2,
                            0)[0].startswith('gather')
            tm = timeit(fn_m, iters)
            tn, to = med(on), med(off)
            # (L3d fwd has the geometry but 17 window rows: a gather row)
            srv = served(dname, H, OH, k, s) and not gat
            if (name, G, N, Cin, H, Cout, k, s, p) in SHAPES:
                tot_n += tn
                tot_off += to
                tot_m += tm
                if srv:
                    srv_on += tn
                    srv_off += to
                if gat:
                    gat_on += tn
                    gat_off += to
                    gat_spread += (max(off) - min(off)) + (max(on) - min(on))
            print(f'{name:6} {dname:5} {to:8.1f} {tn:8.1f} {tn / to:6.2f} '
                  f'{max(off) - min(off):10.1f} {max(on) - min(on):9.1f} '
                  f'{"y" if srv else "g" if gat else "-":>3} {tm:10.1f} {tn / tm:6.2f}  '
                  f'{gflop:.2f}')
    print(f'TOTAL native on {tot_n:.0f}us  off {tot_off:.0f}us  '
          f'miopen {tot_m:.0f}us  ratio {tot_n / tot_m:.2f}')
    print(f'RESIDENT rows: on {srv_on:.0f}us  off {srv_off:.0f}us  '
          f'on/off {srv_on / max(srv_off, 1e-9):.2f}')
    print(f'GATHER rows (res g): on {gat_on:.0f}us  off {gat_off:.0f}us  '
          f'on/off {gat_on / max(gat_off, 1e-9):.2f}  '
          f'summed spreads {gat_spread:.0f}us')


if __name__ == '__main__':
    main()
