#!/usr/bin/env python
"""Per-row A/B of the streaming kernels behind HETEROFL_STREAM_VEC: BN+ReLU
fwd/bwd, the split reduces (timed as the whole conv call: the main kernel is
the same either way, so on - off is the reduce's) and clip+SGD.  Every row is
timed with the switch off and on, alternating, in one process, with hip
events: as replays of two captured graphs of `iters` launches each (the
flagship runs captured graphs, and eager launches floor near 6 us each, above
most of these kernels), or with --eager as plain launches.  Run on a GPU box:
    python scripts/streambench.py [iters] [reps] [--eager]
"""
import os
import sys

import torch

sys.path.insert(0, '.')
from heterofl_amd.ops import require_native  # noqa: E402

VAR = 'HETEROFL_STREAM_VEC'
R, N = 5, 10
HIDDEN = [64, 128, 256, 512]
PLANES = [32, 16, 8, 4]
CONVS = [
    # (name, G, N, Cin, H, Cout, k, stride, pad): scripts/convbench.py SHAPES
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


def timeit(fn, iters):
    """eager launches between two events: floors near 6 us per launch"""
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


def capture(fn, iters):
    """`iters` calls as one captured graph (the switch is read at capture)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_replay(g, iters):
    s = torch.cuda.Event(True)
    e = torch.cuda.Event(True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000  # us


EAGER = '--eager' in sys.argv


def timeit_toggle(fn, iters, reps):
    off, on = [], []
    if EAGER:
        for _ in range(reps):
            os.environ[VAR] = '0'
            off.append(timeit(fn, iters))
            os.environ[VAR] = '1'
            on.append(timeit(fn, iters))
        del os.environ[VAR]
        return off, on
    os.environ[VAR] = '0'
    g_off = capture(fn, iters)
    os.environ[VAR] = '1'
    g_on = capture(fn, iters)
    del os.environ[VAR]
    for _ in range(reps):
        off.append(time_replay(g_off, iters))
        on.append(time_replay(g_on, iters))
    return off, on


def med(v):
    return sorted(v)[len(v) // 2]


def row(name, off, on, note=''):
    to, tn = med(off), med(on)
    so, sn = max(off) - min(off), max(on) - min(on)
    verdict = 'faster' if to - tn > so else 'slower' if tn - to > so \
        else 'same'
    print(f'{name:26} {to:8.1f} {tn:8.1f} {tn / to:6.2f} {so:10.1f} '
          f'{sn:9.1f}  {verdict:6} {note}')
    return to, tn


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    iters = int(args[0]) if len(args) > 0 else 50
    reps = int(args[1]) if len(args) > 1 else 5
    ext = require_native()
    from heterofl_amd.ops.fused import (FusedClipSGD, bn_relu_route,
                                        conv_plan)
    dt = torch.bfloat16
    print(f'toggle: {VAR}; {"eager" if EAGER else "graph replay"}; '
          f'{reps} repeats of {iters} launches, median us; '
          f'spread = max - min; faster / slower = beyond the off spread')
    print(f'{"row":26} {"off_us":>8} {"on_us":>8} {"on/off":>6} '
          f'{"off_spread":>10} {"on_spread":>9}')
    tot = {}

    def add(fam, to, tn):
        a = tot.setdefault(fam, [0.0, 0.0])
        a[0] += to
        a[1] += tn

    # BN+ReLU at the four flagship planes, full and 1/16 width
    for div in (1, 16):
        for H, width in zip(PLANES, HIDDEN):
            C = R * width // div
            x = torch.randn(N, C, H, H, device='cuda').to(dt)
            dy = torch.randn(N, C, H, H, device='cuda').to(dt)
            w = torch.rand(C, device='cuda') + 0.5
            b = torch.randn(C, device='cuda')
            _, mean, invstd = ext.bn_relu_fwd(x, w, b, 1e-5)
            route = bn_relu_route('fwd', N, C, H * H, 2)
            off, on = timeit_toggle(
                lambda: ext.bn_relu_fwd(x, w, b, 1e-5), iters, reps)
            add('bn fwd', *row(f'bn fwd {H}x{H} C={C}', off, on, route))
            off, on = timeit_toggle(
                lambda: ext.bn_relu_bwd(dy, x, w, b, mean, invstd), iters,
                reps)
            add('bn bwd', *row(f'bn bwd {H}x{H} C={C}', off, on, route))

    # split reduces: conv calls whose plan splits
    for name, G, n, Cin, H, Cout, k, s, p in CONVS:
        x = torch.randn(n, G * Cin, H, H, device='cuda').to(dt)
        w = torch.randn(G * Cout, Cin, k, k, device='cuda') * 0.1
        OH = (H + 2 * p - k) // s + 1
        dy = torch.randn(n, G * Cout, OH, OH, device='cuda').to(dt)
        none = torch.Tensor()
        calls = [
            ('fwd', 'fwd', lambda: ext.conv_fwd(x, w, none, none, G, s, p, 0)),
            ('bwdD', 'bwd_data',
             lambda: ext.conv_bwd_data(dy, w, G, s, p, H, H, 0)),
            ('bwdW', 'bwd_weight',
             lambda: ext.conv_bwd_weight(dy, x, G, s, p, k, 0)),
        ]
        for dname, direction, fn in calls:
            split = conv_plan(direction, G, n, Cin, H, H, Cout, k, s, p, 2,
                              0)[1]
            if split <= 1:
                continue
            off, on = timeit_toggle(fn, iters, reps)
            fam = 'splitp reduce' if dname == 'bwdW' else 'out reduce'
            add(fam, *row(f'conv {name} {dname}', off, on, f'split {split}'))

    # clip + SGD over the resnet18 parameter list, R = 5
    from heterofl_amd.fed.batched import BatchedResNet
    for div in (1, 16):
        hidden = [h // div for h in HIDDEN]
        bm = BatchedResNet(R, [3, 32, 32], hidden, [2, 2, 2, 2], 10,
                           1.0 / div, 'bn', True).to('cuda')
        params = [q.detach() for q in bm.parameters()]
        grads = [torch.randn_like(q) for q in params]
        bufs = [torch.zeros_like(q) for q in params]
        opt = FusedClipSGD(params, grads, bufs, R, 'cuda')
        numel = sum(q.numel() for q in params)
        off, on = timeit_toggle(lambda: opt.step(1.0, 0.0, 0.9, 5e-4), iters,
                                reps)
        add('clip+sgd', *row(f'clip+sgd width 1/{div}', off, on,
                             f'{numel} floats, {opt.n_chunks} chunks'))
    for fam, (to, tn) in tot.items():
        print(f'SUM {fam:22} {to:8.1f} {tn:8.1f} {tn / to:6.2f}')


if __name__ == '__main__':
    main()
