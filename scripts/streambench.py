#!/usr/bin/env python
"""Per-row A/B of the streaming kernels behind HETEROFL_STREAM_VEC: BN+ReLU
fwd/bwd, the split reduces (timed as the whole conv call: the main kernel is
the same either way, so on - off is the reduce's) and clip+SGD.  Every row is
timed with the switch off and on, alternating, in one process, with hip
events: as replays of two captured graphs of `iters` launches each (the
flagship runs captured graphs, and eager launches floor near 6 us each, above
most of these kernels), or with --eager as plain launches.  --step times the
vision step's glue behind HETEROFL_STEP_FUSED instead: the old launch chains
(classifier tail at both widths, batch fetch, BN backward + residual add)
against the entries that replace them.  Run on a GPU box:
    python scripts/streambench.py [iters] [reps] [--eager] [--step]
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


def time_pair(fn_off, fn_on, iters, reps):
    """two different call chains instead of one call under a switch; fn_on
    None (a build without the new entry): the chain alone, twice"""
    if fn_on is None:
        fn_on = fn_off
    if EAGER:
        off, on = [], []
        for _ in range(reps):
            off.append(timeit(fn_off, iters))
            on.append(timeit(fn_on, iters))
        return off, on
    g_off = capture(fn_off, iters)
    g_on = capture(fn_on, iters)
    off, on = [], []
    for _ in range(reps):
        off.append(time_replay(g_off, iters))
        on.append(time_replay(g_on, iters))
    return off, on


def step_rows(ext, iters, reps):
    """The vision step's glue behind HETEROFL_STEP_FUSED, old chain (off)
    against the new entry (on): the classifier tail at both widths, the batch
    fetch, BN backward + residual-gradient add at the four flagship planes.
    On a build without the new entries both columns are the old chain."""
    from heterofl_amd.ops import fused
    dt = torch.bfloat16
    J = 10
    has = hasattr(ext, 'head_ce_fwd')
    print(f'toggle: old chain / new entry ({"present" if has else "absent"}); '
          f'{"eager" if EAGER else "graph replay"}; {reps} repeats of '
          f'{iters} chains, median us')
    print(f'{"row":26} {"off_us":>8} {"on_us":>8} {"on/off":>6} '
          f'{"off_spread":>10} {"on_spread":>9}')
    for C in (512, 32):
        feat = torch.randn(N, R * C, 4, 4, device='cuda').to(dt) \
            .requires_grad_()
        w = (torch.randn(R, J, C, device='cuda') / C ** 0.5).requires_grad_()
        b = torch.randn(R, J, device='cuda').requires_grad_()
        y = torch.randint(0, J, (N, R), device='cuda')
        mask = (torch.rand(R, J, device='cuda') > 0.4).float()
        metrics = torch.zeros(R, 3, device='cuda')
        ones = torch.ones(R, device='cuda')

        def chain():
            scores = fused.fused_head(feat, w, b, R)
            losses = fused.fused_masked_ce(scores.float(), y, mask, metrics)
            return torch.autograd.grad(losses.sum(), [feat, w, b])

        def entry():
            losses, _ = fused.fused_head_ce(feat, w, b, y, mask, R,
                                            metrics=metrics)
            return torch.autograd.grad(losses, [feat, w, b],
                                       grad_outputs=ones)

        off, on = time_pair(chain, entry if has else None, iters, reps)
        row(f'head+CE tail C={C}', off, on, '7 launches -> 2')

    B = 10
    cap = (iters + 4) * B
    x_all = torch.randn(cap, R * 3, 32, 32, device='cuda').to(dt)
    y_all = torch.randint(0, J, (cap, R), device='cuda')
    counter = torch.zeros(1, dtype=torch.long, device='cuda')
    ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
    arange = torch.arange(B, device='cuda')
    calls = [0]

    def rewind():
        # first call of every `iters`: the counter back to 0, so a replay
        # never walks off the buffer (one more launch per `iters` chains)
        if calls[0] % iters == 0:
            counter.zero_()
        calls[0] += 1

    def fetch5():
        rewind()
        idx = counter * B + arange
        xb = x_all.index_select(0, idx)
        yb = y_all.index_select(0, idx)
        counter.add_(1)
        return xb, yb

    def fetch1():
        rewind()
        return fused.batch_gather(x_all, y_all, counter, B, ticket)

    # like capture(), with the call count set so that the recorded graph
    # starts with the rewind
    off, on = [], []
    for fn, dst in ((fetch5, off), (fetch1 if has else fetch5, on)):
        if EAGER:
            calls[0] = 0
            dst.extend(timeit(fn, iters) for _ in range(reps))
            continue
        for _ in range(3):
            calls[0] = 1
            counter.zero_()
            fn()
        torch.cuda.synchronize()
        calls[0] = 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        dst.extend(time_replay(g, iters) for _ in range(reps))
    # interleaving is lost here (one graph after the other); spreads say
    # whether that matters
    row('batch fetch B=10', off, on, '5 launches -> 1')

    for div in (1, 16):
        for H, width in zip(PLANES, HIDDEN):
            C = R * width // div
            x = torch.randn(N, C, H, H, device='cuda').to(dt)
            dy = torch.randn(N, C, H, H, device='cuda').to(dt)
            ad = torch.randn(N, C, H, H, device='cuda').to(dt)
            g = torch.rand(C, device='cuda') + 0.5
            bb = torch.randn(C, device='cuda')
            _, mean, invstd = ext.bn_relu_fwd(x, g, bb, 1e-5)
            route = fused.bn_relu_route('bwd', N, C, H * H, 2)
            off, on = time_pair(
                lambda: ext.bn_relu_bwd(dy, x, g, bb, mean, invstd)[0] + ad,
                (lambda: ext.bn_relu_bwd_add(dy, x, g, bb, mean, invstd, ad))
                if has else None, iters, reps)
            row(f'bn bwd+add {H}x{H} C={C}', off, on, route)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    iters = int(args[0]) if len(args) > 0 else 50
    reps = int(args[1]) if len(args) > 1 else 5
    ext = require_native()
    if '--step' in sys.argv:
        step_rows(ext, iters, reps)
        return
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
