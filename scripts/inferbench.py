"""Large-batch inference benchmark.  Run on a GPU box:

    python scripts/inferbench.py [--out profiles/inferbench.txt]

Part 1 — the ten statsbench.py conv shapes at N=500 and N=2048 in bf16:
conv_fwd_large (weight packing excluded), the training-family conv_fwd and
MIOpen (F.conv2d), alternated within one process, warmed, timed with device
events.  FLOP/s are computed from the shapes (2*N*OH*OW*Cout*Cin*k*k).
The 'large/old' column is what ops.fused.large_conv_route rests on; the
'large/miopen' column is the project's <= 1.0x goal for these shapes.

Part 2 — whole-test-set inference: 10k synthetic CIFAR-shaped samples,
resnet18 at rate a, NativeInference against the eager model.

Part 3 — FedRunner.test_levels for a1-e1 levels (--levels, off by default).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from heterofl_amd.ops import require_native
from heterofl_amd.ops.fused import (conv_fwd_large, conv_pack_weight,
                                    large_conv_route)

SHAPES = [  # name, Cin, H, Cout, k, stride, pad  (scripts/statsbench.py)
    ('stem', 3, 32, 64, 3, 1, 1),
    ('L1', 64, 32, 64, 3, 1, 1),
    ('L2d', 64, 32, 128, 3, 2, 1),
    ('L2', 128, 16, 128, 3, 1, 1),
    ('L3d', 128, 16, 256, 3, 2, 1),
    ('L3', 256, 8, 256, 3, 1, 1),
    ('L4d', 256, 8, 512, 3, 2, 1),
    ('L4', 512, 4, 512, 3, 1, 1),
    ('sc2', 64, 32, 128, 1, 2, 0),
    ('sc4', 256, 8, 512, 1, 2, 0),
]


def conv_flops(N, Cin, H, Cout, k, s, p):
    OH = (H + 2 * p - k) // s + 1
    return 2.0 * N * OH * OH * Cout * Cin * k * k


def time_alternating(fns, rounds=5, iters=10):
    """Median-of-rounds device-event time (us) per callable; the callables
    take turns inside every round so drift hits all of them alike."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[i].append(s.elapsed_time(e) / iters * 1000.0)
    return [sorted(t)[len(t) // 2] for t in times]


def bench_convs(emit, dev):
    ext = require_native()
    none = torch.Tensor()
    for N in (500, 2048):
        emit(f'-- conv shapes, bf16, N={N} (us; TFLOP/s from shapes) --')
        emit(f'{"shape":5} {"GFLOP":>7} {"large":>8} {"old":>8} '
             f'{"miopen":>8} {"large_TF":>9} {"old_TF":>7} {"mio_TF":>7} '
             f'{"large/old":>9} {"large/miopen":>12} {"routed":>6}')
        tot = [0.0, 0.0, 0.0]
        for name, Cin, H, Cout, k, s, p in SHAPES:
            x = torch.randn(N, Cin, H, H, device=dev).bfloat16()
            w = torch.randn(Cout, Cin, k, k, device=dev) * 0.1
            w16 = w.bfloat16()
            packed = conv_pack_weight(w)
            tl, to, tm = time_alternating([
                lambda: conv_fwd_large(x, packed, None, None, s, p, Cin,
                                       Cout, k),
                lambda: ext.conv_fwd(x, w, none, none, 1, s, p, 0),
                lambda: F.conv2d(x, w16, None, s, p)])
            fl = conv_flops(N, Cin, H, Cout, k, s, p)
            for i, t in enumerate((tl, to, tm)):
                tot[i] += t
            routed = large_conv_route(N, Cin, H, H, Cout, k, s, p)
            emit(f'{name:5} {fl / 1e9:7.2f} {tl:8.1f} {to:8.1f} {tm:8.1f} '
                 f'{fl / tl / 1e6:9.1f} {fl / to / 1e6:7.1f} '
                 f'{fl / tm / 1e6:7.1f} {tl / to:9.2f} {tl / tm:12.2f} '
                 f'{"yes" if routed else "no":>6}')
        emit(f'TOTAL {"":7} {tot[0]:8.1f} {tot[1]:8.1f} {tot[2]:8.1f} '
             f'{"":9} {"":7} {"":7} {tot[0] / tot[1]:9.2f} '
             f'{tot[0] / tot[2]:12.2f}')


# router sweep: width-level channel counts (rates b..e of L1 / L4) at N=500,
# and small-P cases of full-width layers.  name, N, Cin, H, Cout, k, s, p
ROUTER_SHAPES = [
    ('L1@b', 500, 32, 32, 32, 3, 1, 1), ('L1@c', 500, 16, 32, 16, 3, 1, 1),
    ('L1@d', 500, 8, 32, 8, 3, 1, 1), ('L1@e', 500, 4, 32, 4, 3, 1, 1),
    ('L4@b', 500, 256, 4, 256, 3, 1, 1), ('L4@c', 500, 128, 4, 128, 3, 1, 1),
    ('L4@d', 500, 64, 4, 64, 3, 1, 1), ('L4@e', 500, 32, 4, 32, 3, 1, 1),
    ('sc2@e', 500, 4, 32, 8, 1, 2, 0), ('sc4@e', 500, 16, 8, 32, 1, 2, 0),
    ('L1', 1, 64, 32, 64, 3, 1, 1), ('L1', 4, 64, 32, 64, 3, 1, 1),
    ('L1', 16, 64, 32, 64, 3, 1, 1), ('L1', 64, 64, 32, 64, 3, 1, 1),
    ('L2', 4, 128, 16, 128, 3, 1, 1), ('L2', 16, 128, 16, 128, 3, 1, 1),
    ('L2', 64, 128, 16, 128, 3, 1, 1),
    ('L3', 16, 256, 8, 256, 3, 1, 1), ('L3', 64, 256, 8, 256, 3, 1, 1),
    ('L4', 16, 512, 4, 512, 3, 1, 1), ('L4', 64, 512, 4, 512, 3, 1, 1),
    ('L4', 128, 512, 4, 512, 3, 1, 1), ('L4', 256, 512, 4, 512, 3, 1, 1),
    ('sc4', 64, 256, 8, 512, 1, 2, 0),
]


def bench_router(emit, dev):
    ext = require_native()
    none = torch.Tensor()
    emit('-- router sweep, bf16: conv_fwd_large vs conv_fwd (us) --')
    emit(f'{"shape":6} {"N":>5} {"Cin":>4} {"Cout":>5} {"H":>3} {"P":>7} '
         f'{"large":>8} {"old":>8} {"large/old":>9} {"routed":>6}')
    for name, N, Cin, H, Cout, k, s, p in ROUTER_SHAPES:
        x = torch.randn(N, Cin, H, H, device=dev).bfloat16()
        w = torch.randn(Cout, Cin, k, k, device=dev) * 0.1
        packed = conv_pack_weight(w)
        tl, to = time_alternating([
            lambda: conv_fwd_large(x, packed, None, None, s, p, Cin, Cout, k),
            lambda: ext.conv_fwd(x, w, none, none, 1, s, p, 0)])
        OH = (H + 2 * p - k) // s + 1
        routed = large_conv_route(N, Cin, H, H, Cout, k, s, p)
        emit(f'{name:6} {N:5d} {Cin:4d} {Cout:5d} {H:3d} {N * OH * OH:7d} '
             f'{tl:8.1f} {to:8.1f} {tl / to:9.2f} '
             f'{"yes" if routed else "no":>6}')


def _cfg(control, dev):
    from heterofl_amd.config import default_config
    from heterofl_amd.control import process_control, CONTROL_FIELDS
    cfg = default_config()
    cfg['control'] = dict(zip(CONTROL_FIELDS, control.split('_')))
    cfg['control_name'] = control
    cfg['data_name'] = 'CIFAR10'
    cfg['model_name'] = 'resnet18'
    cfg['device'] = dev
    cfg['engine'] = 'batched'
    cfg['compute_dtype'] = 'bfloat16'
    cfg['metric_name'] = {
        'train': {'Local': ['Local-Loss', 'Local-Accuracy']},
        'test': {'Local': ['Local-Loss', 'Local-Accuracy'],
                 'Global': ['Global-Loss', 'Global-Accuracy']}}
    process_control(cfg)
    cfg['classes_size'] = 10
    return cfg


def _wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1000.0)
    return sorted(ts)[len(ts) // 2]


def bench_whole_pass(emit, dev, n=10000, batch=2048):
    from heterofl_amd.fed.infer import NativeInference
    from heterofl_amd.models import make_model
    cfg = _cfg('1_100_0.1_iid_fix_a1_bn_1_1', dev)
    torch.manual_seed(0)
    model = make_model(cfg, model_rate=1, track=True).to(dev)
    model.train(False)
    x = torch.randn(n, 3, 32, 32, device=dev)
    label = torch.zeros(n, dtype=torch.long, device=dev)

    def eager():
        with torch.no_grad():
            return torch.cat([
                model({'img': x[b:b + batch],
                       'label': label[b:b + batch]})['score']
                for b in range(0, n, batch)])

    def native(large):
        eng = NativeInference(model, torch.bfloat16, large=large)
        return lambda: torch.cat([eng(x[b:b + batch])
                                  for b in range(0, n, batch)])

    emit(f'-- whole-set inference, resnet18 rate a, {n} samples, '
         f'batch {batch} (ms, host clock around a device sync) --')
    runs = [('eager fp32 (MIOpen)', eager),
            ('NativeInference bf16, routed', native(True)),
            ('NativeInference bf16, conv_fwd only', native(False))]
    for name, fn in runs:
        emit(f'{name:38} {_wall(fn):9.1f}')


def bench_levels(emit, dev, spu=100):
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    cfg = _cfg('1_100_0.1_iid_fix_a1-b1-c1-d1-e1_bn_1_1', dev)
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=spu * 100)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 100, 'iid', 10)
    model = make_model(cfg).to(dev)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    emit(f'-- test_levels a1-b1-c1-d1-e1, resnet18, {spu * 100} train / '
         f'{len(ds["test"])} test samples (ms per call, all five levels) --')
    emit(f'{"test_levels":38} {_wall(lambda: runner.test_levels(1), 2):9.1f}')
    emit(f'{"stats() + test() (global level only)":38} '
         f'{_wall(lambda: runner.test(runner.stats(), 1), 2):9.1f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--levels', action='store_true')
    ap.add_argument('--skip-convs', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inferbench needs a GPU')
    dev = 'cuda:0'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f'device: {torch.cuda.get_device_name(0)}')
    if not args.skip_convs:
        bench_convs(emit, dev)
        bench_router(emit, dev)
    bench_whole_pass(emit, dev)
    if args.levels:
        bench_levels(emit, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
