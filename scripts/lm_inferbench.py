"""Masked-LM evaluation benchmark.  Run on a GPU box:

    python scripts/lm_inferbench.py [--out profiles/lm_inferbench.txt]

Part 1 — the vocabulary head at V = 33278, E in {256, 64, 16}, M in {640,
32768}: lm_head_ce (weight packing excluded, splits chosen by the host)
against the two-step baseline bf16 F.linear + lm_ce_fwd, alternated within
one process, warmed, timed with device events.  The 'fused/gemm' column is
what ops.fused.lm_head_route rests on.  A second table sweeps `splits` at
M = 640.

Part 2 — a whole synthetic WikiText2-shaped test set (HETEROFL_BENCH_TOKENS
tokens in the train stream, an eighth of that in the test stream, the real
vocabulary): FedRunner.test through the default eager loop, through
HETEROFL_NATIVE_LM_EVAL=1, and FedRunner.test_lm_levels for a1-b1-c1-d1-e1;
the two native ones once more with HETEROFL_LM_TOPK=5.

Part 3 (--topk) — the fill-mask head on the inputs of part 1, k in {1, 5,
8}: lm_head_topk against lm_head_ce and against the two-step baseline bf16
F.linear + torch.topk(logits.float(), k) + lm_ce_fwd, and a `splits` sweep at
M = 640.  --append adds the run to the --out file as a new section instead
of rewriting it.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from heterofl_amd.ops import require_native
from heterofl_amd.ops.fused import (lm_head_ce, lm_head_pack, lm_head_route,
                                    lm_head_topk)

V = 33278


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


def _head_inputs(M, E, dev):
    g = torch.Generator().manual_seed(M + E)
    x = torch.randn(M, E, generator=g).bfloat16().to(dev)
    w = (torch.randn(V, E, generator=g) * 0.1).to(dev)
    b = torch.randn(V, generator=g).to(dev)
    y = torch.randint(0, V, (M,), generator=g).to(dev)
    return x, w, b, y


def bench_head(emit, dev):
    ext = require_native()
    none = torch.Tensor()
    emit(f'-- vocabulary head, V={V}, bf16 x (us; TFLOP/s from '
         f'2*M*V*E) --')
    emit(f'{"M":>6} {"E":>4} {"fused":>9} {"gemm+ce":>9} {"fused_TF":>9} '
         f'{"gemm_TF":>8} {"fused/gemm":>10} {"max|dnll|":>10} {"routed":>6}')
    for E in (256, 64, 16):
        for M in (640, 32768):
            x, w, b, y = _head_inputs(M, E, dev)
            packed = lm_head_pack(w, b)
            w16, b16 = w.bfloat16(), b.bfloat16()

            def gemm():
                logits = F.linear(x, w16, b16)
                return logits, ext.lm_ce_fwd(logits, y, none, 1)[1]

            tf, tg = time_alternating([
                lambda: lm_head_ce(x, packed, b, y, None, V, E), gemm],
                iters=10 if M == 640 else 3)
            # the two heads on the same inputs (the gemm one rounds its
            # logits to bf16)
            logits, lse = gemm()
            nll_g = lse - logits.gather(1, y.view(-1, 1)).squeeze(1).float()
            nll_f = lm_head_ce(x, packed, b, y, None, V, E)[0]
            fl = 2.0 * M * V * E
            emit(f'{M:6d} {E:4d} {tf:9.1f} {tg:9.1f} {fl / tf / 1e6:9.1f} '
                 f'{fl / tg / 1e6:8.1f} {tf / tg:10.2f} '
                 f'{(nll_f - nll_g).abs().max().item():10.2e} '
                 f'{"yes" if lm_head_route(M, E, V) else "no":>6}')
            del logits
    emit('-- outside the routed envelope (M, E, V): fused vs gemm+ce (us) --')
    for M, E, Vs in ((64, 256, V), (250, 64, V), (640, 256, 10000),
                     (32768, 16, 10000), (640, 64, 1000)):
        g = torch.Generator().manual_seed(M)
        x = torch.randn(M, E, generator=g).bfloat16().to(dev)
        w = (torch.randn(Vs, E, generator=g) * 0.1).to(dev)
        b = torch.randn(Vs, generator=g).to(dev)
        y = torch.randint(0, Vs, (M,), generator=g).to(dev)
        packed = lm_head_pack(w, b)
        w16, b16 = w.bfloat16(), b.bfloat16()
        tf, tg = time_alternating([
            lambda: lm_head_ce(x, packed, b, y, None, Vs, E),
            lambda: ext.lm_ce_fwd(F.linear(x, w16, b16), y, none, 1)])
        emit(f'{M:6d} {E:4d} {Vs:6d} {tf:9.1f} {tg:9.1f} {tf / tg:10.2f} '
             f'{"yes" if lm_head_route(M, E, Vs) else "no":>6}')
    emit('-- lm_head_ce, M=640: time (us) by splits (0 = host choice) --')
    sweep = (0, 1, 13, 26, 52, 104, 208)
    emit(f'{"E":>4} ' + ' '.join(f'{s:>8d}' for s in sweep))
    for E in (256, 64, 16):
        x, w, b, y = _head_inputs(640, E, dev)
        packed = lm_head_pack(w, b)
        ts = time_alternating([
            (lambda s=s: lm_head_ce(x, packed, b, y, None, V, E, splits=s))
            for s in sweep])
        emit(f'{E:4d} ' + ' '.join(f'{t:8.1f}' for t in ts))


def bench_topk(emit, dev):
    ext = require_native()
    none = torch.Tensor()
    emit(f'-- fill-mask head, V={V}, bf16 x (us): lm_head_topk vs lm_head_ce '
         f'vs bf16 F.linear + torch.topk(fp32) + lm_ce_fwd --')
    emit(f'{"M":>6} {"E":>4} {"k":>2} {"topk":>9} {"ce":>9} {"gemm+topk":>10} '
         f'{"topk/ce":>8} {"topk/gemm":>10} {"idx agree":>10}')
    for E in (256, 64, 16):
        for M in (640, 32768):
            x, w, b, y = _head_inputs(M, E, dev)
            packed = lm_head_pack(w, b)
            w16, b16 = w.bfloat16(), b.bfloat16()
            for k in (1, 5, 8):
                def gemm():
                    logits = F.linear(x, w16, b16)
                    top = torch.topk(logits.float(), k)
                    return top, ext.lm_ce_fwd(logits, y, none, 1)[1]

                tt, tc, tg = time_alternating([
                    lambda: lm_head_topk(x, packed, b, y, None, V, E, k),
                    lambda: lm_head_ce(x, packed, b, y, None, V, E), gemm],
                    iters=10 if M == 640 else 3)
                # the share of rows on which the two routes name the same
                # columns (the gemm one ranks bf16-rounded logits)
                idx = lm_head_topk(x, packed, b, y, None, V, E, k)[1]
                same = (idx == gemm()[0].indices).all(1).float().mean().item()
                emit(f'{M:6d} {E:4d} {k:2d} {tt:9.1f} {tc:9.1f} {tg:10.1f} '
                     f'{tt / tc:8.2f} {tt / tg:10.2f} {same:10.3f}')
    emit('-- lm_head_topk, M=640, k=5: time (us) by splits (0 = host '
         'choice) --')
    sweep = (0, 1, 13, 26, 52, 104, 208)
    emit(f'{"E":>4} ' + ' '.join(f'{s:>8d}' for s in sweep))
    for E in (256, 64, 16):
        x, w, b, y = _head_inputs(640, E, dev)
        packed = lm_head_pack(w, b)
        ts = time_alternating([
            (lambda s=s: lm_head_topk(x, packed, b, y, None, V, E, 5,
                                      splits=s)) for s in sweep])
        emit(f'{E:4d} ' + ' '.join(f'{t:8.1f}' for t in ts))


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


def bench_runner(emit, dev):
    from heterofl_amd.config import default_config
    from heterofl_amd.control import process_control, CONTROL_FIELDS
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.logger import Logger
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    cfg = default_config()
    control = '1_100_0.1_iid_fix_a1-b1-c1-d1-e1_bn_1_1'
    cfg['control'] = dict(zip(CONTROL_FIELDS, control.split('_')))
    cfg['control_name'] = control
    cfg['data_name'] = 'WikiText2'
    cfg['model_name'] = 'transformer'
    cfg['device'] = dev
    cfg['engine'] = 'sequential'
    cfg['metric_name'] = {'train': {'Local': ['Local-Loss']},
                          'test': {'Global': ['Global-Loss',
                                              'Global-Perplexity']}}
    process_control(cfg)
    torch.manual_seed(0)
    toks = int(os.environ.get('HETEROFL_BENCH_TOKENS', '2000000'))
    ds = fetch_dataset('WikiText2', synthetic=True, synthetic_size=toks)
    cfg['batch_size'] = {'train': 100, 'test': 10}
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, cfg['num_users'], 'iid')
    model = make_model(cfg).to(dev)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg),
                       logger=Logger(None))
    tokens, windows = runner._stage_lm_eval()
    emit(f'-- whole test set: {tokens.size(0)} rows x {tokens.size(1)} '
         f'tokens, {len(windows)} windows, V={cfg["num_tokens"]} (ms per '
         f'call, host clock around a device sync) --')

    def test():
        runner.logger.reset()
        runner.test(runner.global_model, 1)

    os.environ.pop('HETEROFL_NATIVE_LM_EVAL', None)
    t_eager = _wall(test, 2)
    eager = dict(runner.logger.mean)
    os.environ['HETEROFL_NATIVE_LM_EVAL'] = '1'
    t_native = _wall(test, 3)
    native = dict(runner.logger.mean)
    os.environ.pop('HETEROFL_NATIVE_LM_EVAL', None)
    emit(f'{"test(), eager fp32 per-window loop":44} {t_eager:9.1f}')
    emit(f'{"test(), HETEROFL_NATIVE_LM_EVAL=1":44} {t_native:9.1f}')
    emit(f'{"  ratio native/eager":44} {t_native / t_eager:9.3f}')
    for k in ('test/Global-Loss', 'test/Global-Perplexity'):
        emit(f'  {k}: eager {eager[k]:.6f} native {native[k]:.6f} '
             f'(different masks, mask_rate {cfg["mask_rate"]})')
    t_levels = _wall(lambda: runner.test_lm_levels(1), 2)
    emit(f'{"test_lm_levels a1-b1-c1-d1-e1 (5 levels)":44} {t_levels:9.1f}')
    # the same two native evaluations with token accuracy from the same pass
    os.environ['HETEROFL_LM_TOPK'] = '5'
    os.environ['HETEROFL_NATIVE_LM_EVAL'] = '1'
    t_native5 = _wall(test, 3)
    native5 = dict(runner.logger.mean)
    os.environ.pop('HETEROFL_NATIVE_LM_EVAL', None)
    t_levels5 = _wall(lambda: runner.test_lm_levels(1), 2)
    os.environ.pop('HETEROFL_LM_TOPK', None)
    emit(f'{"test(), native, HETEROFL_LM_TOPK=5":44} {t_native5:9.1f}')
    emit(f'{"  ratio knob on/off":44} {t_native5 / t_native:9.3f}')
    emit(f'{"test_lm_levels, HETEROFL_LM_TOPK=5":44} {t_levels5:9.1f}')
    emit(f'{"  ratio knob on/off":44} {t_levels5 / t_levels:9.3f}')
    for k in sorted(native5):
        if 'Accuracy' in k:
            emit(f'  {k}: {native5[k]:.4f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-head', action='store_true')
    ap.add_argument('--skip-runner', action='store_true')
    ap.add_argument('--topk', action='store_true',
                    help='run part 3 (the fill-mask head)')
    ap.add_argument('--append', action='store_true',
                    help='add to the --out file instead of rewriting it')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lm_inferbench needs a GPU')
    dev = 'cuda:0'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f'device: {torch.cuda.get_device_name(0)}')
    if not args.skip_head:
        bench_head(emit, dev)
    if args.topk:
        bench_topk(emit, dev)
    if not args.skip_runner:
        bench_runner(emit, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
