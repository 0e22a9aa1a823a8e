"""Resident-window grouped-conv kernels (ops/csrc/conv_mfma.hip) against
the staged kernels they replace (bit-exact, HETEROFL_CONV_RESIDENT=0) and
against F.conv2d / autograd on fp32 copies, and the table of which kernel
and split each shape takes.  Run with: pytest tests -m gpu"""
import contextlib
import functools
import os

import pytest
import torch

from tests.conftest import make_cfg

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

# (G, N, Cin, H, Cout, k, stride, pad)
CASES = {
    # OW=16; fwd splitk=2 with the second slice starting mid-channel (k=96:
    # cin 10, tap 6); ragged last chunk (K=180); ragged M; bwdW splitp=4
    'A': (2, 2, 20, 16, 36, 3, 1, 1),
    # stride 2, 9 window rows
    'B': (2, 2, 20, 32, 36, 3, 2, 1),
    # 1x1 stride-2 shortcut, no split (1x1 stays on the gather kernel with
    # the toggle either way: the route must not disturb it)
    'C': (2, 2, 64, 32, 36, 1, 2, 0),
    # rate-1/16: K=36, OW=32
    'D': (3, 2, 4, 32, 4, 3, 1, 1),
    # OW=8, one tile = one sample; splitk=4 with slices at cin 0, 10r6, 21r3,
    # 32r0; bwdW p-chunks of 96 crossing a sample boundary mid-sample
    'E': (2, 3, 40, 8, 24, 3, 1, 1),
    # K=2304, splitk=32 with 8 empty slices; 72 k-steps
    'F': (1, 1, 256, 8, 64, 3, 1, 1),
    # stem: K=27, a single ragged chunk
    'G': (2, 2, 3, 32, 64, 3, 1, 1),
    # window of the unsplit slice exceeds any LDS cap (<= 64 KB): fallback
    'H': (1, 16, 256, 32, 256, 3, 1, 1),
}
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
PARAMS = [(c, d) for c in CASES for d in DTYPES
          if not (c == 'H' and d == 'fp32')]
PARAMS_S1 = [(c, d) for c, d in PARAMS if CASES[c][6] == 1]
PARAMS_K3 = [(c, d) for c, d in PARAMS if CASES[c][5] == 3]


@contextlib.contextmanager
def resident(on):
    prev = os.environ.get('HETEROFL_CONV_RESIDENT')
    os.environ['HETEROFL_CONV_RESIDENT'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_CONV_RESIDENT']
        else:
            os.environ['HETEROFL_CONV_RESIDENT'] = prev


@functools.lru_cache(maxsize=None)
def results(case, dname):
    """Every native result of one case, toggle on ('new') and off ('old'),
    plus the fp32 torch references; computed once per (case, dtype)."""
    import torch.nn.functional as F
    from heterofl_amd.ops import require_native
    ext = require_native()
    G, N, Cin, H, Cout, k, s, p = CASES[case]
    dt = DTYPES[dname]
    torch.manual_seed(0)
    OH = (H + 2 * p - k) // s + 1
    x = torch.randn(N, G * Cin, H, H, device='cuda').to(dt)
    w = torch.randn(G * Cout, Cin, k, k, device='cuda') * 0.1
    b = torch.randn(G * Cout, device='cuda')
    res = torch.randn(N, G * Cout, OH, OH, device='cuda').to(dt)
    dy = torch.randn(N, G * Cout, OH, OH, device='cuda').to(dt)
    none = torch.Tensor()
    out = {}
    for tag, on in (('new', True), ('old', False)):
        with resident(on):
            r = {'fwd': ext.conv_fwd(x, w, none, none, G, s, p, 0),
                 'fwd_bias': ext.conv_fwd(x, w, b, none, G, s, p, 0),
                 'fwd_res': ext.conv_fwd(x, w, b, res, G, s, p, 0)}
            if s == 1:
                r['bwdD'] = ext.conv_bwd_data(dy, w, G, s, p, H, H, 0)
            if k == 3:
                r['bwdW'] = ext.conv_bwd_weight(dy, x, G, s, p, k, 0)
        out[tag] = r
    xf = x.float().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    ref = F.conv2d(xf, wf, None, stride=s, padding=p, groups=G)
    ref.backward(dy.float())
    out['ref'] = {
        'fwd': ref.detach(),
        'fwd_bias': ref.detach() + b.view(1, -1, 1, 1),
        'fwd_res': ref.detach() + b.view(1, -1, 1, 1) + res.float(),
        'bwdD': xf.grad, 'bwdW': wf.grad}
    torch.cuda.synchronize()
    return out


def check(case, dname, key, fp32_bound):
    r = results(case, dname)
    new, old, ref = r['new'][key], r['old'][key], r['ref'][key]
    err = (new.float() - ref).abs().max().item()
    rel = err / ref.abs().max().item()
    print(f'{case} {dname} {key}: equal={torch.equal(new, old)} '
          f'abs={err:.3e} rel={rel:.3e}')
    assert torch.equal(new, old), (case, dname, key)
    if dname == 'fp32':
        assert err < fp32_bound, (case, key, err, fp32_bound)
    else:
        assert rel < 0.05, (case, key, rel)


@needs_gpu
@pytest.mark.parametrize('case,dname', PARAMS)
@pytest.mark.parametrize('key', ['fwd', 'fwd_bias', 'fwd_res'])
def test_resident_fwd(case, dname, key):
    G, N, Cin, H, Cout, k, s, p = CASES[case]
    check(case, dname, key, 5e-4 * Cin * k)


@needs_gpu
@pytest.mark.parametrize('case,dname', PARAMS_S1)
def test_resident_bwd_data(case, dname):
    G, N, Cin, H, Cout, k, s, p = CASES[case]
    check(case, dname, 'bwdD', 5e-4 * Cout * k)


@needs_gpu
@pytest.mark.parametrize('case,dname', PARAMS_K3)
def test_resident_bwd_weight(case, dname):
    G, N, Cin, H, Cout, k, s, p = CASES[case]
    check(case, dname, 'bwdW', 5e-3 * N * H)


# ---------------------------------------------------------------- route table
# Which kernel and split every shape takes (ops.fused.conv_plan: the
# launchers' own plan functions, nothing launched).  Shapes: CASES above plus
# the seven of test_gpu.py::test_mfma_conv_matches_torch.  Rows are
# (fwd, bwd_data, bwd_weight) as (route, split) with the resident toggle on
# and fp8 off, recorded from the host layer as it stood before the routing
# was factored into plan functions (commit e9e3335); the A/C/E/F/H anchors
# are the ones the CASES comments claim.
ROUTE_SHAPES = dict(CASES, **{
    'stem': (5, 10, 3, 32, 64, 3, 1, 1),
    'layer1': (5, 10, 64, 32, 64, 3, 1, 1),
    'down': (5, 10, 64, 32, 128, 3, 2, 1),
    'short': (5, 10, 64, 32, 128, 1, 2, 0),
    'layer4': (5, 10, 512, 4, 512, 3, 1, 1),
    'r16': (3, 10, 4, 32, 4, 3, 1, 1),
    'odd': (2, 7, 20, 16, 36, 3, 2, 1),
})
R, S, GA, G2 = 'resident', 'staged', 'gather', 'gather_s2'
ROUTES = {
    'A': {'bf16': ((R, 2), (R, 4), (R, 4)), 'fp32': ((R, 2), (R, 4), (R, 4))},
    'B': {'bf16': ((R, 2), (G2, 1), (R, 4)),
          'fp32': ((R, 2), (G2, 1), (R, 4))},
    'C': {'bf16': ((GA, 1), (G2, 1), (GA, 4)),
          'fp32': ((GA, 1), (G2, 1), (GA, 4))},
    'D': {'bf16': ((R, 1), (R, 1), (R, 16)),
          'fp32': ((R, 1), (R, 1), (R, 16))},
    'E': {'bf16': ((R, 4), (R, 2), (R, 2)), 'fp32': ((R, 4), (R, 2), (R, 2))},
    'F': {'bf16': ((R, 32), (R, 8), (R, 1)),
          'fp32': ((R, 32), (R, 8), (R, 1))},
    'G': {'bf16': ((R, 1), (R, 8), (R, 16)),
          'fp32': ((R, 1), (R, 8), (R, 16))},
    'H': {'bf16': ((S, 1), (S, 1), (R, 8)), 'fp32': ((S, 1), (S, 1), (S, 8))},
    'stem': {'bf16': ((R, 1), (R, 1), (R, 128)),
             'fp32': ((R, 1), (S, 1), (R, 128))},
    'layer1': {'bf16': ((R, 1), (R, 1), (R, 32)),
               'fp32': ((S, 1), (S, 1), (R, 32))},
    'down': {'bf16': ((R, 4), (G2, 1), (R, 16)),
             'fp32': ((S, 4), (G2, 1), (S, 16))},
    'short': {'bf16': ((GA, 1), (G2, 1), (GA, 32)),
              'fp32': ((GA, 1), (G2, 1), (GA, 32))},
    'layer4': {'bf16': ((GA, 16), (GA, 16), (GA, 1)),
               'fp32': ((GA, 16), (GA, 16), (GA, 1))},
    'r16': {'bf16': ((R, 1), (R, 1), (R, 128)),
            'fp32': ((R, 1), (R, 1), (R, 128))},
    'odd': {'bf16': ((GA, 2), (G2, 1), (R, 4)),
            'fp32': ((GA, 2), (G2, 1), (R, 4))},
}
# bf16 with fp8=1: every direction runs the fp8 instantiation of its gather
# kernel, the toggle either way; bwd-data's kernel per shape (same source)
FP8_BWD_DATA = {
    'A': GA, 'B': G2, 'C': G2, 'D': GA, 'E': GA, 'F': GA, 'G': GA, 'H': GA,
    'stem': GA, 'layer1': GA, 'down': G2, 'short': G2, 'layer4': GA,
    'r16': GA, 'odd': G2}
# fp32 with fp8=1 (no fp8 tiles for fp32): fwd drops to the plain gather
# kernel, bwd-data to the staged kernel, bwd-weight ignores the flag
FP32_FP8 = {
    'A': ((GA, 2), (S, 4), (R, 4)),
    'layer1': ((GA, 1), (S, 1), (R, 32)),
}
DIRECTIONS = ('fwd', 'bwd_data', 'bwd_weight')


def plans(shape, dname, fp8):
    from heterofl_amd.ops.fused import conv_plan
    G, N, Cin, H, Cout, k, s, p = ROUTE_SHAPES[shape]
    esz = {'bf16': 2, 'fp32': 4}[dname]
    out = []
    for d in DIRECTIONS:
        route, split, lds = conv_plan(d, G, N, Cin, H, H, Cout, k, s, p, esz,
                                      fp8)
        assert (lds > 0) == (route == R), (shape, dname, d, route, lds)
        out.append((route, split))
    return tuple(out)


def staged_for_resident(row):
    return tuple((S if r == R else r, sp) for r, sp in row)


@needs_gpu
@pytest.mark.parametrize('shape', list(ROUTE_SHAPES))
def test_conv_route_table(shape):
    assert set(ROUTES) == set(ROUTE_SHAPES) == set(FP8_BWD_DATA)
    for dname in DTYPES:
        want = ROUTES[shape][dname]
        with resident(True):
            assert plans(shape, dname, 0) == want, (shape, dname)
        # toggle off: every resident becomes staged with the same split
        with resident(False):
            assert plans(shape, dname, 0) == staged_for_resident(want), \
                (shape, dname)
    splits = [sp for _, sp in ROUTES[shape]['bf16']]
    want8 = tuple(zip((GA + '_fp8', FP8_BWD_DATA[shape] + '_fp8',
                       GA + '_fp8'), splits))
    for on in (True, False):
        with resident(on):
            assert plans(shape, 'bf16', 1) == want8, (shape, on)
    if shape in FP32_FP8:
        want = FP32_FP8[shape]
        with resident(True):
            assert plans(shape, 'fp32', 1) == want, shape
        with resident(False):
            assert plans(shape, 'fp32', 1) == staged_for_resident(want), shape


@needs_gpu
def test_resident_graph_step_bit_identical(base_cfg):
    """A captured ResNet18 group step (rate 0.0625, R=2, batch 4, 2 replays)
    trains to bit-identical parameters with the toggle on and off."""
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed.batched import BatchedClientTrainer
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset
    cfg = make_cfg(base_cfg, '1_2_1_iid_fix_a1_bn_1_1',
                   data_name='CIFAR10', model_name='resnet18')
    cfg['device'] = 'cuda:0'
    cfg['engine'] = 'batched'
    cfg['compute_dtype'] = 'bfloat16'
    cfg['hip_graphs'] = True
    cfg['num_epochs'] = {'global': 1, 'local': 1}
    cfg['batch_size'] = dict(cfg['batch_size'], train=4)
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=16)
    process_dataset(ds, cfg)
    torch.manual_seed(1)
    data_split, label_split = split_dataset(ds, 2, 'iid', 10)
    # 8 samples per client = 2 replays of the batch-4 step
    assert all(len(data_split['train'][u]) == 8 for u in range(2))
    rate = 0.0625
    torch.manual_seed(2)
    gp = make_model(cfg, model_rate=rate).to('cuda:0').state_dict()
    user_idx = [0, 1]
    rates = [rate, rate]
    results_ = {}
    for on in (True, False):
        with resident(on):
            tr = BatchedClientTrainer(dict(cfg))
            tr.set_data(ds, data_split)
            torch.manual_seed(42)
            torch.cuda.manual_seed_all(42)
            out = tr.train_clients(
                [0, 1], user_idx,
                [{k: v.clone() for k, v in gp.items()} for _ in user_idx],
                rates, None, label_split, 0.1)
            torch.cuda.synchronize()
            results_[on] = dict(out)
    for m in range(2):
        for k in results_[True][m]:
            a, b = results_[True][m][k], results_[False][m][k]
            assert torch.equal(a, b), (m, k)
            if a.is_floating_point():
                assert torch.isfinite(a).all(), (m, k)
