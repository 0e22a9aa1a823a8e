"""Tabled gather grouped-conv kernels (ops/csrc/conv_mfma.hip) against the
untabled gather kernels they replace (bit-exact, HETEROFL_CONV_TABLED=0) and
against F.conv2d / autograd on fp32 copies, and which of the two every
flagship gather shape takes.  Run with: pytest tests -m gpu"""
import contextlib
import functools
import os

import pytest
import torch

from tests.conftest import make_cfg

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

FWD, BWD_DATA, BWD_WEIGHT = 'fwd', 'bwd_data', 'bwd_weight'
T_FWD = 'conv_fwd_tabled_kernel'
T_BD = 'conv_bwd_data_tabled_kernel'
T_BD2 = 'conv_bwd_data_s2_tabled_kernel'
T_BW = 'conv_bwd_weight_tabled_kernel'
O_FWD = 'conv_fwd_kernel'
O_BD = 'conv_bwd_data_kernel'
O_BW = 'conv_bwd_weight_kernel'

# name: ((G, N, Cin, H, Cout, k, stride, pad),
#        {direction: (route, split or None, kernel)} the case is there for)
CASES = {
    # 4x4 planes, one ragged 48-pixel tile spanning three samples; K=360 has
    # a ragged last chunk; fwd split 4 = slices of 96 k, the second starting
    # mid-channel (cin 10, tap 6)
    'plane4': ((2, 3, 40, 4, 24, 3, 1, 1),
               {FWD: ('gather', 4, T_FWD), BWD_DATA: ('gather', None, T_BD),
                BWD_WEIGHT: ('gather', None, T_BW)}),
    # K=2304, one tile, split 32 with 8 empty slices
    'deep': ((1, 1, 256, 4, 64, 3, 1, 1),
             {FWD: ('gather', 32, T_FWD), BWD_DATA: ('gather', None, T_BD),
              BWD_WEIGHT: ('gather', None, T_BW)}),
    # 2x2 planes: every tap row / column leaves the image for some pixel
    'plane2': ((2, 5, 24, 2, 40, 3, 1, 1),
               {FWD: ('gather', None, T_FWD),
                BWD_DATA: ('gather', None, T_BD),
                BWD_WEIGHT: ('gather', None, T_BW)}),
    # L4d-like and L3d-like: gather fwd, parity bwd-data with all four
    # classes, ragged M
    'l4d': ((2, 3, 20, 8, 36, 3, 2, 1),
            {FWD: ('gather', None, T_FWD), BWD_DATA: ('gather_s2', None, T_BD2),
             BWD_WEIGHT: ('gather', None, T_BW)}),
    'l3d': ((2, 2, 20, 16, 36, 3, 2, 1),
            {FWD: ('gather', None, T_FWD),
             BWD_DATA: ('gather_s2', None, T_BD2)}),
    # odd H: stride-2 bwd-data takes the any-geometry kernel's stride-2 branch
    'odd': ((2, 3, 20, 7, 36, 3, 2, 1),
            {FWD: ('gather', None, T_FWD), BWD_DATA: ('gather', None, T_BD),
             BWD_WEIGHT: ('gather', None, T_BW)}),
    # shortcuts; sc_k4 has K=4: a single ragged chunk, K % 4 == 0 but M < 64
    'sc': ((2, 2, 64, 8, 36, 1, 2, 0),
           {FWD: ('gather', None, T_FWD), BWD_DATA: ('gather_s2', None, T_BD2),
            BWD_WEIGHT: ('gather', None, T_BW)}),
    'sc_k4': ((3, 2, 4, 8, 8, 1, 2, 0),
              {FWD: ('gather', None, T_FWD),
               BWD_DATA: ('gather_s2', None, T_BD2),
               BWD_WEIGHT: ('gather', None, T_BW)}),
    # K=27: K % 4 != 0, no vector weight loads
    'k27': ((2, 2, 3, 8, 20, 3, 2, 1),
            {FWD: ('gather', None, T_FWD),
             BWD_DATA: ('gather_s2', None, T_BD2),
             BWD_WEIGHT: ('gather', None, T_BW)}),
    # one over each table capacity (1024 k / j entries per slice, 256 pixels
    # per p-chunk): unsplit slices of 1152 k, 1152 j, a 294-pixel chunk; the
    # untabled kernel runs, toggle either way
    'cap_fwd': ((64, 21, 128, 7, 8, 3, 1, 1), {FWD: ('gather', 1, O_FWD)}),
    'cap_bwdD': ((64, 21, 8, 7, 128, 3, 1, 1),
                 {BWD_DATA: ('gather', 1, O_BD)}),
    'cap_bwdW': ((64, 6, 64, 7, 64, 3, 1, 1),
                 {BWD_WEIGHT: ('gather', 1, O_BW)}),
}
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
PARAMS = [(c, d) for c in CASES for d in DTYPES]
KEY_DIR = {'fwd': FWD, 'fwd_bias': FWD, 'fwd_res': FWD, 'bwdD': BWD_DATA,
           'bwdW': BWD_WEIGHT}


@contextlib.contextmanager
def tabled(on):
    prev = os.environ.get('HETEROFL_CONV_TABLED')
    os.environ['HETEROFL_CONV_TABLED'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_CONV_TABLED']
        else:
            os.environ['HETEROFL_CONV_TABLED'] = prev


def plan(direction, geom, esz, fp8=0):
    """(route, split, kernel name) from the launchers' own plan functions"""
    from heterofl_amd.ops.fused import conv_plan, conv_plan_variant
    G, N, Cin, H, Cout, k, s, p = geom
    route, split, lds = conv_plan(direction, G, N, Cin, H, H, Cout, k, s, p,
                                  esz, fp8)
    assert lds == 0 or route == 'resident', (direction, geom, route, lds)
    return route, split, conv_plan_variant(direction, G, N, Cin, H, H, Cout,
                                           k, s, p, esz, fp8)


def untabled(kernel):
    return kernel.replace('_tabled_kernel', '_kernel')


@functools.lru_cache(maxsize=None)
def results(case, dname):
    """Every native result of one case, toggle on ('new') and off ('old'),
    plus the fp32 torch references; computed once per (case, dtype)."""
    import torch.nn.functional as F
    from heterofl_amd.ops import require_native
    ext = require_native()
    G, N, Cin, H, Cout, k, s, p = CASES[case][0]
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
        with tabled(on):
            out[tag] = {
                'fwd': ext.conv_fwd(x, w, none, none, G, s, p, 0),
                'fwd_bias': ext.conv_fwd(x, w, b, none, G, s, p, 0),
                'fwd_res': ext.conv_fwd(x, w, b, res, G, s, p, 0),
                'bwdD': ext.conv_bwd_data(dy, w, G, s, p, H, H, 0),
                'bwdW': ext.conv_bwd_weight(dy, x, G, s, p, k, 0)}
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
    geom, want = CASES[case]
    esz = {'bf16': 2, 'fp32': 4}[dname]
    # the case has the property it is there for
    d = KEY_DIR[key]
    if d in want:
        route, split, kernel = want[d]
        with tabled(True):
            got = plan(d, geom, esz)
        assert got[0] == route and got[2] == kernel, (case, d, got)
        assert split is None or got[1] == split, (case, d, got)
        with tabled(False):
            assert plan(d, geom, esz) == (got[0], got[1], untabled(kernel)), \
                (case, d)
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
def test_tabled_fwd(case, dname, key):
    G, N, Cin, H, Cout, k, s, p = CASES[case][0]
    check(case, dname, key, 5e-4 * Cin * k)


@needs_gpu
@pytest.mark.parametrize('case,dname', PARAMS)
def test_tabled_bwd_data(case, dname):
    G, N, Cin, H, Cout, k, s, p = CASES[case][0]
    check(case, dname, 'bwdD', 5e-4 * Cout * k)


@needs_gpu
@pytest.mark.parametrize('case,dname', PARAMS)
def test_tabled_bwd_weight(case, dname):
    G, N, Cin, H, Cout, k, s, p = CASES[case][0]
    check(case, dname, 'bwdW', 5e-3 * N * H)


@needs_gpu
@pytest.mark.parametrize('dname', list(DTYPES))
def test_tabled_fwd_misaligned_weight(dname):
    """A weight tensor that is a 4-byte-offset view of a larger buffer: K % 4
    == 0 but the base is not 16-byte aligned, so the scalar weight path runs,
    and agrees with the untabled kernel and with the aligned tensor."""
    from heterofl_amd.ops import require_native
    ext = require_native()
    G, N, Cin, H, Cout, k, s, p = CASES['sc'][0]
    dt = DTYPES[dname]
    torch.manual_seed(0)
    x = torch.randn(N, G * Cin, H, H, device='cuda').to(dt)
    w = torch.randn(G * Cout, Cin, k, k, device='cuda') * 0.1
    buf = torch.zeros(w.numel() + 4, device='cuda')
    wv = buf[1:1 + w.numel()].view_as(w)
    wv.copy_(w)
    assert w.data_ptr() % 16 == 0 and wv.data_ptr() % 16 == 4
    assert wv.is_contiguous() and (Cin * k * k) % 4 == 0
    none = torch.Tensor()
    with tabled(True):
        assert plan(FWD, CASES['sc'][0], x.element_size())[2] == T_FWD
        y_aligned = ext.conv_fwd(x, w, none, none, G, s, p, 0)
        y_view = ext.conv_fwd(x, wv, none, none, G, s, p, 0)
    with tabled(False):
        y_old = ext.conv_fwd(x, wv, none, none, G, s, p, 0)
    assert torch.equal(y_view, y_aligned)
    assert torch.equal(y_view, y_old)


# ----------------------------------------------------------------- plan table
# The flagship's gather shapes (N=10, full width and the rate-1/16 widths,
# groups of 1, 5 and 10 clients: 10 are active per round, and the splits and
# with them the slice lengths depend on G) as (Cin, H, Cout, k, stride, pad)
# -> directions on a gather route.
ALL3 = (FWD, BWD_DATA, BWD_WEIGHT)
FLAGSHIP = {
    'L2d': ((64, 32, 128, 3, 2, 1), (BWD_DATA,)),
    'L3d': ((128, 16, 256, 3, 2, 1), (FWD, BWD_DATA)),
    'L4d': ((256, 8, 512, 3, 2, 1), ALL3),
    'L4': ((512, 4, 512, 3, 1, 1), ALL3),
    'sc2': ((64, 32, 128, 1, 2, 0), ALL3),
    'sc3': ((128, 16, 256, 1, 2, 0), ALL3),
    'sc4': ((256, 8, 512, 1, 2, 0), ALL3),
}
NEW = {FWD: (T_FWD,), BWD_DATA: (T_BD, T_BD2), BWD_WEIGHT: (T_BW,)}


@needs_gpu
@pytest.mark.parametrize('shape', list(FLAGSHIP))
@pytest.mark.parametrize('div', [1, 16])
@pytest.mark.parametrize('G', [1, 5, 10])
def test_tabled_plan_flagship(shape, div, G):
    (Cin, H, Cout, k, s, p), dirs = FLAGSHIP[shape]
    geom = (G, 10, Cin // div, H, Cout // div, k, s, p)
    for esz in (2, 4):
        for d in dirs:
            with tabled(True):
                route, split, kernel = plan(d, geom, esz)
                assert route in ('gather', 'gather_s2'), (shape, d, route)
                assert kernel in NEW[d], (shape, d, kernel)
                assert (route == 'gather_s2') == (kernel == T_BD2)
                # fp8 set: the untabled kernels, fp8 tiles for bf16 tensors
                r8, s8, k8 = plan(d, geom, esz, 1)
                assert s8 == split and '_tabled_' not in k8, (shape, d, k8)
                if esz == 2:
                    assert r8 == route + '_fp8', (shape, d, r8)
                    assert k8 == untabled(kernel) + '<fp8>', (shape, d, k8)
            with tabled(False):
                assert plan(d, geom, esz) == (route, split, untabled(kernel))
                assert '_tabled_' not in plan(d, geom, esz, 1)[2]


def graph_step(base_cfg, rate, batch):
    """Parameters after a captured ResNet18 group step (R=2, 16 synthetic
    samples) with the toggle on and off."""
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
    cfg['batch_size'] = dict(cfg['batch_size'], train=batch)
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=16)
    process_dataset(ds, cfg)
    torch.manual_seed(1)
    data_split, label_split = split_dataset(ds, 2, 'iid', 10)
    assert all(len(data_split['train'][u]) == 8 for u in range(2))
    torch.manual_seed(2)
    gp = make_model(cfg, model_rate=rate).to('cuda:0').state_dict()
    user_idx = [0, 1]
    rates = [rate, rate]
    results_ = {}
    for on in (True, False):
        with tabled(on):
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


@needs_gpu
def test_tabled_graph_step_bit_identical(base_cfg):
    """A captured ResNet18 group step (rate 0.0625, R=2, batch 4, 2 replays)
    trains to bit-identical parameters with the toggle on and off."""
    graph_step(base_cfg, 0.0625, 4)


@needs_gpu
def test_tabled_graph_step_rate1_bit_identical(base_cfg):
    """The same at rate 1 (the 512-channel 4x4 layers) and batch 1, the
    smallest there is: the planes do not depend on the batch, and a 4x4 plane
    still gives BN 16 values per channel."""
    with tabled(True):
        assert plan(FWD, (2, 1, 512, 4, 512, 3, 1, 1), 2)[2] == T_FWD
    graph_step(base_cfg, 1.0, 1)
