"""16-byte-per-lane routes of the streaming kernels (HETEROFL_STREAM_VEC, on
by default): BN+ReLU fwd/bwd (ops/csrc/fused_norm.hip), the split reduces
(ops/csrc/conv_mfma.hip) and clip+SGD (ops/csrc/clip_sgd.hip).  Every output
must be bit-equal to the kernels they replace (HETEROFL_STREAM_VEC=0); the BN
route is also held against an fp64 reference with the tolerances of
tests/test_gpu.py::test_fused_bn_relu_matches_torch.
Run with: pytest tests -m gpu"""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}


@contextlib.contextmanager
def stream_vec(on):
    prev = os.environ.get('HETEROFL_STREAM_VEC')
    os.environ['HETEROFL_STREAM_VEC'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_STREAM_VEC']
        else:
            os.environ['HETEROFL_STREAM_VEC'] = prev


def ext():
    from heterofl_amd.ops import require_native
    return require_native()


# ------------------------------------------------------------------ BN+ReLU
# (N, C, H, W): route expected per dtype for (fwd, bwd)
BN_SHAPES = {
    'slow32': (10, 20, 32, 32),   # 40 trips per lane
    'p4': (10, 8, 4, 4),          # 160 elements < 256 lanes, 20 vectors
    'e192': (3, 5, 8, 8),         # 192 elements, not a multiple of 256
    'hw24': (2, 3, 4, 6),         # a lane's stride crosses samples
    'hw12': (7, 4, 2, 6),         # vector route for fp32 only
    'p7': (4, 3, 7, 7),           # fallback
}
# (fwd, bwd) routes of the (case, dtype) pairs that take the vector route;
# every other pair takes it in neither direction.  slow32 in fp32 stages
# 2 x 40 KB in the backward: over the LDS stage, the direct kernel.
BN_VEC = {('slow32', 'bf16'): ['vec', 'vec'],
          ('slow32', 'fp32'): ['vec', 'direct'],
          ('p4', 'bf16'): ['vec', 'vec'], ('p4', 'fp32'): ['vec', 'vec'],
          ('e192', 'bf16'): ['vec', 'vec'], ('e192', 'fp32'): ['vec', 'vec'],
          ('hw24', 'bf16'): ['vec', 'vec'], ('hw24', 'fp32'): ['vec', 'vec'],
          ('hw12', 'fp32'): ['vec', 'vec']}


def bn_inputs(shape, dt, affine, offset=0):
    g = torch.Generator().manual_seed(7)
    n = 1
    for s in shape:
        n *= s
    C = shape[1]
    flat = torch.randn(n + offset, generator=g).to(dt).cuda()
    x = flat[offset:].view(shape)
    dy = torch.randn(shape, generator=g).to(dt).cuda()
    if affine:
        w = (torch.rand(C, generator=g) + 0.5).cuda()
        b = torch.randn(C, generator=g).cuda()
    else:
        w = b = torch.Tensor()
    return x, dy, w, b


def bn_run(x, dy, w, b, on, bwd=True):
    e = ext()
    with stream_vec(on):
        y, mean, invstd = e.bn_relu_fwd(x, w, b, 1e-5)
        out = [y, mean, invstd]
        if bwd:
            out += e.bn_relu_bwd(dy, x, w, b, mean, invstd)
    torch.cuda.synchronize()
    return out


NAMES = ['y', 'mean', 'invstd', 'dx', 'dgamma', 'dbeta']


@needs_gpu
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('case', list(BN_SHAPES))
def test_bn_vec_bit_equal(case, dname, affine):
    from heterofl_amd.ops.fused import bn_relu_route
    shape = BN_SHAPES[case]
    dt = DTYPES[dname]
    N, C, HW = shape[0], shape[1], shape[2] * shape[3]
    esz = 2 if dname == 'bf16' else 4
    with stream_vec(True):
        routes = [bn_relu_route(d, N, C, HW, esz) for d in ('fwd', 'bwd')]
    if (case, dname) in BN_VEC:
        assert routes == BN_VEC[(case, dname)], routes
    else:
        assert 'vec' not in routes, routes
    with stream_vec(False):
        assert 'vec' not in [bn_relu_route(d, N, C, HW, esz)
                             for d in ('fwd', 'bwd')]
    x, dy, w, b = bn_inputs(shape, dt, affine)
    off = bn_run(x, dy, w, b, False)
    on = bn_run(x, dy, w, b, True)
    for name, a, c in zip(NAMES, off, on):
        assert torch.equal(a, c), (name, case, dname)


@needs_gpu
def test_bn_flagship_planes_take_vec_route():
    from heterofl_amd.ops.fused import bn_relu_route
    with stream_vec(True):
        for H, width in [(32, 64), (16, 128), (8, 256), (4, 512)]:
            for C in (5 * width, 5 * width // 16):
                for d in ('fwd', 'bwd'):
                    assert bn_relu_route(d, 10, C, H * H, 2) == 'vec', (H, C)


@needs_gpu
def test_bn_nonstaged_route_bit_equal():
    """80 KB of bf16 per channel: over the LDS stage, the direct kernel."""
    from heterofl_amd.ops.fused import bn_relu_route
    shape = (10, 2, 64, 64)
    with stream_vec(True):
        assert bn_relu_route('fwd', 10, 2, 64 * 64, 2) == 'direct'
    x, dy, w, b = bn_inputs(shape, torch.bfloat16, True)
    off = bn_run(x, dy, w, b, False, bwd=False)
    on = bn_run(x, dy, w, b, True, bwd=False)
    for name, a, c in zip(NAMES, off, on):
        assert torch.equal(a, c), name


@needs_gpu
@pytest.mark.parametrize('dname', list(DTYPES))
def test_bn_misaligned_base_falls_back(dname):
    """A contiguous view one element into a flat buffer: no 16-byte loads."""
    from heterofl_amd.ops.fused import bn_relu_route
    shape = (3, 5, 8, 8)
    esz = 2 if dname == 'bf16' else 4
    with stream_vec(True):
        assert bn_relu_route('fwd', 3, 5, 64, esz, aligned=False) != 'vec'
        assert bn_relu_route('bwd', 3, 5, 64, esz, aligned=False) != 'vec'
    x, dy, w, b = bn_inputs(shape, DTYPES[dname], True, offset=1)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    ref = bn_inputs(shape, DTYPES[dname], True, offset=1)[0].clone()
    off = bn_run(x, dy, w, b, False)
    on = bn_run(x, dy, w, b, True)
    for name, a, c in zip(NAMES, off, on):
        assert torch.equal(a, c), name
    # and agrees with the same values at an aligned base (the vec route)
    al = bn_run(ref, dy, w, b, True)
    assert ref.data_ptr() % 16 == 0
    for name, a, c in zip(NAMES, on, al):
        assert torch.equal(a, c), name


@needs_gpu
@pytest.mark.parametrize('case', ['slow32', 'p4', 'e192', 'hw24', 'hw12'])
def test_bn_vec_matches_fp64(case):
    """fp32 instantiation of the vector route against torch in fp64, with
    the bounds of test_fused_bn_relu_matches_torch: 1e-4 on y and dx, 2e-3
    on dgamma and dbeta.  (bf16 outputs round at 2^-9 relative and are tied
    to these through the bit-equality tests above: the old bf16 kernels are
    what the rest of the suite checks.)"""
    shape = BN_SHAPES[case]
    x, dy, w, b = bn_inputs(shape, torch.float32, True)
    y, mean, invstd, dx, dgamma, dbeta = bn_run(x, dy, w, b, True)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    ref = F.relu(F.batch_norm(x64, None, None, w64, b64, training=True,
                              eps=1e-5))
    ref.backward(dy.double())
    m64 = x.double().mean(dim=(0, 2, 3))
    is64 = 1.0 / torch.sqrt(x.double().var(dim=(0, 2, 3), unbiased=False)
                            + 1e-5)
    figs = {'y': (y.double() - ref).abs().max().item(),
            'mean': (mean.double() - m64).abs().max().item(),
            'invstd': (invstd.double() - is64).abs().max().item(),
            'dx': (dx.double() - x64.grad).abs().max().item(),
            'dgamma': (dgamma.double() - w64.grad).abs().max().item(),
            'dbeta': (dbeta.double() - b64.grad).abs().max().item()}
    print(case, figs)
    assert figs['y'] < 1e-4
    assert figs['mean'] < 1e-4 and figs['invstd'] < 1e-4
    assert figs['dx'] < 1e-4
    assert figs['dgamma'] < 2e-3 and figs['dbeta'] < 2e-3


# ------------------------------------------------------------ split reduces
# (G, N, Cin, H, Cout): 3x3, stride 1, pad 1
def conv_inputs(G, N, Cin, H, Cout, dt):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, G * Cin, H, H, generator=g).to(dt).cuda()
    w = (torch.randn(G * Cout, Cin, 3, 3, generator=g) * 0.1).cuda()
    bias = torch.randn(G * Cout, generator=g).cuda()
    res = torch.randn(N, G * Cout, H, H, generator=g).to(dt).cuda()
    dy = torch.randn(N, G * Cout, H, H, generator=g).to(dt).cuda()
    return x, w, bias, res, dy


def assert_split(direction, G, N, Cin, H, Cout, esz):
    from heterofl_amd.ops.fused import conv_plan
    split = conv_plan(direction, G, N, Cin, H, H, Cout, 3, 1, 1, esz, 0)[1]
    assert split > 1, (direction, split)


def both(fn):
    with stream_vec(False):
        a = fn()
    with stream_vec(True):
        b = fn()
    torch.cuda.synchronize()
    return a, b


@needs_gpu
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('mode', ['bias_res', 'plain', 'bwd_data'])
def test_out_reduce_vec_bit_equal(mode, dname):
    G, N, Cin, H, Cout = 2, 2, 16, 8, 8
    dt = DTYPES[dname]
    esz = 2 if dname == 'bf16' else 4
    x, w, bias, res, dy = conv_inputs(G, N, Cin, H, Cout, dt)
    e = ext()
    none = torch.Tensor()
    if mode == 'bwd_data':
        # bwd-data reduces over Cout * 9: the channel counts swap places so
        # that its reduction is the 144 that splits in two (72 does not) and
        # dx still has 2048 elements
        Cin, Cout = Cout, Cin
        x, w, bias, res, dy = conv_inputs(G, N, Cin, H, Cout, dt)
        assert_split('bwd_data', G, N, Cin, H, Cout, esz)
        a, b = both(lambda: e.conv_bwd_data(dy, w, G, 1, 1, H, H, 0))
    else:
        assert_split('fwd', G, N, Cin, H, Cout, esz)
        bb, rr = (bias, res) if mode == 'bias_res' else (none, none)
        a, b = both(lambda: e.conv_fwd(x, w, bb, rr, G, 1, 1, 0))
    assert a.numel() == 2048
    assert torch.equal(a, b)


@needs_gpu
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('N', [4, 1])
def test_out_reduce_straddle_and_scalar(N, dname):
    """N=4: total 300 is divisible by 4, chanstride 25 is not, so a vector
    straddles channels.  N=1: total 75, the scalar route."""
    G, Cin, H, Cout = 1, 16, 5, 3
    dt = DTYPES[dname]
    esz = 2 if dname == 'bf16' else 4
    x, w, bias, res, dy = conv_inputs(G, N, Cin, H, Cout, dt)
    assert_split('fwd', G, N, Cin, H, Cout, esz)
    e = ext()
    a, b = both(lambda: e.conv_fwd(x, w, bias, torch.Tensor(), G, 1, 1, 0))
    assert a.numel() == N * 75
    assert torch.equal(a, b)
    # the bias reaches the right channel
    ref = F.conv2d(x.float(), w, bias, 1, 1)
    assert (b.float() - ref).abs().max().item() < (0.1 if esz == 2 else 1e-3)


@needs_gpu
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('shape', [(2, 4, 16, 8, 8), (1, 4, 5, 8, 3)])
def test_splitp_reduce_vec_bit_equal(shape, dname):
    """GK = 2304 (float4 route) and GK = 135 (odd, the scalar kernel)."""
    G, N, Cin, H, Cout = shape
    dt = DTYPES[dname]
    esz = 2 if dname == 'bf16' else 4
    x, w, bias, res, dy = conv_inputs(G, N, Cin, H, Cout, dt)
    assert_split('bwd_weight', G, N, Cin, H, Cout, esz)
    e = ext()
    a, b = both(lambda: e.conv_bwd_weight(dy, x, G, 1, 1, 3, 0))
    assert a.numel() == G * Cout * Cin * 9
    assert torch.equal(a, b)


# ---------------------------------------------------------------- clip + SGD
R = 3
PER = [1, 10, 1728, 65540, 65537]


def sgd_run(on, with_shadows):
    from heterofl_amd.ops.fused import FusedClipSGD
    g = torch.Generator().manual_seed(3)
    params, grads, bufs, shadows = [], [], [], []
    for per in PER:
        p = torch.randn(R * per, generator=g)
        gr = torch.randn(2, R * per, generator=g)
        gr[:, :per] *= 1e-3          # client 0: norm below 1, not clipped
        params.append(p.cuda())
        grads.append(gr.cuda())
        bufs.append(torch.zeros(R * per, device='cuda'))
        shadows.append(p.to(torch.bfloat16).cuda() if with_shadows else None)
    cur = [gr[0].clone() for gr in grads]
    with stream_vec(on):
        opt = FusedClipSGD(params, cur, bufs, R, 'cuda',
                           shadows if with_shadows else None)
        norms = []
        for step in range(2):
            for c, gr in zip(cur, grads):
                c.copy_(gr[step])
            opt.step(1.0, 0.1, 0.9, 5e-4)
            norms.append(opt.normsq.clone())
            norms.append(opt.partials.clone())   # per chunk: nothing absorbs
    torch.cuda.synchronize()
    return params, bufs, [s for s in shadows if s is not None], norms


@needs_gpu
@pytest.mark.parametrize('with_shadows', [False, True])
def test_clip_sgd_vec_bit_equal(with_shadows):
    off = sgd_run(False, with_shadows)
    on = sgd_run(True, with_shadows)
    ns = off[3][0]
    assert ns[0].item() < 1.0 and ns[1].item() > 1.0 and ns[2].item() > 1.0
    for name, a, b in zip(('param', 'buf', 'shadow', 'normsq'), off, on):
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (name, i)
    if with_shadows:
        for p, s in zip(on[0], on[2]):
            assert torch.equal(p.to(torch.bfloat16), s)
