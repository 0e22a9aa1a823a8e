"""The vision step's glue kernels behind HETEROFL_STEP_FUSED: batch_gather
(ops/csrc/batch_gather.hip) against the two index_selects and the counter add
it replaces, bn_relu_bwd_add against bn_relu_bwd(...)[0] + addend on every
route, and one captured resnet18 step with the switch on against off.  All
comparisons are bit-equality.
"""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

DEV = 'cuda:0'


def ext():
    from heterofl_amd.ops import require_native
    return require_native()


@contextlib.contextmanager
def step_fused(on):
    prev = os.environ.get('HETEROFL_STEP_FUSED')
    os.environ['HETEROFL_STEP_FUSED'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_STEP_FUSED']
        else:
            os.environ['HETEROFL_STEP_FUSED'] = prev


# ============================================================== batch_gather
CAP, R = 30, 5
GATHER = {
    # rows of 15 x 32 x 32 bf16: 16-byte accesses
    'bf16-rows': ((R * 3, 32, 32), torch.bfloat16),
    # rows of 300 bytes, no multiple of 16: element accesses
    'fp32-odd': ((3, 5, 5), torch.float32),
}


def _buffers(kind):
    shape, dtype = GATHER[kind]
    gen = torch.Generator().manual_seed(11)
    x_all = torch.randn(CAP, *shape, generator=gen).to(dtype).to(DEV)
    y_all = torch.randint(0, 10, (CAP, R), generator=gen).to(DEV)
    return x_all, y_all


@needs_gpu
@pytest.mark.parametrize('B', [1, 10])
@pytest.mark.parametrize('kind', list(GATHER))
def test_batch_gather_eager(kind, B):
    from heterofl_amd.ops.fused import batch_gather
    x_all, y_all = _buffers(kind)
    counter = torch.zeros(1, dtype=torch.long, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in range(3):
        idx = torch.arange(step * B, (step + 1) * B, device=DEV)
        xb, yb = batch_gather(x_all, y_all, counter, B, ticket)
        torch.cuda.synchronize()
        assert xb.shape == (B,) + x_all.shape[1:] and xb.dtype == x_all.dtype
        assert torch.equal(xb, x_all.index_select(0, idx)), step
        assert torch.equal(yb, y_all.index_select(0, idx)), step
        assert counter.item() == step + 1
        assert ticket.item() == 0


@needs_gpu
@pytest.mark.parametrize('B', [1, 10])
@pytest.mark.parametrize('kind', list(GATHER))
def test_batch_gather_replay(kind, B):
    """One call in a captured graph: every replay fetches the next batch and
    needs no host work in between."""
    from heterofl_amd.ops.fused import batch_gather
    x_all, y_all = _buffers(kind)
    counter = torch.zeros(1, dtype=torch.long, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    batch_gather(x_all, y_all, counter, B, ticket)      # warm-up
    counter.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        xb, yb = batch_gather(x_all, y_all, counter, B, ticket)
    for step in range(3):
        g.replay()
        torch.cuda.synchronize()
        idx = torch.arange(step * B, (step + 1) * B, device=DEV)
        assert torch.equal(xb, x_all.index_select(0, idx)), step
        assert torch.equal(yb, y_all.index_select(0, idx)), step
        assert counter.item() == step + 1
        assert ticket.item() == 0


@needs_gpu
def test_batch_gather_past_the_buffer_returns_zeros():
    """A counter past the last whole batch: nothing is read out of bounds,
    the outputs are all zero, the counter still advances, the ticket is back
    at 0."""
    from heterofl_amd.ops.fused import batch_gather
    x_all, y_all = _buffers('fp32-odd')
    counter = torch.full((1,), 3, dtype=torch.long, device=DEV)   # 3 * 10
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    xb, yb = batch_gather(x_all, y_all, counter, 10, ticket)
    torch.cuda.synchronize()
    assert counter.item() == 4 and ticket.item() == 0
    assert bool((xb == 0).all()) and bool((yb == 0).all())


# =========================================================== bn_relu_bwd_add
# smallest shape of each backward route: name -> ((N, C, H, W), {io: route})
BN_ADD = {
    'vec': ((2, 3, 4, 4), {'fp32': 'vec', 'bf16': 'vec'}),
    'staged': ((2, 3, 5, 1), {'fp32': 'staged', 'bf16': 'staged'}),
    # 2 * N * HW * esz over the 64 KB stage in both dtypes
    'direct': ((5, 2, 64, 64), {'fp32': 'direct', 'bf16': 'direct'}),
}
IO = {'fp32': torch.float32, 'bf16': torch.bfloat16}


@needs_gpu
@pytest.mark.parametrize('io_name', list(IO))
@pytest.mark.parametrize('name', list(BN_ADD))
def test_bn_relu_bwd_add(name, io_name):
    """dx has the bits of the separate add of the two tensors in their own
    dtype, round_T(float(round_T(dx)) + float(addend)); dgamma and dbeta are
    bn_relu_bwd's.  In bf16 that is two roundings: the fp32 kernel on the same
    (bf16-valued) inputs gives dx before its rounding, and among the random
    addends some must round differently added to that than added to the
    rounded dx, or the test would not tell the two apart."""
    from heterofl_amd.ops.fused import bn_relu_route
    shape, routes = BN_ADD[name]
    N, C, H, W = shape
    dt = IO[io_name]
    assert bn_relu_route('bwd', N, C, H * W, 2 if io_name == 'bf16' else 4) \
        == routes[io_name]
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=gen).to(dt).to(DEV)
    dy = torch.randn(shape, generator=gen).to(dt).to(DEV)
    ad = torch.randn(shape, generator=gen).to(dt).to(DEV)
    w = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    b = torch.randn(C, generator=gen).to(DEV)
    e = ext()
    _, mean, invstd = e.bn_relu_fwd(x, w, b, 1e-5)
    dx0, dg0, db0 = e.bn_relu_bwd(dy, x, w, b, mean, invstd)
    dx1, dg1, db1 = e.bn_relu_bwd_add(dy, x, w, b, mean, invstd, ad)
    torch.cuda.synchronize()
    assert dx1.dtype == dt
    assert torch.equal(dx1, dx0 + ad)
    assert torch.equal(dg1, dg0) and torch.equal(db1, db0)
    if io_name == 'bf16':
        dx32 = e.bn_relu_bwd(dy.float(), x.float(), w, b, mean, invstd)[0]
        once = (dx32 + ad.float()).to(dt)
        twice = (dx32.to(dt).float() + ad.float()).to(dt)
        torch.cuda.synchronize()
        differ = int((once != twice).sum().item())
        print('bn_relu_bwd_add {}: {} of {} elements round differently once '
              'than twice'.format(name, differ, dx32.numel()))
        assert differ > 0
        assert torch.equal(dx1, twice)


@needs_gpu
def test_bn_relu_bwd_add_rejects_mismatched_addend():
    e = ext()
    x = torch.randn(2, 3, 4, 4, device=DEV)
    w = torch.ones(3, device=DEV)
    b = torch.zeros(3, device=DEV)
    _, mean, invstd = e.bn_relu_fwd(x, w, b, 1e-5)
    with pytest.raises(RuntimeError, match='addend'):
        e.bn_relu_bwd_add(x, x, w, b, mean, invstd, x[:1])


# ================================================================ whole step
def _graphed(seed, fused_on):
    from heterofl_amd.fed.batched import BatchedResNet
    from heterofl_amd.fed.graphs import GraphedGroupStep
    R2, batch = 2, 4
    torch.manual_seed(seed)
    model = BatchedResNet(R2, [3, 32, 32], [4, 8, 16, 32], [2, 2, 2, 2], 10,
                          1.0 / 16, 'bn', True).to(DEV)
    model.train(True)
    gs = GraphedGroupStep(model, R2, batch, 0.05, 0.9, 5e-4, 10, 3 * batch,
                          True, torch.device(DEV))
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(3 * batch, R2 * 3, 32, 32, generator=gen).to(DEV)
    y = torch.randint(0, 10, (3 * batch, R2), generator=gen).to(DEV)
    masks = (torch.rand(R2, 10, generator=gen) > 0.3).float().to(DEV)
    with step_fused(fused_on):
        gs.begin_round(masks)
        gs.run_epochs(x.to(torch.bfloat16), y, 3)      # captures, 3 replays
    torch.cuda.synchronize()
    return gs


@needs_gpu
def test_captured_step_switch_on_equals_off():
    """resnet18 at rate 1/16, R = 2, batch 4, bf16: parameters, momentum
    buffers, metrics and the counter after 3 replays."""
    on = _graphed(5, True)
    off = _graphed(5, False)
    assert on.counter.item() == 3 and off.counter.item() == 3
    assert on._ticket.item() == 0
    assert torch.equal(on.metrics, off.metrics), (on.metrics, off.metrics)
    assert bool((on.metrics[:, 2] == 12).all())
    for i, (a, b) in enumerate(zip(on.params, off.params)):
        assert torch.equal(a, b), ('param', i)
    for i, (a, b) in enumerate(zip(on.bufs, off.bufs)):
        assert torch.equal(a, b), ('momentum', i)
    assert any(bool((b != 0).any()) for b in on.bufs)
