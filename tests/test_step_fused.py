"""CPU checks of the HETEROFL_STEP_FUSED wiring on the torch path: the
head + CE helper (fed.batched.step_losses / step_grads), the blocks'
forward_alias residual, and the torch fallback of the alias BN+ReLU
function."""
import torch

from heterofl_amd.fed import batched as B
from heterofl_amd.ops import fused as F


def _resnet(R=2, dtype=torch.float64, scale=True):
    torch.manual_seed(0)
    m = B.BatchedResNet(R, [3, 32, 32], [4, 8, 16, 32], [2, 2, 2, 2], 10,
                        1.0 / 16, 'bn', scale).to(dtype)
    m.train(True)
    return m


def _conv(R=2, dtype=torch.float64):
    torch.manual_seed(0)
    m = B.BatchedConv(R, [1, 28, 28], [4, 8, 8, 16], 10, 1.0 / 16, 'bn',
                      True).to(dtype)
    m.train(True)
    return m


def _batch(model, in_ch, hw, R=2, N=4):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, R * in_ch, hw, hw, generator=gen, dtype=torch.float64)
    y = torch.randint(0, 10, (N, R), generator=gen)
    masks = (torch.rand(R, 10, generator=gen) > 0.3).float()
    return x, y, masks


def _run(model, x, y, masks, fused):
    params = [p for p in model.parameters() if p.requires_grad]
    metrics = torch.zeros(model.R, 3, dtype=torch.float64)
    losses, scores = B.step_losses(model, x, y, masks, metrics=metrics,
                                   fused=fused)
    grads = B.step_grads(losses, params, fused=fused)
    return losses.detach(), scores.detach(), grads, metrics


def _same(a, b, tol=0.0):
    la, sa, ga, ma = a
    lb, sb, gb, mb = b
    pairs = [(la, lb), (sa, sb), (ma, mb)] + list(zip(ga, gb))
    for i, (p, q) in enumerate(pairs):
        assert p.shape == q.shape
        if tol == 0.0:
            assert torch.equal(p, q), i
        else:
            assert (p - q).abs().max().item() <= tol * (1 + q.abs().max().item()), i


def test_resnet_helper_matches_model_forward():
    """stop before the head + fused_head_ce's torch twin + ones as
    grad_outputs against model(x) + batched_masked_ce + losses.sum()"""
    m = _resnet()
    x, y, masks = _batch(m, 3, 32)
    _same(_run(m, x, y, masks, True), _run(m, x, y, masks, False))


def test_conv_helper_matches_model_forward():
    m = _conv()
    x, y, masks = _batch(m, 1, 28)
    _same(_run(m, x, y, masks, True), _run(m, x, y, masks, False))


def test_step_grads_accumulates_into_grad():
    m = _conv()
    x, y, masks = _batch(m, 1, 28)
    params = [p for p in m.parameters() if p.requires_grad]
    want = _run(m, x, y, masks, False)[2]
    for fused in (True, False):
        for p in params:
            p.grad = None
        losses, _ = B.step_losses(m, x, y, masks, fused=fused)
        B.step_grads(losses, fused=fused)
        for p, g in zip(params, want):
            assert torch.equal(p.grad, g)


def test_block_alias_wiring_matches_plain_blocks(monkeypatch):
    """Every shortcut-free block takes its residual from the alias output of
    its first BN+ReLU (the function's torch fallback here), so the block
    input has that one consumer and its gradient is summed inside the
    function's backward: same losses and parameter gradients as the plain
    modules, up to fp64 rounding.  Without the Scaler: like the kernels, the
    function leaves out x / rate, which cancels in a train-mode norm only up
    to eps."""
    m = _resnet(scale=False)
    x, y, masks = _batch(m, 3, 32)
    plain = _run(m, x, y, masks, False)
    calls = []

    def forward_alias(self, t):
        calls.append(self)
        return F.fused_norm_relu_alias(t, self.weight, self.bias)

    monkeypatch.setattr(B.BNormReLU, 'forward_alias', forward_alias)
    aliased = _run(m, x, y, masks, True)
    # resnet18: layer1 has two shortcut-free blocks, layers 2-4 one each
    assert len(calls) == 5
    _same(aliased, plain, tol=1e-9)


def test_alias_function_gradcheck():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(3, 4, 2, 3, generator=gen, dtype=torch.float64,
                    requires_grad=True)
    w = (torch.rand(4, generator=gen, dtype=torch.float64) + 0.5) \
        .requires_grad_()
    b = torch.randn(4, generator=gen, dtype=torch.float64).requires_grad_()

    def both(x, w, b):
        y, alias = F.fused_norm_relu_alias(x, w, b)
        return y, alias * 1.5

    def only_y(x, w, b):
        return F.fused_norm_relu_alias(x, w, b)[0]

    def only_alias(x, w, b):
        return F.fused_norm_relu_alias(x, w, b)[1]

    for fn in (both, only_y, only_alias):
        assert torch.autograd.gradcheck(fn, (x, w, b), eps=1e-6, atol=1e-6)


def test_alias_is_the_input():
    x = torch.randn(2, 3, 4, 4, dtype=torch.float64, requires_grad=True)
    w = torch.ones(3, dtype=torch.float64)
    b = torch.zeros(3, dtype=torch.float64)
    y, alias = F.fused_norm_relu_alias(x * 1.0, w, b)
    assert alias.shape == x.shape and torch.equal(alias, x)
    ref = torch.relu(torch.nn.functional.batch_norm(
        x, None, None, w, b, training=True, eps=1e-5))
    assert (y - ref).abs().max().item() < 1e-12
