"""GPU tests of the fused LM head kernel and the native masked-LM evaluator
(MI355X).  Run with: pytest tests -m gpu"""
import pytest
import torch
import torch.nn.functional as F

from heterofl_amd.ops.fused import lm_head_ce, lm_head_pack
from tests.conftest import make_cfg

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')
DEV = 'cuda:0'

# (M, E, V): one row / one ragged tile; ragged everything with E % 32 != 0;
# several row tiles at full K with a ragged last column tile; the real vocab
HEAD_CASES = [(1, 16, 33), (130, 40, 1000), (300, 256, 130),
              (64, 256, 33278)]
_head_cache = {}


def _head_case(shape, extras):
    """Inputs (bf16-representable), the fp32 host reference and the per-row
    error scale delta_i = max_j (Ep+1) 2^-23 (|x_i|.|W_j| + |b_j|); computed
    once per case and shared."""
    key = (shape, extras)
    if key not in _head_cache:
        M, E, V = shape
        g = torch.Generator().manual_seed(M + E + V)
        x = torch.randn(M, E, generator=g).bfloat16()
        w = (torch.randn(V, E, generator=g) * 0.2).bfloat16().float()
        labels = torch.randint(0, V, (M,), generator=g)
        bias = mask = None
        logits = x.float() @ w.t()
        A = x.float().abs() @ w.abs().t()
        if extras:
            bias = torch.randn(V, generator=g)
            mask = (torch.rand(V, generator=g) < 0.5).float()
            mask[labels[0]] = 0        # a masked label
            logits = (logits + bias).masked_fill(mask.view(1, V) == 0, 0)
            A = A + bias.abs()
        Ep = -(-E // 32) * 32
        delta = (Ep + 1) * 2.0 ** -23 * A.max(dim=1).values
        lse = torch.logsumexp(logits, dim=1)
        nll = F.cross_entropy(logits, labels, reduction='none')
        _head_cache[key] = {
            'x': x, 'w': w, 'labels': labels, 'bias': bias, 'mask': mask,
            'nll': nll, 'lse': lse, 'delta': delta}
    return _head_cache[key]


def _run_head(case, shape, splits):
    M, E, V = shape
    packed = lm_head_pack(case['w'].to(DEV), case['bias'] if case['bias']
                          is None else case['bias'].to(DEV))
    args = (case['x'].to(DEV), packed,
            None if case['bias'] is None else case['bias'].to(DEV),
            case['labels'].to(DEV),
            None if case['mask'] is None else case['mask'].to(DEV), V, E)
    return args, lm_head_ce(*args, splits=splits)


@needs_gpu
@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('splits', [1, 3, 0])
@pytest.mark.parametrize('shape', HEAD_CASES)
def test_lm_head_ce_matches_host(shape, splits, extras):
    """|nll - ref| <= 2 delta_i + V 2^-24 + 1e-5 and |lse - ref| <= delta_i +
    V 2^-24 + 1e-5 per row: fp32 accumulation error of the logits (twice for
    the NLL, which also subtracts the label's logit), fp32 summation of V
    positive terms, and the exp/log intrinsics."""
    M, E, V = shape
    case = _head_case(shape, extras)
    args, (nll, lse) = _run_head(case, shape, splits)
    torch.cuda.synchronize()
    assert nll.shape == (M,) and lse.shape == (M,)
    assert nll.dtype == torch.float32 and lse.dtype == torch.float32
    tail = V * 2.0 ** -24 + 1e-5
    e_nll = (nll.cpu() - case['nll']).abs() - (2 * case['delta'] + tail)
    e_lse = (lse.cpu() - case['lse']).abs() - (case['delta'] + tail)
    print('lm_head_ce', shape, 'splits', splits, 'extras', extras,
          'worst nll err - bound', e_nll.max().item(),
          'worst lse err - bound', e_lse.max().item())
    assert e_nll.max().item() <= 0 and e_lse.max().item() <= 0
    # no atomics: a second launch reproduces the result bit for bit
    nll2, lse2 = lm_head_ce(*args, splits=splits)
    assert torch.equal(nll, nll2) and torch.equal(lse, lse2)


@needs_gpu
@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('shape', HEAD_CASES)
def test_lm_head_ce_splits_agree(shape, extras):
    M, E, V = shape
    case = _head_case(shape, extras)
    _, (nll1, lse1) = _run_head(case, shape, 1)
    _, (nll3, lse3) = _run_head(case, shape, 3)
    tail = V * 2.0 ** -24 + 1e-5
    delta = case['delta'].to(DEV)
    assert ((nll1 - nll3).abs() - (2 * delta + tail)).max().item() <= 0
    assert ((lse1 - lse3).abs() - (delta + tail)).max().item() <= 0


@needs_gpu
@pytest.mark.parametrize('V,E', [(33, 16), (1000, 40), (130, 256)])
def test_lm_head_pack_layout(V, E):
    g = torch.Generator().manual_seed(V)
    w = torch.randn(V, E, generator=g)
    packed = lm_head_pack(w.to(DEV), None).cpu()
    Vp, Ep = -(-V // 64) * 64, -(-E // 32) * 32
    assert packed.dtype == torch.bfloat16 and packed.shape == (Vp, Ep)
    assert torch.equal(packed[:V, :E], w.bfloat16())
    assert Vp > V or Ep > E
    if Vp > V:
        assert packed[V:].float().abs().max().item() == 0
    if Ep > E:
        assert packed[:, E:].float().abs().max().item() == 0


# -------------------------------------------------------- NativeLMInference
def _window_losses(nll_of, src, label, windows):
    """Mean NLL of every (start, length) window."""
    return torch.tensor([
        nll_of(src[:, s:s + n].contiguous(), label[:, s:s + n].contiguous())
        .double().mean().item() for s, n in windows], dtype=torch.float64)


def _eager_nll(model, autocast):
    def run(src, label):
        with torch.no_grad(), torch.autocast('cuda', torch.bfloat16,
                                             enabled=autocast):
            x = model.transformer_embedding(src)
            for layer in model.transformer_encoder['layers']:
                x = layer(x)
            out = model.decoder(x).permute(0, 2, 1)
            return F.cross_entropy(out, label, reduction='none').float()
    return run


def _autocast_error(model, src, label, windows):
    """(eager fp32 window losses, e_autocast): the error of the existing
    eager model under bf16 autocast against its own fp32 run, on the same
    inputs.  It is the yardstick of the native evaluator's bf16 error: the
    same activation precision, and autocast additionally rounds the logits
    to bf16."""
    model.train(False)
    ref = _window_losses(_eager_nll(model, False), src, label, windows)
    ac = _window_losses(_eager_nll(model, True), src, label, windows)
    return ref, (ac - ref).abs().max().item()


@needs_gpu
@pytest.mark.parametrize('rate', [1.0, 0.0625])
def test_native_lm_inference_bf16(base_cfg, rate):
    """e_native <= 2 e_autocast over 8 windows (7 full + a tail of 25), and
    the fused and two-step heads agree within e_autocast.  The factor 2
    covers the different rounding points of the two bf16 pipelines.
    Measured on MI355X (profiles/lm_inferbench.txt): rate 1 e_native 4.2e-4,
    e_autocast 9.0e-4, fused vs gemm 6.8e-5; rate 0.0625 2.5e-4, 8.7e-4,
    4.8e-5."""
    from heterofl_amd.fed.infer import NativeLMInference
    from heterofl_amd.models import make_model
    V = 1000   # 15 full column tiles + 40 columns
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1-c1-e1_bn_1_1',
                   data_name='WikiText2', model_name='transformer',
                   num_tokens=V)
    torch.manual_seed(6)
    model = make_model(dict(cfg, global_model_rate=rate), model_rate=rate)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model = model.to(DEV)
    T = 7 * 64 + 25
    label = torch.randint(0, V, (10, T)).to(DEV)
    src = label.masked_fill((torch.rand(10, T) < 0.15).to(DEV), V)
    windows = [(s, min(64, T - s)) for s in range(0, T, 64)]
    ref, e_autocast = _autocast_error(model, src, label, windows)
    fused = _window_losses(NativeLMInference(model, head='fused').window_nll,
                           src, label, windows)
    gemm = _window_losses(NativeLMInference(model, head='gemm').window_nll,
                          src, label, windows)
    e_native = (fused - ref).abs().max().item()
    e_heads = (fused - gemm).abs().max().item()
    print('native LM evaluator rate', rate, 'e_native', e_native,
          'e_autocast', e_autocast, 'gemm head err',
          (gemm - ref).abs().max().item(), 'fused vs gemm', e_heads)
    assert e_native <= 2.0 * e_autocast, (rate, e_native, e_autocast)
    assert e_heads <= e_autocast, (rate, e_heads, e_autocast)


@needs_gpu
def test_lm_levels_gpu(base_cfg):
    """test_lm_levels on the device (batched engine, mask_rate 0): each
    level's loss is within 2 e_autocast(level) of the CPU oracle's."""
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    from tests.test_lm_infer import LM_METRICS, _oracle_lm_level
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1-c1-e1_bn_1_1',
                   data_name='WikiText2', model_name='transformer')
    cfg['metric_name'] = LM_METRICS
    cfg['mask_rate'] = 0.0
    cfg['device'] = DEV
    cfg['engine'] = 'batched'
    torch.manual_seed(0)
    ds = fetch_dataset('WikiText2', synthetic=True, synthetic_size=20_000)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 4, 'iid')
    model = make_model(cfg)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    model = model.to(DEV)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    levels = runner.test_lm_levels(1)
    assert sorted(levels) == [0.0625, 0.25, 1.0]
    tokens, windows = runner._stage_lm_eval()
    assert windows[-1][1] < cfg['bptt']
    # the CPU oracle: same parameters, eager fp32 on the host
    cpu_cfg = dict(cfg, device='cpu')
    cpu_model = make_model(cpu_cfg)
    cpu_model.load_state_dict({k: v.cpu()
                               for k, v in model.state_dict().items()})
    cpu_runner = FedRunner(cpu_cfg, ds, data_split, label_split, cpu_model,
                           make_optimizer(cpu_model, cfg['lr'], cpu_cfg))
    mask = torch.zeros(tuple(tokens.shape))
    for rate, got in levels.items():
        ref = _oracle_lm_level(cpu_runner, ds, cpu_cfg, rate, mask)
        _, e_autocast = _autocast_error(runner.level_models[rate], tokens,
                                        tokens, windows)
        err = abs(got['Global-Loss'] - ref['Global-Loss'])
        print('LM level', rate, 'loss', got['Global-Loss'], 'cpu oracle',
              ref['Global-Loss'], 'err', err, 'e_autocast', e_autocast)
        assert err <= 2.0 * e_autocast, (rate, err, e_autocast)
