"""Native masked-LM evaluation — CPU side: the torch path of lm_head_ce,
NativeLMInference against the model's own sub-modules, the
HETEROFL_NATIVE_LM_EVAL knob of FedRunner.test, test_lm_levels and the
transformer branch of run_fed_eval.  The torch paths are the oracle for the
GPU kernels in test_gpu_lm_infer.py."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from heterofl_amd.data import BatchDataset, fetch_dataset, split_dataset
from heterofl_amd.fed import FedRunner
from heterofl_amd.fed.infer import NativeLMInference
from heterofl_amd.logger import Logger
from heterofl_amd.models import make_model
from heterofl_amd.ops.fused import lm_head_ce, lm_head_pack
from heterofl_amd.utils import process_dataset, make_optimizer
from tests.conftest import make_cfg

LEVELS = '1_4_0.5_iid_fix_a1-c1-e1_bn_1_1'
LM_METRICS = {'train': {'Local': ['Local-Loss', 'Local-Perplexity']},
              'test': {'Global': ['Global-Loss', 'Global-Perplexity']}}


# --------------------------------------------------------------- lm_head_ce
@pytest.mark.parametrize('masked', [False, True])
def test_lm_head_ce_torch_path(masked):
    V, E, M = 130, 40, 7
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, E, generator=g)
    w = torch.randn(V, E, generator=g) * 0.3
    b = torch.randn(V, generator=g)
    labels = torch.randint(0, V, (M,), generator=g)
    mask = None
    if masked:
        mask = (torch.rand(V, generator=g) < 0.6).float()
        mask[labels[0]] = 0   # a masked label
        mask[labels[1]] = 1
    packed = lm_head_pack(w, b)
    assert packed.shape == (192, 64)
    assert torch.equal(packed[:V, :E], w)
    assert packed[V:].abs().max() == 0 and packed[:, E:].abs().max() == 0
    nll, lse = lm_head_ce(x, packed, b, labels, mask, V, E)
    logits = x @ w.t() + b
    if masked:
        logits = logits.masked_fill(mask.view(1, V) == 0, 0)
    ref_nll = F.cross_entropy(logits, labels, reduction='none')
    ref_lse = torch.logsumexp(logits, dim=1)
    assert nll.shape == (M,) and lse.shape == (M,)
    assert (nll - ref_nll).abs().max().item() <= 1e-5
    assert (lse - ref_lse).abs().max().item() <= 1e-5


# --------------------------------------------------------------- window_nll
def _model_nll(model, src, label):
    """The model's own sub-modules, then F.cross_entropy per token."""
    with torch.no_grad():
        model.train(False)
        x = model.transformer_embedding(src)
        for layer in model.transformer_encoder['layers']:
            x = layer(x)
        out = model.decoder(x).permute(0, 2, 1)
        return F.cross_entropy(out, label, reduction='none')


@pytest.mark.parametrize('rate', [1.0, 0.0625])
@pytest.mark.parametrize('S', [64, 16])
def test_window_nll_matches_model(base_cfg, rate, S):
    cfg = make_cfg(base_cfg, LEVELS, data_name='WikiText2',
                   model_name='transformer', num_tokens=130)
    torch.manual_seed(4)
    model = make_model(dict(cfg, global_model_rate=rate), model_rate=rate)
    with torch.no_grad():   # non-trivial biases and LayerNorm affines
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    label = torch.randint(0, 130, (5, S))
    src = label.masked_fill(torch.rand(5, S) < 0.15, 130)
    ref = _model_nll(model, src, label)
    got = NativeLMInference(model).window_nll(src, label)
    assert got.shape == (5, S) and got.dtype == torch.float32
    assert (got - ref).abs().max().item() <= 1e-5
    # the chunked path computes the same thing
    got2 = NativeLMInference(model, chunk=2).window_nll(src, label)
    assert (got2 - ref).abs().max().item() <= 1e-5


def test_native_lm_inference_rejects_other_models(base_cfg):
    cfg = make_cfg(base_cfg, LEVELS)
    with pytest.raises(TypeError):
        NativeLMInference(make_model(cfg))


# ------------------------------------------------------------------- runner
def _lm_runner(base_cfg, mask_rate, seed=0, logger=None):
    cfg = make_cfg(base_cfg, LEVELS, data_name='WikiText2',
                   model_name='transformer')
    cfg['metric_name'] = LM_METRICS
    cfg['mask_rate'] = mask_rate
    torch.manual_seed(seed)
    ds = fetch_dataset('WikiText2', synthetic=True, synthetic_size=20_000)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, cfg['num_users'], 'iid')
    model = make_model(cfg)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg), logger=logger)
    return runner, ds, cfg


def _close(a, b):
    return abs(a - b) <= 1e-5 * max(1.0, abs(b))


def test_native_lm_eval_knob_matches_eager(base_cfg, monkeypatch):
    runner, ds, cfg = _lm_runner(base_cfg, 0.0, logger=Logger(None))
    T = ds['test'][:]['label'].size(1)
    assert T % cfg['bptt'] != 0 and T > cfg['bptt']   # a tail window exists
    monkeypatch.delenv('HETEROFL_NATIVE_LM_EVAL', raising=False)
    runner.test(runner.global_model, 1)
    eager = dict(runner.logger.mean)
    runner.logger.reset()
    monkeypatch.setenv('HETEROFL_NATIVE_LM_EVAL', '1')
    runner.test(runner.global_model, 1)
    native = dict(runner.logger.mean)
    for k in ('test/Global-Loss', 'test/Global-Perplexity'):
        assert k in eager and k in native
        assert _close(native[k], eager[k]), (k, native[k], eager[k])


def _oracle_lm_level(runner, ds, cfg, rate, mask):
    """Eager level model looped over the BatchDataset windows with the
    shared (rows, T) mask."""
    fed = runner.federation
    user = fed.model_rate.index(rate)
    (params,), _ = fed.distribute([user], resample=False)
    model = make_model(dict(cfg, global_model_rate=rate), model_rate=rate)
    model.load_state_dict(params)
    windows = BatchDataset(ds['test'], cfg['bptt'])
    losses, ppls, start = [], [], 0
    for i in range(len(windows)):
        label = windows[i]['label']
        S = label.size(1)
        src = label.masked_fill(mask[:, start:start + S] == 1,
                                cfg['num_tokens'])
        start += S
        loss = _model_nll(model, src, label).double().mean().item()
        losses.append(loss)
        ppls.append(math.exp(loss))
    return {'Global-Loss': sum(losses) / len(losses),
            'Global-Perplexity': sum(ppls) / len(ppls)}


def test_lm_levels_match_oracle(base_cfg, monkeypatch):
    runner, ds, cfg = _lm_runner(base_cfg, 0.15, logger=Logger(None))
    rates = sorted(set(cfg['model_rate']), reverse=True)
    assert rates == [1.0, 0.25, 0.0625]
    torch.manual_seed(21)
    got = runner.test_lm_levels(1)
    assert list(got.keys()) == rates
    assert set(runner.level_models) == set(rates)
    torch.manual_seed(21)
    tokens = ds['test'][:]['label']
    mask = torch.bernoulli(torch.full(tuple(tokens.shape), cfg['mask_rate']))
    assert 0 < mask.sum() < mask.numel()
    for rate in rates:
        ref = _oracle_lm_level(runner, ds, cfg, rate, mask)
        assert set(got[rate]) == {'Global-Loss', 'Global-Perplexity'}
        for k, v in ref.items():
            assert _close(got[rate][k], v), (rate, k, got[rate][k], v)
            key = 'test/{}@{}'.format(k, rate)
            assert _close(runner.logger.mean[key], got[rate][k]), key
    # the global-rate level is what test() logs under the knob, same seed
    rb, _, _ = _lm_runner(base_cfg, 0.15, logger=Logger(None))
    monkeypatch.setenv('HETEROFL_NATIVE_LM_EVAL', '1')
    torch.manual_seed(21)
    rb.test(rb.global_model, 1)
    for k in ('Global-Loss', 'Global-Perplexity'):
        assert _close(rb.logger.mean['test/' + k],
                      got[cfg['global_model_rate']][k]), k


def test_lm_levels_rejects_vision(base_cfg):
    cfg = make_cfg(base_cfg, LEVELS)
    torch.manual_seed(0)
    ds = fetch_dataset('MNIST', synthetic=True, synthetic_size=40)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 4, 'iid', cfg['classes_size'])
    model = make_model(cfg)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    with pytest.raises(NotImplementedError):
        runner.test_lm_levels(1)


# ------------------------------------------------------------- run_fed_eval
def test_run_fed_eval_lm_levels_knob(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('HETEROFL_MAX_ROUNDS', '1')
    monkeypatch.setenv('HETEROFL_SYNTHETIC_SIZE', '20000')
    monkeypatch.delenv('HETEROFL_EVAL_LEVELS', raising=False)
    monkeypatch.delenv('HETEROFL_NATIVE_LM_EVAL', raising=False)
    from heterofl_amd.config import default_config
    from heterofl_amd.entry import run_fed_experiment, run_fed_eval
    from heterofl_amd.utils import load
    cfg = default_config()
    cfg.update({'data_name': 'WikiText2', 'model_name': 'transformer',
                'device': 'cpu', 'engine': 'sequential', 'synthetic': True,
                'num_experiments': 1, 'init_seed': 0, 'resume_mode': 0})
    cfg['control'] = {'fed': '1', 'num_users': '4', 'frac': '0.5',
                      'data_split_mode': 'iid', 'model_split_mode': 'fix',
                      'model_mode': 'a1-c1-e1', 'norm': 'bn', 'scale': '1',
                      'mask': '1'}
    cfg['control_name'] = LEVELS
    run_fed_experiment(dict(cfg), 'Global-Perplexity', -1, LM_METRICS)
    tag = '0_WikiText2_label_transformer_' + LEVELS
    assert os.path.exists('./output/model/{}_best.pt'.format(tag))
    run_fed_eval(dict(cfg), LM_METRICS)
    res = load('./output/result/{}.pt'.format(tag))
    assert 'levels' not in res
    monkeypatch.setenv('HETEROFL_EVAL_LEVELS', '1')
    run_fed_eval(dict(cfg), LM_METRICS)
    res = load('./output/result/{}.pt'.format(tag))
    assert sorted(res['levels']) == [0.0625, 0.25, 1.0]
    for lv in res['levels'].values():
        assert set(lv) == {'Global-Loss', 'Global-Perplexity'}
        assert all(math.isfinite(v) for v in lv.values())
