"""Native fill-mask — CPU side: the torch path of lm_head_topk (the oracle of
the kernel in test_gpu_lm_topk.py), NativeLMInference.window_topk /
fill_mask against the model's own logits, and the HETEROFL_LM_TOPK knob of
FedRunner.test_lm_levels / FedRunner.test."""
import pytest
import torch

from heterofl_amd.fed.infer import NativeLMInference
from heterofl_amd.logger import Logger
from heterofl_amd.models import make_model
from heterofl_amd.ops.fused import lm_head_ce, lm_head_pack, lm_head_topk
from tests.conftest import make_cfg
from tests.test_lm_infer import LEVELS, _lm_runner


# ------------------------------------------------------------- lm_head_topk
def _hand_topk(x, w, b, mask, k):
    """Plain loops: fp32 logits, masked columns 0, ordered by (value
    descending, column ascending)."""
    M, E = x.shape
    V = w.shape[0]
    vals, idxs = [], []
    for i in range(M):
        row = []
        for j in range(V):
            z = torch.tensor(0.0)
            for e in range(E):
                z = z + x[i, e] * w[j, e]
            z = z + b[j]
            if mask is not None and mask[j] == 0:
                z = torch.tensor(0.0)
            row.append((-z.item(), j))
        row.sort()
        vals.append([-v for v, _ in row[:k]])
        idxs.append([j for _, j in row[:k]])
    return torch.tensor(vals), torch.tensor(idxs)


@pytest.mark.parametrize('masked', [False, True])
def test_lm_head_topk_torch_path(masked):
    M, E, V = 5, 8, 12
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, E, generator=g)
    w = torch.randn(V, E, generator=g) * 0.3
    b = torch.randn(V, generator=g)
    labels = torch.randint(0, V, (M,), generator=g)
    mask = None
    if masked:
        mask = torch.ones(V)
        mask[torch.tensor([1, 4, 9])] = 0   # three exact ties at 0 per row
    packed = lm_head_pack(w, b)
    for k in (1, 5, 8):
        val, idx, lse, nll = lm_head_topk(x, packed, b, labels, mask, V, E, k)
        ref_v, ref_i = _hand_topk(x, w, b, mask, k)
        assert val.shape == (M, k) and idx.shape == (M, k)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32
        assert torch.equal(idx, ref_i)
        assert (val - ref_v).abs().max().item() <= 1e-5
        logits = x @ w.t() + b
        if masked:
            logits = logits.masked_fill(mask.view(1, V) == 0, 0)
        assert (lse - torch.logsumexp(logits, 1)).abs().max().item() <= 1e-5
        ref_nll = torch.nn.functional.cross_entropy(logits, labels,
                                                    reduction='none')
        assert (nll - ref_nll).abs().max().item() <= 1e-5
        # labels absent: an empty NLL, everything else unchanged
        val2, idx2, lse2, nll2 = lm_head_topk(x, packed, b, None, mask, V, E,
                                              k)
        assert nll2.numel() == 0
        assert torch.equal(val2, val) and torch.equal(idx2, idx) \
            and torch.equal(lse2, lse)
    for bad in (0, 9, V + 1):
        with pytest.raises(ValueError):
            lm_head_topk(x, packed, b, labels, mask, V, E, bad)


@pytest.mark.parametrize('extras', [False, True])
def test_lm_head_ce_and_topk_describe_the_same_logits(extras):
    """The torch paths of the two entry points return equal lse / nll for
    the same inputs (one ragged tile: M = 7, E = 16, V = 33)."""
    M, E, V = 7, 16, 33
    g = torch.Generator().manual_seed(M + E + V)
    x = torch.randn(M, E, generator=g)
    w = torch.randn(V, E, generator=g) * 0.2
    labels = torch.randint(0, V, (M,), generator=g)
    bias = mask = None
    if extras:
        bias = torch.randn(V, generator=g)
        mask = (torch.rand(V, generator=g) < 0.5).float()
        mask[labels[0]] = 0        # a masked label
    packed = lm_head_pack(w, bias)
    nll, lse = lm_head_ce(x, packed, bias, labels, mask, V, E)
    assert nll.shape == (M,) and lse.shape == (M,)
    for k in (1, 5, 8):
        _, _, lse_k, nll_k = lm_head_topk(x, packed, bias, labels, mask, V,
                                          E, k)
        assert torch.equal(lse, lse_k) and torch.equal(nll, nll_k), k


def test_lm_head_topk_k_equals_v():
    """k = V returns the whole vocabulary in order (V <= 8, the largest k),
    k = V + 1 raises."""
    M, E, V = 5, 8, 6
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, E, generator=g)
    w = torch.randn(V, E, generator=g) * 0.3
    b = torch.randn(V, generator=g)
    packed = lm_head_pack(w, b)
    val, idx, _, _ = lm_head_topk(x, packed, b, None, None, V, E, V)
    ref_v, ref_i = _hand_topk(x, w, b, None, V)
    assert torch.equal(idx, ref_i)
    assert torch.equal(idx.sort(1).values, torch.arange(V).expand(M, V))
    assert (val - ref_v).abs().max().item() <= 1e-5
    with pytest.raises(ValueError):
        lm_head_topk(x, packed, b, None, None, V, E, V + 1)


def tie_case():
    """(40, 32, 200) from the generator recipe of _head_case in
    test_gpu_lm_infer.py (seed M+E+V, W scaled by 0.2, bf16-representable),
    no bias, vocab_mask live on columns 5, 70, 199 only: 197 columns per row
    are exactly 0, so the top 8 are decided by the tie rule."""
    M, E, V = 40, 32, 200
    g = torch.Generator().manual_seed(M + E + V)
    x = torch.randn(M, E, generator=g).bfloat16()
    w = (torch.randn(V, E, generator=g) * 0.2).bfloat16().float()
    mask = torch.zeros(V)
    mask[torch.tensor([5, 70, 199])] = 1
    logits = (x.float() @ w.t()).masked_fill(mask.view(1, V) == 0, 0)
    val, idx = torch.sort(logits, dim=1, descending=True, stable=True)
    return {'x': x, 'w': w, 'mask': mask, 'logits': logits,
            'val': val[:, :8], 'idx': idx[:, :8]}


def test_lm_head_topk_tie_rule():
    case = tie_case()
    M, E, V = 40, 32, 200
    # what makes the case decisive: every row's top 8 holds >= 5 exact zeros
    # and the three live logits are far from 0 (no rounding can reorder them)
    assert ((case['val'] == 0).sum(1) >= 5).all()
    live = case['logits'][:, [5, 70, 199]]
    assert live.abs().min().item() > 1e-3
    assert case['idx'][0].tolist() == [70, 5, 0, 1, 2, 3, 4, 6]
    packed = lm_head_pack(case['w'], None)
    val, idx, _, _ = lm_head_topk(case['x'].float(), packed, None, None,
                                  case['mask'], V, E, 8)
    assert torch.equal(idx, case['idx'])
    assert torch.equal(val, case['val'])
    # an independent ordering: python sort by (-value, column)
    for i in range(M):
        order = sorted(range(V), key=lambda j: (-case['logits'][i, j].item(),
                                                j))[:8]
        assert idx[i].tolist() == order


# ---------------------------------------------------- window_topk / fill_mask
def _cpu_transformer(base_cfg, rate, V=130):
    cfg = make_cfg(base_cfg, LEVELS, data_name='WikiText2',
                   model_name='transformer', num_tokens=V)
    torch.manual_seed(4)
    model = make_model(dict(cfg, global_model_rate=rate), model_rate=rate)
    with torch.no_grad():   # non-trivial biases and LayerNorm affines
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return model


def _model_logp(model, src):
    with torch.no_grad():
        model.train(False)
        x = model.transformer_embedding(src)
        for layer in model.transformer_encoder['layers']:
            x = layer(x)
        return torch.log_softmax(model.decoder(x).float(), dim=-1)


@pytest.mark.parametrize('rate', [1.0, 0.0625])
def test_window_topk_and_fill_mask(base_cfg, rate):
    V, N, S, k = 130, 5, 16, 5
    model = _cpu_transformer(base_cfg, rate, V)
    label = torch.randint(0, V, (N, S))
    src = label.masked_fill(torch.rand(N, S) < 0.15, V)
    masked = src == V
    assert 0 < masked.sum() < masked.numel()
    engine = NativeLMInference(model)
    ids, logp, nll = engine.window_topk(src, k=k, label=label)
    assert ids.shape == (N, S, k) and ids.dtype == torch.int64
    assert logp.shape == (N, S, k) and logp.dtype == torch.float32
    assert nll.shape == (N, S) and nll.dtype == torch.float32
    assert torch.equal(nll, engine.window_nll(src, label))
    assert ids.min().item() >= 0 and ids.max().item() < V
    assert (logp[..., 1:] <= logp[..., :-1]).all()
    assert logp.exp().sum(-1).max().item() <= 1.0 + 1e-6
    # against the model's own log-softmax
    ref = _model_logp(model, src)
    assert (logp - ref.gather(-1, ids)).abs().max().item() <= 1e-5
    assert (logp[..., 0] - ref.max(-1).values).abs().max().item() <= 1e-5
    # no label: no NLL, same predictions; chunking changes nothing
    ids2, logp2, none = NativeLMInference(model, chunk=2).window_topk(src,
                                                                      k=k)
    assert none is None and torch.equal(ids2, ids)
    assert (logp2 - logp).abs().max().item() <= 1e-5
    # only_masked: the masked positions of the full run, fillers elsewhere
    ids_m, logp_m, nll_m = engine.window_topk(src, k=k, label=label,
                                              only_masked=True)
    assert (ids_m[~masked] == -1).all()
    assert (logp_m[~masked] == float('-inf')).all()
    assert (nll_m[~masked] == 0).all()
    assert torch.equal(ids_m[masked], ids[masked])
    assert (logp_m[masked] - logp[masked]).abs().max().item() <= 1e-5
    assert (nll_m[masked] - nll[masked]).abs().max().item() <= 1e-5
    # fill_mask: the same predictions as rows, in row-major position order
    pos, f_ids, probs = engine.fill_mask(src, k=k)
    assert torch.equal(pos, masked.nonzero())
    assert f_ids.shape == (pos.size(0), k) and probs.shape == f_ids.shape
    assert torch.equal(f_ids, ids_m[masked])
    assert torch.equal(probs, logp_m[masked].exp())
    assert probs.sum(1).max().item() <= 1.0 + 1e-6
    with pytest.raises(ValueError):
        engine.window_topk(src, k=9)


def test_window_topk_nothing_masked(base_cfg):
    model = _cpu_transformer(base_cfg, 0.0625)
    src = torch.randint(0, 130, (2, 16))
    engine = NativeLMInference(model)
    ids, logp, nll = engine.window_topk(src, k=3, label=src,
                                        only_masked=True)
    assert (ids == -1).all() and (logp == float('-inf')).all()
    assert (nll == 0).all()
    pos, f_ids, probs = engine.fill_mask(src, k=3)
    assert pos.shape == (0, 2) and f_ids.shape == (0, 3) \
        and probs.shape == (0, 3)


# ------------------------------------------------------------------- runner
def fixed_src(tokens, num_tokens, seed=11):
    """tokens with about 15 % of the positions replaced by the <mask> id,
    from a seeded generator of its own (no global RNG draw)."""
    g = torch.Generator().manual_seed(seed)
    hide = torch.rand(tuple(tokens.shape), generator=g) < 0.15
    return tokens.masked_fill(hide.to(tokens.device), num_tokens)


def recount_levels(runner, src, k):
    """{rate: accuracy keys} recounted from window_topk's ids of every
    level model, windows arranged as the runner arranges them (all full
    windows as one batch of sequences, the tail as another)."""
    tokens, windows = runner._stage_lm_eval()
    bptt, V = runner.cfg['bptt'], runner.cfg['num_tokens']
    starts = [s for s, n in windows if n == bptt]
    idx = torch.tensor(starts, device=tokens.device).view(-1, 1) + \
        torch.arange(bptt, device=tokens.device).view(1, -1)
    batches = [(src[:, idx].permute(1, 0, 2).reshape(-1, bptt),
                tokens[:, idx].permute(1, 0, 2).reshape(-1, bptt),
                len(starts))]
    for s, n in windows:
        if n != bptt:
            batches.append((src[:, s:s + n].contiguous(),
                            tokens[:, s:s + n].contiguous(), 1))
    out = {}
    for rate, model in runner.level_models.items():
        engine = NativeLMInference(model)
        per_window = []   # (n, hit1, hitk, mn, mhit1, mhitk)
        for s, y, groups in batches:
            ids, _, _ = engine.window_topk(s, k=k)
            ids, s, y = ids.cpu(), s.cpu(), y.cpu()
            hit1 = (ids[..., 0] == y).view(groups, -1)
            hitk = (ids == y.unsqueeze(-1)).any(-1).view(groups, -1)
            m = (s == V).view(groups, -1)
            for w in range(groups):
                per_window.append((
                    hit1[w].numel(), int(hit1[w].sum()), int(hitk[w].sum()),
                    int(m[w].sum()), int((hit1[w] & m[w]).sum()),
                    int((hitk[w] & m[w]).sum())))
        nw = len(per_window)
        res = {'Global-Accuracy':
               sum(100.0 * c[1] / c[0] for c in per_window) / nw,
               'Global-Accuracy-Top{}'.format(k):
               sum(100.0 * c[2] / c[0] for c in per_window) / nw}
        mn = sum(c[3] for c in per_window)
        if mn:
            res['Global-Masked-Accuracy'] = \
                100.0 * sum(c[4] for c in per_window) / mn
            res['Global-Masked-Accuracy-Top{}'.format(k)] = \
                100.0 * sum(c[5] for c in per_window) / mn
        out[rate] = res
    return out


BASE_KEYS = {'Global-Loss', 'Global-Perplexity'}
ACC_KEYS = {'Global-Accuracy', 'Global-Accuracy-Top5'}
MASKED_KEYS = {'Global-Masked-Accuracy', 'Global-Masked-Accuracy-Top5'}


def test_lm_levels_topk_knob(base_cfg, monkeypatch):
    runner, ds, cfg = _lm_runner(base_cfg, 0.15, logger=Logger(None))
    tokens, windows = runner._stage_lm_eval()
    src = fixed_src(tokens, cfg['num_tokens'])
    assert (src == cfg['num_tokens']).any()
    monkeypatch.setattr(runner, '_lm_masked_src', lambda t: src)
    monkeypatch.setenv('HETEROFL_LM_TOPK', '5')
    got = runner.test_lm_levels(1)
    ref = recount_levels(runner, src, 5)
    assert sorted(got) == [0.0625, 0.25, 1.0]
    for rate, lv in got.items():
        assert set(lv) == BASE_KEYS | ACC_KEYS | MASKED_KEYS
        for name in ACC_KEYS | MASKED_KEYS:
            assert lv[name] == ref[rate][name], (rate, name)
            assert 0.0 <= lv[name] <= 100.0
            logged = runner.logger.mean['test/{}@{}'.format(name, rate)]
            assert abs(logged - lv[name]) <= 1e-9 * max(1.0, lv[name])
        assert lv['Global-Accuracy'] <= lv['Global-Accuracy-Top5']


def test_lm_levels_topk_no_masked_positions(base_cfg, monkeypatch):
    runner, ds, cfg = _lm_runner(base_cfg, 0.0, logger=Logger(None))
    monkeypatch.setenv('HETEROFL_LM_TOPK', '1')   # and no Top-k keys at 1
    got = runner.test_lm_levels(1)
    for rate, lv in got.items():
        assert set(lv) == BASE_KEYS | {'Global-Accuracy'}
    assert not any('Masked' in k or 'Top' in k for k in runner.logger.mean)


def test_lm_topk_knob_off_and_rng(base_cfg, monkeypatch):
    """Knob off: exactly the two keys; the knob does not change what is
    drawn from the global torch RNG, nor the loss (same mask, the NLL of the
    same logits from the other head op)."""
    states, res = {}, {}
    for knob in (None, '5'):
        runner, ds, cfg = _lm_runner(base_cfg, 0.15, logger=Logger(None))
        if knob is None:
            monkeypatch.delenv('HETEROFL_LM_TOPK', raising=False)
        else:
            monkeypatch.setenv('HETEROFL_LM_TOPK', knob)
        torch.manual_seed(21)
        got = runner.test_lm_levels(1)
        states[knob] = torch.get_rng_state()
        res[knob] = got
        for lv in got.values():
            assert set(lv) == (BASE_KEYS if knob is None
                               else BASE_KEYS | ACC_KEYS | MASKED_KEYS)
    assert torch.equal(states[None], states['5'])
    for rate, lv in res[None].items():
        for name in BASE_KEYS:
            assert abs(res['5'][rate][name] - lv[name]) \
                <= 1e-5 * max(1.0, abs(lv[name])), (rate, name)
    monkeypatch.setenv('HETEROFL_LM_TOPK', '0')
    assert all(set(lv) == BASE_KEYS
               for lv in runner.test_lm_levels(1).values())


@pytest.mark.parametrize('bad', ['9', '-1', 'five', '2.5'])
def test_lm_topk_knob_rejects_bad_values(base_cfg, monkeypatch, bad):
    runner, ds, cfg = _lm_runner(base_cfg, 0.0)
    monkeypatch.setenv('HETEROFL_LM_TOPK', bad)
    with pytest.raises(ValueError):
        runner.test_lm_levels(1)


def test_native_lm_test_logs_accuracy(base_cfg, monkeypatch):
    """FedRunner.test under HETEROFL_NATIVE_LM_EVAL=1 logs the global-rate
    level's accuracies without the @rate suffix."""
    runner, ds, cfg = _lm_runner(base_cfg, 0.15, logger=Logger(None))
    tokens, _ = runner._stage_lm_eval()
    src = fixed_src(tokens, cfg['num_tokens'])
    monkeypatch.setattr(runner, '_lm_masked_src', lambda t: src)
    monkeypatch.setenv('HETEROFL_LM_TOPK', '5')
    levels = runner.test_lm_levels(1)
    runner.logger.reset()
    monkeypatch.setenv('HETEROFL_NATIVE_LM_EVAL', '1')
    runner.test(runner.global_model, 1)
    mean = dict(runner.logger.mean)
    top = levels[cfg['global_model_rate']]
    for name in BASE_KEYS | ACC_KEYS | MASKED_KEYS:
        assert abs(mean['test/' + name] - top[name]) \
            <= 1e-5 * max(1.0, abs(top[name])), name
    monkeypatch.delenv('HETEROFL_LM_TOPK')
    runner.logger.reset()
    runner.test(runner.global_model, 1)
    assert set(runner.logger.mean) == {'test/' + k for k in BASE_KEYS}
