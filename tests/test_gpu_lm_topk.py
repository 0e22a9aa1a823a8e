"""GPU tests of the fused top-k LM head kernel, NativeLMInference.window_topk
and the HETEROFL_LM_TOPK knob (MI355X).  Run with: pytest tests -m gpu"""
import pytest
import torch

from heterofl_amd.ops import require_native
from heterofl_amd.ops.fused import lm_head_pack, lm_head_topk
from tests.conftest import make_cfg
from tests.test_gpu_lm_infer import (HEAD_CASES, _autocast_error, _head_case,
                                     _run_head)
from tests.test_lm_topk import (ACC_KEYS, BASE_KEYS, MASKED_KEYS, fixed_src,
                                recount_levels, tie_case)

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')
DEV = 'cuda:0'
_ref_cache = {}


def _ref_case(shape, extras):
    """_head_case plus the fp32 host logits and their stable descending
    sort (first 9 ranks), computed once per case and shared."""
    key = (shape, extras)
    if key not in _ref_cache:
        case = dict(_head_case(shape, extras))
        logits = case['x'].float() @ case['w'].t()
        if extras:
            logits = (logits + case['bias']).masked_fill(
                case['mask'].view(1, -1) == 0, 0)
        val, idx = torch.sort(logits, dim=1, descending=True, stable=True)
        case.update(logits=logits, sval=val[:, :9].contiguous(),
                    sidx=idx[:, :9].contiguous())
        _ref_cache[key] = case
    return _ref_cache[key]


def _check_topk(val, idx, logits, sval, sidx, delta, mask, k, tag):
    """Assertions (a) - (e) of a (M, k) prediction against fp32 host logits
    whose per-row error scale is delta:
    (a) |val - sorted reference| <= delta (order statistics move by at most
        the sup-norm perturbation);
    (b) the reference logit at every returned column is within delta of the
        returned value, columns distinct and inside [0, V);
    (c) val non-increasing, bit-equal neighbours in ascending column order;
    (d) on separated rows (every adjacent pair of the reference top-(k+1)
        is more than 2 delta apart or both columns vocab-masked) the columns
        equal the reference exactly;
    (e) at least 85 % of the rows are separated."""
    M, V = logits.shape
    val, idx = val.cpu(), idx.cpu()
    assert val.shape == (M, k) and idx.shape == (M, k)
    assert val.dtype == torch.float32 and idx.dtype == torch.int64
    d = delta.view(-1, 1)
    e_a = ((val - sval[:, :k]).abs() - d).max().item()
    assert idx.min().item() >= 0 and idx.max().item() < V
    e_b = ((logits.gather(1, idx) - val).abs() - d).max().item()
    assert (idx.sort(1).values.diff(dim=1) > 0).all()
    assert (val.diff(dim=1) <= 0).all()
    same = val[:, 1:] == val[:, :-1]
    assert (idx.diff(dim=1)[same] > 0).all()
    gap = sval[:, :k] - sval[:, 1:k + 1]
    ok = gap > 2 * d
    if mask is not None:
        dead = mask[sidx] == 0
        ok |= dead[:, :k] & dead[:, 1:k + 1]
    sep = ok.all(1)
    print('lm_head_topk', tag, 'k', k, 'worst (a) err - delta', e_a,
          'worst (b) err - delta', e_b, 'separated rows', int(sep.sum()),
          'of', M)
    assert e_a <= 0 and e_b <= 0
    assert torch.equal(idx[sep], sidx[:, :k][sep])
    assert sep.sum().item() >= 0.85 * M


def _topk_args(case, shape):
    M, E, V = shape

    def dev(t):
        return None if t is None else t.to(DEV)

    packed = lm_head_pack(case['w'].to(DEV), dev(case['bias']))
    return (case['x'].to(DEV), packed, dev(case['bias']),
            dev(case['labels']), dev(case['mask']), V, E)


@needs_gpu
@pytest.mark.parametrize('k', [1, 5, 8])
@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('splits', [1, 3, 0])
@pytest.mark.parametrize('shape', HEAD_CASES)
def test_lm_head_topk_matches_host(shape, splits, extras, k):
    """(a) - (e) of _check_topk; (f) row_lse / row_nll within the bounds of
    test_lm_head_ce_matches_host; (g) a second launch is bit-equal."""
    M, E, V = shape
    case = _ref_case(shape, extras)
    args = _topk_args(case, shape)
    val, idx, lse, nll = lm_head_topk(*args, k, splits=splits)
    torch.cuda.synchronize()
    _check_topk(val, idx, case['logits'], case['sval'], case['sidx'],
                case['delta'], case['mask'], k,
                (shape, 'splits', splits, 'extras', extras))
    assert nll.shape == (M,) and lse.shape == (M,)
    assert nll.dtype == torch.float32 and lse.dtype == torch.float32
    tail = V * 2.0 ** -24 + 1e-5
    e_nll = (nll.cpu() - case['nll']).abs() - (2 * case['delta'] + tail)
    e_lse = (lse.cpu() - case['lse']).abs() - (case['delta'] + tail)
    print('worst nll err - bound', e_nll.max().item(),
          'worst lse err - bound', e_lse.max().item())
    assert e_nll.max().item() <= 0 and e_lse.max().item() <= 0
    again = lm_head_topk(*args, k, splits=splits)
    for a, b in zip((val, idx, lse, nll), again):
        assert torch.equal(a, b)


@needs_gpu
@pytest.mark.parametrize('splits', [1, 3])
def test_lm_head_topk_tie_rule_gpu(splits):
    """197 of 200 columns are exactly 0: the columns must equal the stable
    sort's, the zeros bit for bit."""
    case = tie_case()
    M, E, V = 40, 32, 200
    packed = lm_head_pack(case['w'].to(DEV), None)
    val, idx, _, nll = lm_head_topk(case['x'].to(DEV), packed, None, None,
                                    case['mask'].to(DEV), V, E, 8,
                                    splits=splits)
    assert nll.numel() == 0
    assert torch.equal(idx.cpu(), case['idx'])
    zero = case['val'] == 0
    assert (val.cpu()[zero] == 0).all()
    A = case['x'].float().abs() @ case['w'].abs().t()
    delta = 33 * 2.0 ** -23 * A.max(dim=1).values
    assert ((val.cpu() - case['val']).abs() - delta.view(-1, 1)).max() <= 0


@needs_gpu
@pytest.mark.parametrize('shape', HEAD_CASES[:2])
def test_lm_head_topk_without_labels(shape):
    M, E, V = shape
    args = list(_topk_args(_ref_case(shape, True), shape))
    val, idx, lse, nll = lm_head_topk(*args, 5, splits=3)
    args[3] = None
    val2, idx2, lse2, nll2 = lm_head_topk(*args, 5, splits=3)
    assert nll.shape == (M,) and nll2.numel() == 0
    assert torch.equal(val, val2) and torch.equal(idx, idx2) \
        and torch.equal(lse, lse2)


@needs_gpu
def test_lm_head_topk_rejects_bad_k():
    shape = HEAD_CASES[0]
    args = _topk_args(_ref_case(shape, False), shape)
    ext = require_native()
    none = torch.Tensor()
    for bad in (0, 9, 34):
        with pytest.raises(ValueError):
            lm_head_topk(*args, bad)
        with pytest.raises(RuntimeError):   # the binding's own TORCH_CHECK
            ext.lm_head_topk(args[0], args[1], none, none, none, args[5],
                             args[6], bad, 0)


@needs_gpu
@pytest.mark.parametrize('extras', [False, True])
@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('shape', HEAD_CASES)
def test_lm_head_ce_unchanged_next_to_topk(shape, splits, extras):
    """lm_head_ce is the top-k kernel instantiated without lists: it still
    meets its host reference, and on the first three shapes its (row_nll,
    row_lse) at the same explicit `splits` are bit-equal to lm_head_topk's
    for k = 1 and k = 5."""
    M, E, V = shape
    case = _head_case(shape, extras)
    args, (nll, lse) = _run_head(case, shape, splits)
    tail = V * 2.0 ** -24 + 1e-5
    e_nll = (nll.cpu() - case['nll']).abs() - (2 * case['delta'] + tail)
    e_lse = (lse.cpu() - case['lse']).abs() - (case['delta'] + tail)
    assert e_nll.max().item() <= 0 and e_lse.max().item() <= 0
    if shape in HEAD_CASES[:3]:
        for k in (1, 5):
            _, _, lse_k, nll_k = lm_head_topk(*args, k, splits=splits)
            assert torch.equal(nll, nll_k) and torch.equal(lse, lse_k), k


# -------------------------------------------------------- NativeLMInference
@needs_gpu
@pytest.mark.parametrize('rate', [1.0, 0.0625])
def test_window_topk_bf16(base_cfg, rate):
    """window_topk(k=5) on the model of test_native_lm_inference_bf16, per
    window (7 of 64 and a tail of 25): against fp32 host logits built from
    the engine's own bf16 hidden rows and the bf16-rounded head weight,
    (a) - (e) hold for the head's values and columns, window_topk returns
    those columns and logp == value - lse within delta_i + V 2^-24 + 1e-5,
    and only_masked agrees bit for bit on the masked positions."""
    from heterofl_amd.fed.infer import NativeLMInference
    from heterofl_amd.models import make_model
    V, k = 1000, 5
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
    engine = NativeLMInference(model)
    lin2 = model.decoder.linear2
    w = lin2.weight.detach().bfloat16().float().cpu()
    b = lin2.bias.detach().float().cpu()
    E = w.size(1)
    Ep = -(-E // 32) * 32
    tail = V * 2.0 ** -24 + 1e-5
    for s0 in range(0, T, 64):
        s = src[:, s0:s0 + 64].contiguous()
        y = label[:, s0:s0 + 64].contiguous()
        with torch.no_grad():
            h = engine._hidden(s)
        M = h.size(0)
        hf = h.float().cpu()
        logits = hf @ w.t() + b
        delta = (Ep + 1) * 2.0 ** -23 * (hf.abs() @ w.abs().t()
                                         + b.abs()).max(dim=1).values
        sval, sidx = torch.sort(logits, dim=1, descending=True, stable=True)
        splits = engine.ext.lm_head_topk_splits(M, V)
        val, idx, lse, _ = lm_head_topk(h, engine.packed, engine.head_b,
                                        None, None, V, E, k, splits=splits)
        _check_topk(val, idx, logits, sval[:, :9], sidx[:, :9], delta, None,
                    k, ('rate', rate, 'window', s0))
        ids, logp, nll = engine.window_topk(s, k=k, label=y)
        assert ids.shape == (10, s.size(1), k) and nll.shape == s.shape
        assert torch.equal(ids.view(M, k), idx)
        e_lp = (logp.view(M, k) - (val - lse.view(-1, 1))).abs().cpu() \
            - (delta + tail).view(-1, 1)
        ref_lp = sval[:, :k] - torch.logsumexp(logits, 1).view(-1, 1)
        e_ref = (logp.view(M, k).cpu() - ref_lp).abs() \
            - (2 * delta + tail).view(-1, 1)
        assert e_lp.max().item() <= 0 and e_ref.max().item() <= 0
        ref_nll = torch.logsumexp(logits, 1) - logits.gather(
            1, y.reshape(-1, 1).cpu()).squeeze(1)
        e_nll = (nll.view(M).cpu() - ref_nll).abs() - (2 * delta + tail)
        assert e_nll.max().item() <= 0
        ids_m, logp_m, nll_m = engine.window_topk(s, k=k, label=y,
                                                  only_masked=True)
        masked = s == V
        assert masked.any() and not masked.all()
        assert torch.equal(ids_m[masked], ids[masked])
        assert torch.equal(logp_m[masked], logp[masked])
        assert torch.equal(nll_m[masked], nll[masked])
        assert (ids_m[~masked] == -1).all() and (nll_m[~masked] == 0).all()
        assert (logp_m[~masked] == float('-inf')).all()
    pos, f_ids, probs = engine.fill_mask(src[:, :64].contiguous(), k=k)
    assert torch.equal(pos, (src[:, :64] == V).nonzero())
    assert f_ids.shape == (pos.size(0), k)
    assert probs.sum(1).max().item() <= 1.0 + 1e-5


@needs_gpu
def test_lm_levels_topk_gpu(base_cfg, monkeypatch):
    """HETEROFL_LM_TOPK=5 on the batched engine with an injected src: the
    four accuracy keys per level equal an integer recount on the host from
    that level's window_topk ids, and each level's loss is within
    2 e_autocast(level) of the knob-off loss on the same src."""
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.models import make_model
    from heterofl_amd.utils import process_dataset, make_optimizer
    from tests.test_lm_infer import LM_METRICS
    cfg = make_cfg(base_cfg, '1_4_0.5_iid_fix_a1-c1-e1_bn_1_1',
                   data_name='WikiText2', model_name='transformer')
    cfg['metric_name'] = LM_METRICS
    cfg['mask_rate'] = 0.15
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
    tokens, windows = runner._stage_lm_eval()
    src = fixed_src(tokens, cfg['num_tokens'])
    monkeypatch.setattr(runner, '_lm_masked_src', lambda t: src)
    monkeypatch.delenv('HETEROFL_LM_TOPK', raising=False)
    off = runner.test_lm_levels(1)
    monkeypatch.setenv('HETEROFL_LM_TOPK', '5')
    got = runner.test_lm_levels(1)
    ref = recount_levels(runner, src, 5)
    assert sorted(got) == [0.0625, 0.25, 1.0]
    for rate, lv in got.items():
        assert set(off[rate]) == BASE_KEYS
        assert set(lv) == BASE_KEYS | ACC_KEYS | MASKED_KEYS
        for name in sorted(ACC_KEYS | MASKED_KEYS):
            assert lv[name] == ref[rate][name], (rate, name, lv[name],
                                                 ref[rate][name])
        _, e_autocast = _autocast_error(runner.level_models[rate], src,
                                        tokens, windows)
        err = abs(lv['Global-Loss'] - off[rate]['Global-Loss'])
        print('LM level', rate, {n: lv[n] for n in sorted(lv)},
              'knob-off loss', off[rate]['Global-Loss'], 'err', err,
              'e_autocast', e_autocast)
        assert err <= 2.0 * e_autocast, (rate, err, e_autocast)
