"""Native inference engine and per-width-level evaluation — CPU side (the
torch paths are the oracle for the GPU kernels in test_gpu_infer.py)."""
import os

import pytest
import torch
import torch.nn.functional as F

from heterofl_amd.data import (fetch_dataset, split_dataset, make_data_loader)
from heterofl_amd.fed import FedRunner
from heterofl_amd.fed.federation import Federation
from heterofl_amd.logger import Logger
from heterofl_amd.metrics import accuracy
from heterofl_amd.models import make_model
from heterofl_amd.models.functional import masked_cross_entropy
from heterofl_amd.ops.fused import eval_metrics
from heterofl_amd.utils import process_dataset, make_optimizer, collate
from tests.conftest import make_cfg

LEVELS = '1_4_0.5_iid_fix_a1-c1-e1_{}_1_1'


# ------------------------------------------------------------ slice_for_rate
@pytest.mark.parametrize('model_name,data_name', [
    ('conv', 'MNIST'), ('resnet18', 'CIFAR10'), ('transformer', 'WikiText2')])
def test_slice_for_rate_matches_distribute(base_cfg, model_name, data_name):
    cfg = make_cfg(base_cfg, LEVELS.format('bn'), data_name=data_name,
                   model_name=model_name)
    torch.manual_seed(0)
    model = make_model(cfg)
    gp = model.state_dict()
    fed = Federation(gp, cfg['model_rate'], {u: list(range(10))
                                             for u in range(4)}, cfg)
    assert len(set(fed.model_rate)) == 3
    before = {k: v.clone() for k, v in gp.items()}
    for u in range(cfg['num_users']):
        rate = fed.model_rate[u]
        (lp,), _ = fed.distribute([u], resample=False)
        sl = fed.slice_for_rate(rate)
        assert list(sl.keys()) == list(lp.keys())
        for k in lp:
            assert sl[k].shape == lp[k].shape, k
            assert torch.equal(sl[k], lp[k]), k
        # fresh storage: no alias of the global parameters
        gptrs = {v.untyped_storage().data_ptr() for v in gp.values()}
        for k, v in sl.items():
            assert v.untyped_storage().data_ptr() not in gptrs, k
            if v.is_floating_point():
                v.add_(1.0)
        for k in gp:
            assert torch.equal(gp[k], before[k]), k


# ------------------------------------------------------------- eval_metrics
def eval_case(device='cpu'):
    """37 samples, 10 classes, 5 users: user 3 is empty, sample 0 belongs to
    users 0 and 1, samples 33..36 to nobody; every label lies inside its
    user's split, so zero-logit ties cannot hit the true class."""
    g = torch.Generator().manual_seed(5)
    N, C, U = 37, 10, 5
    splits = [[0, 1, 2], [2, 3, 4], [5, 6], [7], [8, 9, 0]]
    owners = {0: list(range(0, 9)), 1: [0] + list(range(9, 17)),
              2: list(range(17, 25)), 3: [], 4: list(range(25, 33))}
    labels = torch.zeros(N, dtype=torch.long)
    for u, idx in owners.items():
        for i in idx:
            if i == 0:
                labels[i] = 2          # shared by users 0 and 1
            else:
                ls = splits[u]
                labels[i] = ls[int(torch.randint(0, len(ls), (1,),
                                                 generator=g))]
    labels[33:] = torch.randint(0, C, (4,), generator=g)
    scores = torch.randn(N, C, generator=g) * 3
    ptr, samples = [0], []
    mask = torch.zeros(U, C)
    for u in range(U):
        samples.extend(owners[u])
        ptr.append(len(samples))
        mask[u, splits[u]] = 1
    return {'scores': scores.to(device), 'labels': labels.to(device),
            'ptr': torch.tensor(ptr).to(device),
            'samples': torch.tensor(samples).to(device),
            'mask': mask.to(device), 'splits': splits, 'owners': owners}


def eval_case_reference(case):
    """Per-user loop with masked_cross_entropy and metrics.accuracy (fp64
    sums of the per-user fp32 results)."""
    scores, labels = case['scores'].cpu(), case['labels'].cpu()
    C = scores.size(1)
    local = []
    for u, idx in case['owners'].items():
        if not idx:
            local.append((0.0, 0, 0))
            continue
        idx = torch.tensor(idx)
        sc, loss = masked_cross_entropy(scores[idx], labels[idx],
                                        torch.tensor(case['splits'][u]), C)
        n = idx.numel()
        local.append((loss.item() * n,
                      int(round(accuracy(sc, labels[idx]) * n / 100.0)), n))
    n = scores.size(0)
    glob = (F.cross_entropy(scores, labels).item() * n,
            int(round(accuracy(scores, labels) * n / 100.0)), n)
    return local, glob


def check_eval_case(local, glob, case):
    ref_local, ref_glob = eval_case_reference(case)
    local, glob = local.cpu().tolist(), glob.cpu().tolist()
    for got, ref in zip(local + [glob], ref_local + [ref_glob]):
        assert got[1] == ref[1] and got[2] == ref[2], (got, ref)
        assert abs(got[0] - ref[0]) <= 1e-5 * max(abs(ref[0]), 1e-30), \
            (got, ref)


def test_eval_metrics_fallback_matches_per_user_loop():
    case = eval_case()
    local, glob = eval_metrics(case['scores'], case['labels'], case['ptr'],
                               case['samples'], case['mask'])
    assert local.shape == (5, 3) and glob.shape == (3,)
    check_eval_case(local, glob, case)


# -------------------------------------------------------------- test_levels
def _make_runner(cfg, n_data, seed=0, logger=None):
    torch.manual_seed(seed)
    ds = fetch_dataset(cfg['data_name'], synthetic=True, synthetic_size=n_data)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, cfg['num_users'],
                                            cfg['data_split_mode'],
                                            cfg.get('classes_size'))
    model = make_model(cfg)
    with torch.no_grad():   # non-trivial norm affine parameters
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    opt = make_optimizer(model, cfg['lr'], cfg)
    return FedRunner(cfg, ds, data_split, label_split, model, opt,
                     logger=logger), ds


def _oracle_level(runner, ds, cfg, rate):
    """Eager model at `rate` with Scaler rate 1, the level's slice loaded,
    a train-mode pass over the unshuffled train batches, then an eval-mode
    per-user / global evaluation."""
    fed = runner.federation
    user = fed.model_rate.index(rate)
    (params,), _ = fed.distribute([user], resample=False)
    with torch.no_grad():
        model = make_model(dict(cfg, global_model_rate=rate), model_rate=rate,
                           track=True)
        model.load_state_dict(params, strict=False)
        model.train(True)
        scfg = dict(cfg)
        scfg['shuffle'] = dict(cfg['shuffle'], train=False)
        for batch in make_data_loader({'train': ds['train']}, scfg)['train']:
            model(collate(batch))
        model.train(False)
        test = ds['test']
        x = torch.stack([test[i]['img'] for i in range(len(test))])
        y = torch.tensor(test.target)
        logits = model({'img': x, 'label': y})['score']
        C = cfg['classes_size']
        loss = correct = count = 0.0
        for u in range(cfg['num_users']):
            idx = torch.tensor(runner.data_split['test'][u], dtype=torch.long)
            if idx.numel() == 0:
                continue
            sc, l = masked_cross_entropy(
                logits[idx], y[idx], torch.tensor(runner.label_split[u])
                if cfg['mask'] else None, C)
            loss += l.item() * idx.numel()
            correct += accuracy(sc, y[idx]) * idx.numel() / 100.0
            count += idx.numel()
        return {'Local-Loss': loss / count,
                'Local-Accuracy': 100.0 * correct / count,
                'Global-Loss': F.cross_entropy(logits, y).item(),
                'Global-Accuracy': accuracy(logits, y)}


@pytest.mark.parametrize('norm', ['bn', 'gn'])
@pytest.mark.parametrize('model_name,data_name,n_data', [
    ('conv', 'MNIST', 80), ('resnet18', 'CIFAR10', 60)])
def test_levels_match_oracle(base_cfg, model_name, data_name, n_data, norm):
    cfg = make_cfg(base_cfg, LEVELS.format(norm), data_name=data_name,
                   model_name=model_name)
    runner, ds = _make_runner(cfg, n_data)
    rates = sorted(set(cfg['model_rate']), reverse=True)
    assert len(rates) == 3
    # the CIFAR train transforms draw from the global RNG: both sides start
    # from the same seed and walk the levels in the same order
    torch.manual_seed(123)
    got = runner.test_levels(1)
    assert list(got.keys()) == rates
    torch.manual_seed(123)
    for rate in rates:
        ref = _oracle_level(runner, ds, cfg, rate)
        assert set(got[rate]) == set(ref)
        for k, v in ref.items():
            assert abs(got[rate][k] - v) <= 1e-5 * max(1.0, abs(v)), \
                (rate, k, got[rate][k], v)


@pytest.mark.parametrize('model_name,data_name,n_data', [
    ('conv', 'MNIST', 80), ('resnet18', 'CIFAR10', 60)])
def test_global_level_matches_stats_then_test(base_cfg, model_name,
                                              data_name, n_data):
    cfg = make_cfg(base_cfg, LEVELS.format('bn'), data_name=data_name,
                   model_name=model_name)
    cfg['engine'] = 'batched'
    # two runners from one seed hold identical global models and splits
    ra, _ = _make_runner(cfg, n_data, logger=Logger(None))
    torch.manual_seed(9)
    ra.test(ra.stats(), 1)
    ref = ra.logger.mean
    rb, _ = _make_runner(cfg, n_data, logger=Logger(None))
    torch.manual_seed(9)
    got = rb.test_levels(1)[cfg['global_model_rate']]
    for k in ('Local-Loss', 'Local-Accuracy', 'Global-Loss',
              'Global-Accuracy'):
        v = ref['test/' + k]
        assert abs(got[k] - v) <= 1e-6 * max(1.0, abs(v)), (k, got[k], v)
        # and the level is logged under the '@rate' suffix
        key = 'test/{}@{}'.format(k, cfg['global_model_rate'])
        assert rb.logger.mean[key] == pytest.approx(got[k], rel=1e-12)


def test_levels_rejects_transformer(base_cfg):
    cfg = make_cfg(base_cfg, LEVELS.format('bn'), data_name='WikiText2',
                   model_name='transformer')
    cfg['metric_name'] = {'train': {'Local': ['Local-Loss']},
                          'test': {'Global': ['Global-Loss']}}
    torch.manual_seed(0)
    ds = fetch_dataset('WikiText2', synthetic=True, synthetic_size=20_000)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, cfg['num_users'], 'iid')
    model = make_model(cfg)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    with pytest.raises(NotImplementedError):
        runner.test_levels(1)


# ------------------------------------------------------------- run_fed_eval
def test_run_fed_eval_levels_knob(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('HETEROFL_MAX_ROUNDS', '1')
    monkeypatch.setenv('HETEROFL_SYNTHETIC_SIZE', '40')
    monkeypatch.delenv('HETEROFL_EVAL_LEVELS', raising=False)
    from heterofl_amd.config import default_config
    from heterofl_amd.entry import run_fed_experiment, run_fed_eval
    from heterofl_amd.utils import load
    cfg = default_config()
    cfg.update({'data_name': 'MNIST', 'model_name': 'conv', 'device': 'cpu',
                'engine': 'sequential', 'synthetic': True,
                'num_experiments': 1, 'init_seed': 0, 'resume_mode': 0})
    cfg['control'] = {'fed': '1', 'num_users': '4', 'frac': '0.5',
                      'data_split_mode': 'iid', 'model_split_mode': 'fix',
                      'model_mode': 'a1-c1-e1', 'norm': 'bn', 'scale': '1',
                      'mask': '1'}
    cfg['control_name'] = LEVELS.format('bn')
    metric_name = {'train': {'Local': ['Local-Loss', 'Local-Accuracy']},
                   'test': {'Local': ['Local-Loss', 'Local-Accuracy'],
                            'Global': ['Global-Loss', 'Global-Accuracy']}}
    run_fed_experiment(dict(cfg), 'Global-Accuracy', +1, metric_name)
    tag = '0_MNIST_label_conv_' + LEVELS.format('bn')
    assert os.path.exists('./output/model/{}_best.pt'.format(tag))
    run_fed_eval(dict(cfg), metric_name)
    res = load('./output/result/{}.pt'.format(tag))
    assert 'levels' not in res
    monkeypatch.setenv('HETEROFL_EVAL_LEVELS', '1')
    run_fed_eval(dict(cfg), metric_name)
    res = load('./output/result/{}.pt'.format(tag))
    assert sorted(res['levels']) == [0.0625, 0.25, 1.0]
    for lv in res['levels'].values():
        assert set(lv) == {'Local-Loss', 'Local-Accuracy', 'Global-Loss',
                           'Global-Accuracy'}
