"""GPU tests of rolling sub-model extraction (MI355X): the rolled pack
kernel (pack_slices_roll) and the combine accumulate kernel
(combine_accumulate) against the torch paths of Federation.  Everything is
compared bit for bit: a pack is a copy, and the accumulate kernel performs
the torch loop's fp32 additions in the torch loop's order.
Run with: pytest tests -m gpu"""
import pytest
import torch

from heterofl_amd.fed import Federation
from heterofl_amd.models import make_model
from tests.conftest import make_cfg

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')
DEV = 'cuda:0'
CONTROL = '1_4_1_iid_fix_a1-e1_bn_1_1'
MODELS = [('resnet18', 'CIFAR10', {}),
          ('transformer', 'WikiText2', {'num_tokens': 300})]
IDS = [m[0] for m in MODELS]
ROUNDS = [2, 63, 64, 500]
USERS = [0, 1, 2, 3]


def _fed(base_cfg, model_name, data_name, kw, submodel='roll'):
    cfg = make_cfg(base_cfg, CONTROL, data_name=data_name,
                   model_name=model_name, **kw)
    cfg['device'] = DEV
    cfg['submodel'] = submodel
    cfg['roll_step'] = 1
    g = torch.Generator().manual_seed(5)
    if model_name == 'transformer':
        label_split = {u: sorted(torch.randperm(300, generator=g)[:150]
                                 .tolist()) for u in range(4)}
    else:
        label_split = {u: sorted(torch.randperm(10, generator=g)[:2]
                                 .tolist()) for u in range(4)}
    torch.manual_seed(0)
    model = make_model(cfg, model_rate=1).to(DEV)
    return Federation(model.state_dict(), cfg['model_rate'], label_split,
                      cfg)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------- 1. pack
@needs_gpu
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_pack_matches_eager(base_cfg, monkeypatch, model_name,
                                 data_name, kw):
    fed = _fed(base_cfg, model_name, data_name, kw)
    for rnd in ROUNDS:
        monkeypatch.delenv('HETEROFL_FORCE_EAGER', raising=False)
        fed.last_pack_per_tensor = None
        native, pidx = fed.distribute(USERS, resample=False, round=rnd)
        assert fed.last_pack_route == 'roll'
        # every weight and bias, q/k/v included, came from the kernel
        per_tensor = fed.last_pack_per_tensor
        assert not any('linear_q' in k or 'linear_k' in k or 'linear_v' in k
                       for _, k in per_tensor)
        assert per_tensor == []
        monkeypatch.setenv('HETEROFL_FORCE_EAGER', '1')
        eager, pidx2 = fed.distribute(USERS, resample=False, round=rnd)
        assert fed.last_pack_route == 'torch'
        assert fed.last_pack_per_tensor is None
        for m in USERS:
            assert list(native[m].keys()) == list(eager[m].keys())
            for k in eager[m]:
                assert native[m][k].shape == eager[m][k].shape, (k, m, rnd)
                assert torch.equal(native[m][k], eager[m][k]), (k, m, rnd)


# ----------------------------------------------------------- 2. accumulate
@needs_gpu
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_accumulate_matches_torch(base_cfg, monkeypatch, model_name,
                                       data_name, kw):
    fed = _fed(base_cfg, model_name, data_name, kw)
    gp = fed.global_parameters
    start = {k: v.clone() for k, v in gp.items()}
    g = torch.Generator().manual_seed(11)
    for rnd in ROUNDS:
        monkeypatch.delenv('HETEROFL_NATIVE_COMBINE', raising=False)
        local, pidx = fed.distribute(USERS, resample=False, round=rnd)
        trained = {m: {k: v + torch.randn(v.shape, generator=g).to(DEV)
                       for k, v in local[m].items()} for m in (0, 1, 3)}
        tmp_n, cnt_n = fed.accumulate(trained, pidx, USERS, slots=[0, 1, 3])
        assert fed.last_combine_route == 'kernel'
        # every fp32 key, q/k/v included, came from the kernel
        assert fed.last_combine_keys == [k for k, v in gp.items()
                                         if v.dtype == torch.float32]
        assert fed.last_combine_keys == list(gp.keys())
        monkeypatch.setenv('HETEROFL_NATIVE_COMBINE', '0')
        tmp_t, cnt_t = fed.accumulate(trained, pidx, USERS, slots=[0, 1, 3])
        assert fed.last_combine_route == 'torch'
        assert fed.last_combine_keys == []
        assert list(tmp_n.keys()) == list(tmp_t.keys()) == list(gp.keys())
        for k in gp:
            assert tmp_n[k].shape == tmp_t[k].shape == gp[k].shape, k
            assert torch.equal(cnt_n[k], cnt_t[k]), (k, rnd)
            assert torch.equal(_bits(tmp_n[k]), _bits(tmp_t[k])), (k, rnd)
        fed.finalize(tmp_n, cnt_n)
        after_n = {k: v.clone() for k, v in gp.items()}
        for k, v in gp.items():
            v.copy_(start[k])
        fed.finalize(tmp_t, cnt_t)
        for k, v in gp.items():
            assert torch.equal(v, after_n[k]), (k, rnd)
            v.copy_(start[k])


# -------------------------------------------------------- 3. static opt-in
@needs_gpu
def test_static_native_combine_opt_in(base_cfg, monkeypatch):
    fed = _fed(base_cfg, 'resnet18', 'CIFAR10', {}, submodel='static')
    monkeypatch.delenv('HETEROFL_NATIVE_COMBINE', raising=False)
    local, pidx = fed.distribute(USERS, resample=False)
    assert fed.last_pack_route == 'static'
    g = torch.Generator().manual_seed(3)
    trained = {m: {k: v + torch.randn(v.shape, generator=g).to(DEV)
                   for k, v in local[m].items()} for m in USERS}
    tmp_t, cnt_t = fed.accumulate(trained, pidx, USERS)
    assert fed.last_combine_route == 'torch'   # the default is unchanged
    monkeypatch.setenv('HETEROFL_NATIVE_COMBINE', '1')
    tmp_n, cnt_n = fed.accumulate(trained, pidx, USERS)
    assert fed.last_combine_route == 'kernel'
    assert fed.last_combine_keys == list(fed.global_parameters.keys())
    for k in tmp_t:
        assert torch.equal(cnt_n[k], cnt_t[k]), k
        assert torch.equal(_bits(tmp_n[k]), _bits(tmp_t[k])), k


# ------------------------------------------------------ 4. smallest shapes
def _window_indices(win, n):
    period, shift, take = win
    return torch.tensor([(j // take) * period + (shift + j % take) % period
                         for j in range(n)], dtype=torch.long)


def _oracle(shape, clients):
    """tmp/cnt of one tensor from the clients' explicit index lists, one
    client at a time in list order (CPU, fp32)."""
    tmp = torch.zeros(shape)
    cnt = torch.zeros(shape)
    O = shape[0]
    I = shape[1] if len(shape) > 1 else 1
    for val, ow, iw, mask in clients:
        n_out = (O // ow[0]) * ow[2]
        oidx = _window_indices(ow, n_out)
        val = val.cpu()
        if mask is not None:
            keep = torch.tensor(mask, dtype=torch.bool)
            oidx, val = oidx[keep], val[keep]
        if len(shape) > 1:
            iw = iw if iw is not None else (I, 0, I)
            iidx = _window_indices(iw, (I // iw[0]) * iw[2])
            tmp[oidx.unsqueeze(1), iidx.unsqueeze(0)] += val
            cnt[oidx.unsqueeze(1), iidx.unsqueeze(0)] += 1
        else:
            tmp[oidx] += val
            cnt[oidx] += 1
    return tmp, cnt


@needs_gpu
def test_combine_kernel_smallest_shapes():
    from heterofl_amd.ops.fused import combine_accumulate
    g = torch.Generator().manual_seed(7)

    def val(*shape):
        return torch.randn(*shape, generator=g).to(DEV)

    cases = [
        # inner 9: shift = period - 1 (rows 5, 0, 1; cols 3, 0), a per-head
        # window of take 1 (rows 1, 3, 5), and take 1 over period 1 columns
        ((6, 4, 3, 3), [
            (val(3, 2, 3, 3), (6, 5, 3), (4, 3, 2), None),
            (val(3, 4, 3, 3), (2, 1, 1), (4, 0, 4), None),
            (val(1, 4, 3, 3), (6, 2, 1), (1, 0, 1), None)]),
        # inner 1 with row masks: one all-zero, one partial
        ((5, 7), [
            (val(5, 3), (5, 0, 5), (7, 6, 3), [0, 0, 0, 0, 0]),
            (val(5, 7), (5, 0, 5), (7, 0, 7), [1, 0, 0, 1, 1]),
            (val(2, 7), (5, 4, 2), None, None)]),
        # 1-D: a wrapping window, a masked full axis, period 1
        ((5,), [
            (val(2), (5, 4, 2), None, None),
            (val(5), (5, 0, 5), None, [0, 1, 0, 0, 1]),
            (val(5), (1, 0, 1), None, None)]),
        # nobody reported
        ((3, 2), []),
        # only an all-zero row mask: cnt 0 and tmp 0 everywhere
        ((8,), [(val(8), (8, 0, 8), None, [0] * 8)]),
        # more than one block of 1024 elements, ragged tail
        ((40, 30, 3, 3), [
            (val(20, 15, 3, 3), (40, 39, 20), (30, 29, 15), None),
            (val(40, 30, 3, 3), (40, 0, 40), (30, 0, 30), None),
            (val(10, 6, 3, 3), (8, 7, 2), (5, 3, 1), None)]),
    ]
    shapes = [c[0] for c in cases]
    clients = [c[1] for c in cases]
    tmps, cnts = combine_accumulate(shapes, clients, torch.device(DEV))
    torch.cuda.synchronize()
    for (shape, ents), tmp, cnt in zip(cases, tmps, cnts):
        ref_t, ref_c = _oracle(shape, ents)
        assert tuple(tmp.shape) == shape and tuple(cnt.shape) == shape
        assert torch.equal(cnt.cpu(), ref_c), shape
        assert torch.equal(_bits(tmp.cpu()), _bits(ref_t)), shape
    assert not tmps[3].any() and not cnts[3].any()
    assert not tmps[4].any() and not cnts[4].any()
    # a slice that does not match its windows is refused before the launch
    with pytest.raises(ValueError):
        combine_accumulate([(6, 4)], [[(val(3, 3), (6, 5, 3), (4, 3, 2),
                                        None)]], torch.device(DEV))


# ------------------------------------------------------ 5. a batched round
@needs_gpu
def test_batched_round_under_roll(base_cfg, monkeypatch):
    """resnet18, batched engine, a wrapping round: the new global
    parameters equal the torch combine of the same trained client states."""
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.fed import FedRunner
    from heterofl_amd.utils import process_dataset, make_optimizer
    monkeypatch.delenv('HETEROFL_NATIVE_COMBINE', raising=False)
    monkeypatch.delenv('HETEROFL_FORCE_EAGER', raising=False)
    cfg = make_cfg(base_cfg, CONTROL, data_name='CIFAR10',
                   model_name='resnet18')
    cfg['device'] = DEV
    cfg['engine'] = 'batched'
    cfg['compute_dtype'] = 'bfloat16'
    cfg['submodel'] = 'roll'
    cfg['num_epochs'] = {'global': 1, 'local': 1}
    torch.manual_seed(0)
    ds = fetch_dataset('CIFAR10', synthetic=True, synthetic_size=80)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, 4, 'iid',
                                            cfg['classes_size'])
    model = make_model(cfg).to(DEV)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    fed = runner.federation
    before = {k: v.clone() for k, v in fed.global_parameters.items()}
    seen = {}
    distribute, train_clients = fed.distribute, runner.trainer.train_clients

    def rec_distribute(*a, **kw):
        out = distribute(*a, **kw)
        seen['pidx'] = out[1]
        return out

    def rec_train(*a, **kw):
        out = [(m, {k: v.clone() for k, v in sd.items()})
               for m, sd in train_clients(*a, **kw)]
        seen['states'] = dict(out)
        return out

    fed.distribute = rec_distribute
    runner.trainer.train_clients = rec_train
    user_idx = runner.train_round(63)
    torch.cuda.synchronize()
    assert fed.last_pack_route == 'roll'
    assert fed.last_combine_route == 'kernel'
    from heterofl_amd.fed.federation import ROLL
    assert any(ps.out.kind == ROLL for pi in seen['pidx']
               for ps in pi.values())
    start = {k: v.clone() for k, v in before.items()}
    oracle = Federation(before, cfg['model_rate'], label_split, cfg)
    oracle.model_rate = list(fed.model_rate)
    monkeypatch.setenv('HETEROFL_NATIVE_COMBINE', '0')
    tmp_d, cnt_d = oracle.accumulate(seen['states'], seen['pidx'], user_idx,
                                     slots=sorted(seen['states']))
    assert oracle.last_combine_route == 'torch'
    oracle.finalize(tmp_d, cnt_d)
    # `before` now holds the oracle's result (finalize writes in place)
    assert oracle.global_parameters is before
    assert any(not torch.equal(before[k], start[k]) for k in start)
    for k, v in fed.global_parameters.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, before[k]), k
