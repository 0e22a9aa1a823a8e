"""Rolling sub-model extraction (cfg['submodel'] = 'roll') on the CPU paths:
index maps, slices, the distribute -> combine round trip, the coverage the
mode exists for, linearity of accumulate, and three federated rounds.

The expected indices are built here from the rule "the window of a W-wide
axis at round R starts at ((R - 1) * roll_step) % W", independently of
Axis.indices(): torch.roll(torch.arange(W), -s)[:n], per head for q/k/v.
"""
import math

import pytest
import torch

from heterofl_amd.fed import Federation, FedRunner, Axis
from heterofl_amd.fed.federation import FULL, PREFIX, GATHER, ROLL
from heterofl_amd.models import make_model
from tests.conftest import make_cfg

CONTROL = '1_4_1_iid_fix_a1-e1_bn_1_1'
MODELS = [('conv', 'MNIST', {}), ('resnet18', 'CIFAR10', {}),
          ('transformer', 'WikiText2', {'num_tokens': 300})]
IDS = [m[0] for m in MODELS]
LEVELS = [1.0, 0.5, 0.25, 0.125, 0.0625]   # a..e
# shift 0 / no wrap / wraps on the 64-wide axis / wraps on the 512-wide axis
# (and, at 63 and 500, on the 32-wide per-head axis)
ROUNDS = [1, 2, 63, 64, 500]
WRAP_ROUND = 63
HEADS, HEAD_DIM = 8, 32


def _cfg(base_cfg, model_name, data_name, kw, submodel='roll', roll_step=1,
         control=CONTROL):
    cfg = make_cfg(base_cfg, control, data_name=data_name,
                   model_name=model_name, **kw)
    cfg['submodel'] = submodel
    cfg['roll_step'] = roll_step
    return cfg


def _label_split(model_name, users=4, seed=0):
    """mask=1 splits: 2 classes per user (vision), a random half of the
    vocabulary (transformer)."""
    g = torch.Generator().manual_seed(seed)
    if model_name == 'transformer':
        return {u: sorted(torch.randperm(300, generator=g)[:150].tolist())
                for u in range(users)}
    return {u: sorted(torch.randperm(10, generator=g)[:2].tolist())
            for u in range(users)}


def _fed(cfg, model_name, seed=0):
    torch.manual_seed(seed)
    model = make_model(cfg, model_rate=1)
    return Federation(model.state_dict(), cfg['model_rate'],
                      _label_split(model_name), cfg)


# ------------------------------------------------- independent expectations
class _Expect:
    """Expected index tensors of one (rate, round), and a tally of which
    sliced axes wrapped."""

    def __init__(self, rate, rnd, step=1):
        self.rate, self.base = rate, (rnd - 1) * step
        self.wrapped = self.unwrapped = 0

    def _tally(self, s, n, width):
        if n < width:
            if s + n > width:
                self.wrapped += 1
            else:
                self.unwrapped += 1

    def win(self, width):
        n = math.ceil(width * self.rate)
        if n == width:
            return torch.arange(width)
        s = self.base % width
        self._tally(s, n, width)
        return torch.roll(torch.arange(width), -s)[:n]

    def heads(self):
        n = math.ceil(HEAD_DIM * self.rate)
        if n == HEAD_DIM:
            return torch.arange(HEADS * HEAD_DIM)
        s = self.base % HEAD_DIM
        self._tally(s, n, HEAD_DIM)
        one = torch.roll(torch.arange(HEAD_DIM), -s)[:n]
        return torch.cat([h * HEAD_DIM + one for h in range(HEADS)])

    def table(self, model_name):
        """{key: (out indices, in indices or None)} of the checked keys."""
        full = torch.arange
        if model_name == 'conv':
            return {
                'blocks.0.weight': (self.win(64), full(1)),
                'blocks.0.bias': (self.win(64), None),
                'blocks.5.weight': (self.win(128), self.win(64)),
                'blocks.7.weight': (self.win(128), None),       # norm
                'blocks.15.weight': (self.win(512), self.win(256)),
                'blocks.21.weight': (full(10), self.win(512)),  # classifier
                'blocks.21.bias': (full(10), None)}
        if model_name == 'resnet18':
            return {
                'conv1.weight': (self.win(64), full(3)),
                'layer1.0.n1.weight': (self.win(64), None),     # norm
                'layer2.0.conv1.weight': (self.win(128), self.win(64)),
                'layer2.0.conv2.weight': (self.win(128), self.win(128)),
                'layer2.0.shortcut.weight': (self.win(128), self.win(64)),
                'layer4.1.conv2.weight': (self.win(512), self.win(512)),
                'n4.bias': (self.win(512), None),
                'linear.weight': (full(10), self.win(512)),     # classifier
                'linear.bias': (full(10), None)}
        mha = 'transformer_encoder.layers.1.mha.'
        enc = 'transformer_encoder.layers.1.'
        return {
            'transformer_embedding.embedding.weight':
                (full(301), self.win(256)),
            'transformer_embedding.norm.weight': (self.win(256), None),
            mha + 'linear_q.weight': (self.heads(), self.win(256)),
            mha + 'linear_q.bias': (self.heads(), None),
            # the running index resets to the layer input after q and k
            mha + 'linear_k.weight': (self.heads(), self.win(256)),
            mha + 'linear_v.bias': (self.heads(), None),
            mha + 'linear_o.weight': (self.win(256), self.heads()),
            enc + 'linear1.weight': (self.win(512), self.win(256)),
            enc + 'linear2.weight': (self.win(256), self.win(512)),
            'decoder.linear2.weight': (full(300), self.win(256)),
            'decoder.linear2.bias': (full(300), None)}


# ------------------------------------------------------------------ 1. maps
def test_axis_roll_indices():
    ax = Axis.roll(3, 8, 6)
    assert ax.kind == ROLL and ax.n == 3
    assert ax.indices().tolist() == [6, 7, 0]
    assert Axis.roll(2, 5, 12).indices().tolist() == [2, 3]
    assert not ax.is_dense_prefix()


@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_maps(base_cfg, model_name, data_name, kw):
    cfg = _cfg(base_cfg, model_name, data_name, kw)
    fed = _fed(cfg, model_name)
    wrapped = unwrapped = 0
    for rnd in ROUNDS:
        for rate in LEVELS:
            pidx = fed.split_for_rate(rate, round=rnd)
            exp = _Expect(rate, rnd)
            for k, (out, inp) in exp.table(model_name).items():
                ps = pidx[k]
                assert torch.equal(ps.out.indices(), out), (k, rate, rnd)
                if inp is None:
                    assert ps.inp is None, k
                else:
                    assert torch.equal(ps.inp.indices(), inp), (k, rate, rnd)
            wrapped += exp.wrapped
            unwrapped += exp.unwrapped
    assert wrapped > 0 and unwrapped > 0, (wrapped, unwrapped)


def test_rounds_cover_every_wrap_class():
    """The chosen rounds wrap on the 64-, the 512- and the 32-wide axis,
    and leave each of them unwrapped at least once."""
    for width in (64, 512, 32):
        n = width // 2
        shifts = [(r - 1) % width for r in ROUNDS]
        assert any(s and s + n > width for s in shifts), width
        assert any(s and s + n <= width for s in shifts), width
    assert (ROUNDS[0] - 1) == 0


# ----------------------------------------------------------- 2. degenerate
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_degenerate(base_cfg, model_name, data_name, kw):
    """Round 1 is the static split; a full-width client gets whole axes at
    every round; static mode ignores the round.

    A window that covers its whole axis is FULL under roll mode at every
    round, round 1 included, where static mode says PREFIX(size): at round
    1 those axes are compared by n and by being a dense prefix, every other
    axis by kind and n."""
    roll = _fed(_cfg(base_cfg, model_name, data_name, kw), model_name)
    static = _fed(_cfg(base_cfg, model_name, data_name, kw, 'static'),
                  model_name)
    gp = roll.global_parameters

    def axes(ps, k):
        return [(ps.out, gp[k].size(0)),
                (ps.inp, gp[k].size(1) if gp[k].dim() > 1 else None)]

    for rate in LEVELS:
        today = static.split_for_rate(rate)
        first = roll.split_for_rate(rate, round=1)
        assert list(first.keys()) == list(today.keys())
        for k in today:
            for (a, size), (b, _) in zip(axes(first[k], k),
                                         axes(today[k], k)):
                if b is None:
                    assert a is None, k
                    continue
                assert a.n == b.n, k
                if b.kind == PREFIX and b.n == size:
                    assert a.kind == FULL, k
                else:
                    assert a.kind == b.kind, (k, a, b)
                assert torch.equal(a.indices(), b.indices()), k
        # static mode ignores the round; so does roll mode without one
        for pidx in (static.split_for_rate(rate, round=WRAP_ROUND),
                     roll.split_for_rate(rate)):
            for k in today:
                for (a, _), (b, _) in zip(axes(pidx[k], k),
                                          axes(today[k], k)):
                    assert (a is None) == (b is None), k
                    if b is not None:
                        assert (a.kind, a.n) == (b.kind, b.n), k
                        assert torch.equal(a.indices(), b.indices()), k
    for rnd in ROUNDS:
        pidx = roll.split_for_rate(1.0, round=rnd)
        for k, ps in pidx.items():
            for a, size in axes(ps, k):
                if a is None:
                    continue
                # q/k/v stay GATHER; a head taken whole is not permuted
                assert a.kind in (FULL, GATHER), (k, rnd, a)
                assert torch.equal(a.indices(), torch.arange(size)), (k, rnd)


def test_invalid_submodel_raises(base_cfg):
    cfg = _cfg(base_cfg, 'conv', 'MNIST', {}, submodel='random')
    with pytest.raises(ValueError):
        _fed(cfg, 'conv')


def test_cfg_without_keys_is_static(base_cfg):
    cfg = _cfg(base_cfg, 'conv', 'MNIST', {})
    del cfg['submodel'], cfg['roll_step']
    fed = _fed(cfg, 'conv')
    ps = fed.split_for_rate(0.5, round=WRAP_ROUND)['blocks.5.weight']
    assert ps.out.kind == PREFIX and ps.inp.kind == PREFIX


def test_config_and_cli_surface():
    from heterofl_amd.config import default_config
    from heterofl_amd.entry import parse_args
    cfg = default_config()
    assert cfg['submodel'] == 'static' and cfg['roll_step'] == 1
    out = parse_args(['--submodel', 'roll', '--roll_step', '3'], cfg=cfg)
    assert out['submodel'] == 'roll' and out['roll_step'] == 3
    assert parse_args([], cfg=cfg)['submodel'] == 'static'


# --------------------------------------------------------------- 3. slices
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_slices(base_cfg, model_name, data_name, kw):
    cfg = _cfg(base_cfg, model_name, data_name, kw)
    fed = _fed(cfg, model_name)
    gp = fed.global_parameters
    for rnd in (2, WRAP_ROUND, 500):
        for rate in (0.5, 0.0625):
            pidx = fed.split_for_rate(rate, round=rnd)
            sl = fed.slice_for_rate(rate, round=rnd)
            assert list(sl.keys()) == list(gp.keys())
            for k, v in gp.items():
                ps = pidx[k]
                ref = v.index_select(0, ps.out.indices())
                if v.dim() > 1:
                    ref = ref.index_select(1, ps.inp.indices())
                assert torch.equal(sl[k], ref), (k, rate, rnd)
        # distribute hands every slot the slice of its rate
        user_idx = [3, 0, 2, 1]
        local, pidx = fed.distribute(user_idx, resample=False, round=rnd)
        for m, u in enumerate(user_idx):
            sl = fed.slice_for_rate(fed.model_rate[u], round=rnd)
            assert list(sl.keys()) == list(local[m].keys())
            for k in sl:
                assert torch.equal(sl[k], local[m][k]), (k, m, rnd)
    # a rolled slice still loads into a model built at its rate
    local_model = make_model(cfg, model_rate=0.0625)
    local_model.load_state_dict(fed.slice_for_rate(0.0625, round=WRAP_ROUND))


# ----------------------------------------------------------- 4. round trip
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_round_trip(base_cfg, model_name, data_name, kw):
    """distribute -> combine with untouched client parameters leaves the
    global parameters bit-unchanged.  The global values are small integers,
    so the sum of c equal values and its division by c are exact in fp32
    whatever the count c: a changed bit is a wrong index, not rounding."""
    cfg = _cfg(base_cfg, model_name, data_name, kw)
    fed = _fed(cfg, model_name)
    g = torch.Generator().manual_seed(1)
    for v in fed.global_parameters.values():
        v.copy_(torch.randint(-8, 9, v.shape, generator=g).to(v.dtype))
    before = {k: v.clone() for k, v in fed.global_parameters.items()}
    user_idx = [0, 1, 2, 3]
    local, pidx = fed.distribute(user_idx, resample=False, round=WRAP_ROUND)
    assert any(ps.out.kind == ROLL for ps in pidx[3].values())
    fed.combine(local, pidx, user_idx)
    for k, v in fed.global_parameters.items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------- 5. coverage
def test_roll_trains_every_channel(base_cfg):
    """Level-e clients alone, roll_step 1, 64 consecutive rounds: the union
    of the covered channels of the conv model's 64-wide first layer is the
    whole layer; under static it is the first ceil(64 / 16) channels."""
    key, width = 'blocks.0.weight', 64
    covered = {}
    for mode in ('roll', 'static'):
        cfg = _cfg(base_cfg, 'conv', 'MNIST', {}, submodel=mode)
        torch.manual_seed(0)
        model = make_model(cfg, model_rate=1)
        fed = Federation(model.state_dict(), [0.0625] * 4,
                         {u: list(range(10)) for u in range(4)}, cfg)
        seen = torch.zeros(width, dtype=torch.bool)
        for rnd in range(1, width + 1):
            pidx = fed.split_model([0], round=rnd)
            cnt = fed.count_map(pidx, [0])[key]
            seen |= (cnt > 0).flatten(1).any(1)
        covered[mode] = seen
    assert covered['roll'].all()
    n = math.ceil(width / 16)
    assert covered['static'][:n].all() and not covered['static'][n:].any()


# ------------------------------------------------------------ 6. linearity
@pytest.mark.parametrize('model_name,data_name,kw', MODELS, ids=IDS)
def test_roll_accumulate_is_linear(base_cfg, model_name, data_name, kw):
    """accumulate over slots {0, 2} plus over {1, 3} equals accumulate over
    all four (integer-valued inputs: the sums are exact), and count_map
    equals the summed counts — what the multi-rank combine relies on."""
    cfg = _cfg(base_cfg, model_name, data_name, kw)
    fed = _fed(cfg, model_name)
    user_idx = [2, 0, 3, 1]
    local, pidx = fed.distribute(user_idx, resample=False, round=WRAP_ROUND)
    g = torch.Generator().manual_seed(2)
    local = [{k: torch.randint(-8, 9, v.shape, generator=g).to(v.dtype)
              for k, v in lp.items()} for lp in local]
    t_all, c_all = fed.accumulate(local, pidx, user_idx)
    t_a, c_a = fed.accumulate(local, pidx, user_idx, slots=[0, 2])
    t_b, c_b = fed.accumulate(local, pidx, user_idx, slots=[1, 3])
    cmap = fed.count_map(pidx, user_idx)
    for k in t_all:
        assert torch.equal(t_a[k] + t_b[k], t_all[k]), k
        assert torch.equal(c_a[k] + c_b[k], c_all[k]), k
        assert torch.equal(cmap[k], c_all[k]), k


# ----------------------------------------------------------- 7. end to end
def test_roll_three_rounds(base_cfg):
    from heterofl_amd.data import fetch_dataset, split_dataset
    from heterofl_amd.utils import process_dataset, make_optimizer
    cfg = _cfg(base_cfg, 'conv', 'MNIST', {}, roll_step=7)
    cfg['num_epochs'] = {'global': 3, 'local': 1}
    torch.manual_seed(0)
    ds = fetch_dataset('MNIST', synthetic=True, synthetic_size=80)
    process_dataset(ds, cfg)
    data_split, label_split = split_dataset(ds, cfg['num_users'], 'iid',
                                            cfg.get('classes_size'))
    model = make_model(cfg)
    runner = FedRunner(cfg, ds, data_split, label_split, model,
                       make_optimizer(model, cfg['lr'], cfg))
    fed = runner.federation
    before = {k: v.clone() for k, v in fed.global_parameters.items()}
    maps = []
    distribute = fed.distribute

    def recording(*a, **kw):
        out = distribute(*a, **kw)
        maps.append(out[1])
        return out

    fed.distribute = recording

    def global_loss():
        model.load_state_dict(fed.global_parameters)
        model.train(True)
        with torch.no_grad():
            batch = {'img': torch.stack([ds['train'][i]['img']
                                         for i in range(40)]),
                     'label': torch.tensor(ds['train'].target[:40])}
            return model(batch)['loss'].item()

    for ep in range(1, 4):
        user_idx = runner.train_round(ep)
        assert math.isfinite(global_loss()), ep
        # the level-e clients of round ep trained the window at 7 (ep - 1)
        slot = next(m for m, u in enumerate(user_idx)
                    if fed.model_rate[u] == 0.0625)
        ax = maps[-1][slot]['blocks.0.weight'].out
        assert ax.indices().tolist() == \
            [(7 * (ep - 1) + j) % 64 for j in range(4)], (ep, ax)
    for v in fed.global_parameters.values():
        assert torch.isfinite(v).all()
    w0, w1 = before['blocks.0.weight'], fed.global_parameters['blocks.0.weight']
    changed = (w0 != w1).flatten(1).any(1)
    assert changed[4:].any()   # beyond level e's static prefix of 4
