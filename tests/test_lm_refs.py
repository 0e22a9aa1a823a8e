"""CPU tests of the LM-kernel references in tests/lm_refs.py: the
quantisation-aware attention emulations against exact fp64 autograd, the two
emulations against each other, the fp32-vs-fp64 spread table the GPU tests
read, and the plain references against torch's own ops."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import lm_refs as R

CASES = R.ATTN_CASES
IDS = [R.attn_case_id(c) for c in CASES]
# second-order terms of the first-order bound: three roundings of 2^-8 each
SECOND_ORDER = (1 + R.U_BF16) ** 3


@pytest.mark.parametrize('io_name', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_emulation_within_rounding_of_exact(case, io_name):
    """fp64 emulation vs exact fp64 autograd on the same bf16-rounded
    inputs: the distance is bounded by what rounding P and dS to bf16 (2^-8
    relative each) can do, attn_rounding_bound, nothing fitted."""
    io = R.IO_DTYPES[io_name]
    q, k, v, g = R.attn_inputs(case, io)
    em = R.attn_emul(case, (q, k, v, g), torch.float64, io)
    ex = R.attn_exact(*(R.bf16r(t.double()) for t in (q, k, v, g)),
                      R.attn_temperature(case))
    # the bound is about P and dS only; the emulated output is unrounded
    bound = R.attn_rounding_bound(em)
    for name in R.ATTN_OUTPUTS:
        err = R.max_abs(em[name], ex[name])
        assert math.isfinite(err)
        assert err <= bound[name] * SECOND_ORDER + 1e-12, \
            (name, err, bound[name])


@pytest.mark.parametrize('case', [c for c in CASES if c[2] <= R.KV_BLOCK],
                         ids=[i for c, i in zip(CASES, IDS)
                              if c[2] <= R.KV_BLOCK])
def test_block_emulation_equals_small_at_one_block(case):
    """At S <= 64 the two schemes differ only in where P is rounded."""
    x = R.attn_inputs(case, torch.float32)
    temp = R.attn_temperature(case)
    a = R.attn_small_emul(*x, temp)
    b = R.attn_block_emul(*x, temp)
    ba, bb = R.attn_rounding_bound(a), R.attn_rounding_bound(b)
    for name in R.ATTN_OUTPUTS:
        err = R.max_abs(a[name], b[name])
        assert err <= (ba[name] + bb[name]) * SECOND_ORDER + 1e-12, \
            (name, err)


@pytest.mark.parametrize('io_name', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_spread_table(case, io_name):
    """Fill ATTN_SPREAD for every GPU case.  An emulation whose fp32 run is
    off by a whole bf16 rounding of the tensor (2^-8 of its norm) would be no
    yardstick; the max-abs spread stays under the rounding bound."""
    spread = R.attn_spread(case, io_name)
    assert (R.attn_case_id(case), io_name) in R.ATTN_SPREAD
    io = R.IO_DTYPES[io_name]
    em = R.attn_emul(case, R.attn_inputs(case, io), torch.float64, io)
    bound = R.attn_rounding_bound(em)
    for name in R.ATTN_OUTPUTS:
        fro, mx = spread[name]
        print('SPREAD {} {} {} relfro={:.3e} maxabs={:.3e}'.format(
            R.attn_case_id(case), io_name, name, fro, mx))
        assert math.isfinite(fro) and fro < R.U_BF16, (name, fro)
        assert mx <= bound[name], (name, mx, bound[name])


def test_scale_error_is_visible():
    """What the table is for: a 1 % error in inv_temp moves the emulation by
    far more than 10 x its fp32-vs-fp64 spread."""
    case = CASES[0]
    x = R.attn_inputs(case, torch.float32)
    temp = R.attn_temperature(case)
    good = R.attn_small_emul(*x, temp)
    bad = R.attn_small_emul(*x, temp / 1.01)
    spread = R.attn_emul_spread('small')
    for name in R.ATTN_OUTPUTS:
        moved = R.rel_fro(bad[name], good[name])
        print('SCALE1.01 {} moved={:.3e} 10xspread={:.3e}'.format(
            name, moved, 10 * spread[name][0]))
        assert moved > 10 * max(spread[name][0], 1e-6), name


@pytest.mark.parametrize('emul', ['small', 'block'])
def test_emulation_spread_table(emul):
    """The per-emulation table is the maximum of the per-case one."""
    table = R.attn_emul_spread(emul)
    assert table is R.ATTN_EMUL_SPREAD[emul]
    mine = [R.ATTN_SPREAD[(R.attn_case_id(c), io)] for c in CASES
            for io in R.IO_DTYPES if (c[0] == 'small') == (emul == 'small')]
    for name in R.ATTN_OUTPUTS:
        print('EMUL_SPREAD {} {} relfro={:.3e} maxabs={:.3e}'.format(
            emul, name, *table[name]))
        assert table[name][0] == max(r[name][0] for r in mine)
        assert table[name][1] == max(r[name][1] for r in mine)
        assert 1e-6 < table[name][0] < R.U_BF16


def test_stable_inputs_reach_60():
    for case in CASES:
        if case[5] == 'randn':
            continue
        q, k, _, _ = R.attn_inputs(case, torch.float32)
        s = q.double() @ k.double().transpose(1, 2) / R.attn_temperature(case)
        assert 55 < s.max().item() < 65 and -65 < s.min().item() < -40
        top = s.argmax(-1)
        if case[5] == 'stable_last':
            assert bool((top >= 128).all())
        elif case[5] == 'stable_first':
            assert bool((top < 64).all())


def test_bf16_helpers():
    x = torch.tensor([1.0, 1.5, 0.99, 3.0, 1e-3, 300.0], dtype=torch.float64)
    ulp = R.bf16_ulp(x)
    assert ulp.tolist()[:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6]
    nxt = (x.to(torch.bfloat16).float().double() + ulp).to(torch.bfloat16)
    assert bool((nxt.double() > x.to(torch.bfloat16).double()).all())
    assert bool(((R.bf16r(x) - x).abs() <= ulp / 2).all())


def test_layernorm_ref_matches_formula():
    torch.manual_seed(0)
    Rn, B, S, E = 3, 2, 5, 96
    x = torch.randn(Rn, B, S, E, dtype=torch.float64) * 2 + 3
    g, b = torch.rand(Rn, E).double() + 0.5, torch.randn(Rn, E).double()
    dy = torch.randn(Rn, B, S, E, dtype=torch.float64)
    ref = R.layernorm_ref(x, g, b, dy)
    mu = x.mean(-1, keepdim=True)
    xh = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    assert R.max_abs(ref['y'], xh * g.view(Rn, 1, 1, E)
                     + b.view(Rn, 1, 1, E)) < 1e-12
    assert R.max_abs(ref['dgamma'], (dy * xh).sum((1, 2))) < 1e-11
    assert R.max_abs(ref['dbeta'], dy.sum((1, 2))) < 1e-12
    dxh = dy * g.view(Rn, 1, 1, E)
    dx = (dxh - dxh.mean(-1, keepdim=True)
          - xh * (dxh * xh).mean(-1, keepdim=True)) \
        / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    assert R.max_abs(ref['dx'], dx) < 1e-11


@pytest.mark.parametrize('masked', [True, False])
def test_lm_ce_ref_matches_cross_entropy(masked):
    torch.manual_seed(0)
    Rn, B, S, V = 3, 2, 4, 37
    logits = torch.randn(Rn, B, S, V, dtype=torch.float64) * 5
    tokens = torch.randint(0, V, (Rn, B, S))
    mask = (torch.rand(Rn, V) > 0.3).float() if masked else None
    w = torch.rand(Rn, dtype=torch.float64) + 0.5
    ref = R.lm_ce_ref(logits, tokens, mask, w)
    z = logits.clone()
    if masked:
        z = z * mask.double().view(Rn, 1, 1, V)
    want = torch.stack([F.cross_entropy(z[r].reshape(-1, V),
                                        tokens[r].reshape(-1))
                        for r in range(Rn)])
    assert R.max_abs(ref['losses'], want) < 1e-12
    if masked:
        dead = (mask == 0).view(Rn, 1, 1, V).expand_as(logits)
        assert bool((ref['dlogits'][dead] == 0).all())
    # rows of dlogits sum to 0 over the live + masked softmax mass only when
    # nothing is masked
    if not masked:
        assert ref['dlogits'].sum(-1).abs().max().item() < 1e-12


def test_dropout_refs_match_autograd():
    torch.manual_seed(0)
    x = torch.randn(1000, dtype=torch.float64, requires_grad=True)
    keep = torch.rand(1000) > 0.3
    dy = torch.randn(1000, dtype=torch.float64)
    rate, p = 0.5, 0.3
    y = F.gelu(x / rate) * keep.double() / (1 - p)
    (dx,) = torch.autograd.grad(y, x, dy)
    ref = R.gelu_drop_ref(x, keep, dy, rate, p)
    assert R.max_abs(ref['y'], y) < 1e-13 and R.max_abs(ref['dx'], dx) < 1e-13
    s = torch.randn(1000, dtype=torch.float64, requires_grad=True)
    h = torch.randn(1000, dtype=torch.float64, requires_grad=True)
    t = s + F.dropout(h / rate, 0.0) * keep.double() / (1 - p)
    ds, dh = torch.autograd.grad(t, (s, h), dy)
    ref = R.res_drop_ref(s, h, keep, dy, rate, p)
    assert R.max_abs(ref['t'], t) < 1e-13
    assert torch.equal(ref['dsrc'], ds) and R.max_abs(ref['dh'], dh) < 1e-13


def test_embed_pos_ref_matches_embedding():
    torch.manual_seed(0)
    Rn, B, S, E, V, P = 2, 3, 5, 16, 11, 9
    table = torch.randn(Rn, V, E, dtype=torch.float64)
    pos = torch.randn(Rn, P, E, dtype=torch.float64)
    ids = torch.randint(0, V, (Rn, B, S))
    ids[0] = 4                       # one never-varying client
    dy = torch.randn(Rn, B, S, E, dtype=torch.float64)
    ref = R.embed_pos_ref(ids, table, pos, dy, 0.5)
    for r in range(Rn):
        want = (F.embedding(ids[r], table[r]) + pos[r, :S]) / 0.5
        assert R.max_abs(ref['out'][r], want) < 1e-13
    assert bool((ref['dpos'][:, S:] == 0).all())
    assert bool((ref['dtable'][0, :4] == 0).all())
    assert R.max_abs(ref['dtable'][0, 4], dy[0].sum((0, 1)) / 0.5) < 1e-12
    assert R.max_abs(ref['dpos'][:, :S], dy.sum(1) / 0.5) < 1e-12
