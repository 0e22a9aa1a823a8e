"""CPU tests of the vision-kernel references in tests/vision_refs.py: each
fp64 reference against torch's own fp64 ops, the fp32-vs-fp64 spread tables
the GPU tolerances hang on (pytest -s prints them; the docstring of
tests/test_gpu_vision_kernels.py quotes them), the ReLU-boundary condition of
every BN / GN case, and the one-pass variance probe of profiles/NOTES.md."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vision_refs as V

F64, F32 = torch.float64, torch.float32
IOS = list(V.IO_DTYPES)
REL = 1e-12


def _agree(tag, a, ref, scale=None):
    """1e-12 relative to the largest reference value, or to `scale` where
    the value is what is left of larger terms that cancel."""
    scale = max(ref.abs().max().item(), scale or 0.0) or 1.0
    err = V.max_abs(a, ref)
    assert err <= REL * scale, (tag, err, scale)


def _leaf(t):
    return None if t is None else t.double().requires_grad_(True)


def _spread_lines(kernel, cid, names, r32, r64):
    for name in names:
        a, b = getattr(r32, name), getattr(r64, name)
        if a is None:
            continue
        mx, fro = V.max_abs(a, b), V.rel_fro(a, b)
        print('VSPREAD {} {} {} maxabs={:.3e} relfro={:.3e} maxref={:.3e}'
              .format(kernel, cid, name, mx, fro, b.abs().max().item()))
        assert math.isfinite(mx) and math.isfinite(fro), (cid, name)
        # an fp32 run further off than one bf16 rounding is no yardstick
        assert fro < 2.0 ** -8, (cid, name, fro)


# ------------------------------------------------------------------ BN / GN
def _torch_norm(kind, x, w, b, dy, G):
    x64 = x.double().requires_grad_(True)
    w64, b64 = _leaf(w), _leaf(b)
    e = V.eps32(V.EPS, F64)
    if kind == 'bn':
        z = F.batch_norm(x64, None, None, w64, b64, training=True, eps=e)
    else:
        z = F.group_norm(x64, G, w64, b64, eps=e)
    y = F.relu(z)
    leaves = [t for t in (x64, w64, b64) if t is not None]
    grads = torch.autograd.grad(y, leaves, dy.double())
    return y.detach(), grads


def _check_norm_against_torch(kind, tag, x, w, b, dy, G=None):
    for one_pass in (True, False):
        if kind == 'bn':
            ref = V.bn_relu(x, w, b, dy, dtype=F64, one_pass=one_pass)
        else:
            ref = V.gn_relu(x, w, b, dy, G, dtype=F64, one_pass=one_pass)
        y, grads = _torch_norm(kind, x, w, b, dy, G)
        t = (tag, one_pass)
        _agree(t + ('y',), ref.y, y)
        # dx = invstd g (d - k1 - xhat k2): the terms are of this size
        top = (ref.invstd.max() * dy.double().abs().max()
               * (w.double().abs().max() if w is not None else 1.0)).item()
        _agree(t + ('dx',), ref.dx, grads[0], top)
        if w is not None:
            _agree(t + ('dgamma',), ref.dgamma, grads[1])
            _agree(t + ('dbeta',), ref.dbeta, grads[2])
        xs = x.double()
        if kind == 'bn':
            m = xs.mean((0, 2, 3))
            v = xs.var((0, 2, 3), unbiased=False)
        else:
            xg = xs.reshape(xs.size(0) * G, -1)
            m, v = xg.mean(1), xg.var(1, unbiased=False)
        _agree(t + ('mean',), ref.mean, m)
        _agree(t + ('invstd',), ref.invstd,
               1.0 / torch.sqrt(v + V.eps32(V.EPS, F64)))


BN_FREE = [v for v in V.BN_VARIANTS if v[0] in V.BN_BOUNDARY_FREE]
BN_FREE_IDS = [V.bn_variant_id(v) for v in BN_FREE]


@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('variant', BN_FREE, ids=BN_FREE_IDS)
def test_bn_ref_matches_torch(variant, io_name):
    case, affine = variant
    x, dy, w, b = V.bn_inputs(case, io_name, affine)
    if x.numel() // x.size(1) == 1:
        # F.batch_norm refuses one value per channel in training; the closed
        # form: var 0, invstd = eps^-1/2, y = relu(b), dx = 0
        ref = V.bn_relu(x, w, b, dy, dtype=F64)
        bb = b.double() if affine else torch.zeros(x.size(1), dtype=F64)
        _agree('y', ref.y, bb.clamp_min(0).view(1, -1, 1, 1).expand_as(ref.y))
        _agree('invstd', ref.invstd,
               torch.full_like(ref.invstd, V.eps32(V.EPS, F64) ** -0.5))
        assert bool((ref.dx == 0).all()) and bool((ref.dgamma == 0).all())
        _agree('dbeta', ref.dbeta,
               (dy.double() * (bb.view(1, -1, 1, 1) > 0)).sum((0, 2, 3)))
        return
    _check_norm_against_torch('bn', case, x, w, b, dy)


def test_bn_split3_ref_matches_torch():
    x, dy, w, b = V.bn_inputs('split3', 'fp32', True)
    _check_norm_against_torch('bn', 'split3', x, w, b, dy)


@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', list(V.GN_CASES))
def test_gn_ref_matches_torch(case, io_name, affine):
    x, dy, w, b, G = V.gn_inputs(case, io_name, affine)
    _check_norm_against_torch('gn', case, x, w, b, dy, G)


def test_gn_ref_rejects_bad_grouping():
    x = torch.randn(2, 6, 2, 2)
    with pytest.raises(ValueError):
        V.gn_relu(x, None, None, x, 4)


def _boundary(pre32, pre64):
    """The set an fp32 error could flip.  pre == 0 exactly (an all-zero or
    constant channel or a one-element group, without affine: x == mean bit
    for bit) is left out: the kernels' backward masks and the GN forward
    compute (x - mean) * invstd * g + b, where xhat is exactly 0 in any
    arithmetic and `pre > 0` is false as in the reference.  The BN forward's
    x * scale + shift is a rounding residual there, either sign, of size
    2^-24 |x * scale|: y's tolerance has to cover it, and in `special` it
    does; see BN_VARIANTS for m1."""
    tau = V.boundary_tau(pre32, pre64)
    return V.relu_boundary(pre64, tau) & (pre64 != 0), tau


@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('variant', BN_FREE, ids=BN_FREE_IDS)
def test_bn_cases_have_no_boundary_elements(variant, io_name):
    case, affine = variant
    x, dy, w, b = V.bn_inputs(case, io_name, affine)
    r64 = V.bn_relu(x, w, b, dy, dtype=F64)
    r32 = V.bn_relu(x, w, b, dy, dtype=F32)
    near, tau = _boundary(r32.pre, r64.pre)
    print('VBOUNDARY bn {} {} affine={} tau={:.3e} near={}'.format(
        case, io_name, affine, tau, int(near.sum())))
    assert int(near.sum()) == 0
    _spread_lines('bn', '{}-{}-{}'.format(case, io_name,
                                          'affine' if affine else 'plain'),
                  V.NORM_OUTPUTS + ('pre',), r32, r64)


@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', list(V.GN_CASES))
def test_gn_cases_have_no_boundary_elements(case, io_name, affine):
    x, dy, w, b, G = V.gn_inputs(case, io_name, affine)
    r64 = V.gn_relu(x, w, b, dy, G, dtype=F64)
    r32 = V.gn_relu(x, w, b, dy, G, dtype=F32)
    near, tau = _boundary(r32.pre, r64.pre)
    print('VBOUNDARY gn {} {} affine={} tau={:.3e} near={}'.format(
        case, io_name, affine, tau, int(near.sum())))
    assert int(near.sum()) == 0
    _spread_lines('gn', '{}-{}-{}'.format(case, io_name,
                                          'affine' if affine else 'plain'),
                  V.NORM_OUTPUTS + ('pre',), r32, r64)


@pytest.mark.parametrize('io_name', IOS)
def test_bn_split3_boundary_share(io_name):
    """8.5 M elements: some lie within tau of the boundary whatever the
    seed.  They are excluded from the y / dx comparison on the GPU, and what
    flipping them can do to the sums over the mask is bounded exactly; the
    excluded share must stay under 1e-4."""
    x, dy, w, b = V.bn_inputs('split3', io_name, True)
    r64 = V.bn_relu(x, w, b, dy, dtype=F64)
    r32 = V.bn_relu(x, w, b, dy, dtype=F32)
    near, tau = _boundary(r32.pre, r64.pre)
    share = near.double().mean().item()
    s_gamma, s_beta, s_dx = V.bn_flip_slack(x, w, dy, r64, near)
    print('VBOUNDARY bn split3 {} tau={:.3e} near={} share={:.3e} '
          'slack dgamma={:.3e} dbeta={:.3e} dx={:.3e}'.format(
              io_name, tau, int(near.sum()), share, s_gamma.max().item(),
              s_beta.max().item(), s_dx.max().item()))
    assert share <= V.SPLIT3_MAX_SHARE
    _spread_lines('bn', 'split3-' + io_name, V.NORM_OUTPUTS + ('pre',),
                  r32, r64)
    # the fp32 reference itself obeys the rule it sets for the kernels
    keep = ~near
    assert V.max_abs(r32.y[keep], r64.y[keep]) <= V.fp32_tol(r32.y, r64.y)
    flipped = (r32.pre > 0) != (r64.pre > 0)
    assert bool((near | ~flipped).all())


def test_bn_one_pass_offset_probe():
    """invstd of randn + offset, relative error against fp64: the kernels'
    one-pass fp32 variance, a two-pass fp32 variance, torch's fp32
    batch_norm.  The table is in profiles/NOTES.md."""
    gen = torch.Generator().manual_seed(0)
    base = torch.randn(10, 8, 32, 32, generator=gen)
    dy = torch.zeros_like(base)
    worst = {}
    for off in (0.0, 8.0, 64.0):
        x = base + off
        r64 = V.bn_relu(x, None, None, dy, dtype=F64, one_pass=False)
        one = V.bn_relu(x, None, None, dy, dtype=F32, one_pass=True)
        two = V.bn_relu(x, None, None, dy, dtype=F32, one_pass=False)
        _, _, t_is = torch.native_batch_norm(x, None, None, None, None, True,
                                             0.0, V.EPS)
        rel = lambda a: ((a.double() - r64.invstd).abs()
                         / r64.invstd).max().item()
        worst[off] = (rel(one.invstd), rel(two.invstd), rel(t_is))
        print('VOFFSET mu/sigma={:g} one_pass_fp32={:.1e} two_pass_fp32={:.1e}'
              ' torch_fp32={:.1e}'.format(off, *worst[off]))
    # exact to 1e-5 up to mu/sigma = 8, (mu/sigma)^2 * 1e-7 beyond
    assert worst[0.0][0] < 1e-6 and worst[8.0][0] < 1e-5
    assert worst[64.0][0] < 10 * 64.0 ** 2 * 1e-7
    assert worst[64.0][0] > 10 * worst[64.0][1]
    for off in worst:
        assert worst[off][1] < 1e-6 and worst[off][2] < 1e-6


# ---------------------------------------------------------------- masked CE
@pytest.mark.parametrize('case', V.CE_CASES,
                         ids=[V.ce_case_id(c) for c in V.CE_CASES])
def test_masked_ce_ref_matches_torch(case):
    scores, labels, mask, up = V.ce_inputs(case)
    ref = V.masked_ce(scores, labels, mask, up, dtype=F64)
    N, R, C = scores.shape
    s = scores.double().requires_grad_(True)
    z = s if mask is None else s.masked_fill(mask.unsqueeze(0) == 0, 0)
    logp = F.log_softmax(z, dim=-1)
    nll = -logp.gather(2, labels.unsqueeze(-1)).squeeze(-1)
    losses = nll.mean(0)
    (ds,) = torch.autograd.grad((losses * up.double()).sum(), s)
    _agree('losses', ref.losses, losses.detach())
    _agree('dscores', ref.dscores, ds)
    _agree('sum_nll', ref.metrics[:, 0], nll.detach().sum(0))
    assert torch.equal(ref.metrics[:, 1],
                       (z.argmax(-1) == labels).double().sum(0))
    assert bool((ref.metrics[:, 2] == N).all())
    if mask is not None:
        dead = (mask == 0).unsqueeze(0).expand(N, R, C)
        assert bool((ref.dscores[dead] == 0).all())
    # no ties among live scores: the prediction does not hang on tie rules
    live = z.detach() if mask is None else \
        z.detach().masked_fill(mask.unsqueeze(0) == 0, float('nan'))
    srt = live.sort(-1).values
    gaps = (srt[..., 1:] - srt[..., :-1])
    assert not bool((gaps == 0).any())
    r32 = V.masked_ce(scores, labels, mask, up, dtype=F32)
    assert torch.equal(r32.metrics[:, 1].double(), ref.metrics[:, 1])
    _spread_lines('ce', V.ce_case_id(case), ('losses', 'dscores'), r32, ref)
    nll_slack, d_slack = V.masked_ce_intrinsic_slack(scores, labels, mask, up)
    print('VSLACK ce {} nll={:.3e} dscores={:.3e}'.format(
        V.ce_case_id(case), nll_slack.max().item(), d_slack.max().item()))
    assert nll_slack.max().item() < 1e-3 and d_slack.max().item() < 1e-3


# --------------------------------------------------------------------- head
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', V.HEAD_CASES,
                         ids=[V.head_case_id(c) for c in V.HEAD_CASES])
def test_head_ref_matches_torch(case, io_name, bias):
    N, R, C, H, W, J = case
    feat, w, b, ds = V.head_inputs(case, io_name, bias)
    ref = V.head(feat, w, b, ds, R, dtype=F64)
    f = feat.double().requires_grad_(True)
    w64, b64 = _leaf(w), _leaf(b)
    pooled = F.adaptive_avg_pool2d(f, 1).reshape(N, R, C)
    scores = torch.einsum('nrc,rjc->nrj', pooled, w64)
    if bias:
        scores = scores + b64
    leaves = [f, w64] + ([b64] if bias else [])
    grads = torch.autograd.grad(scores, leaves, ds.double())
    _agree('scores', ref.scores, scores.detach())
    _agree('pooled', ref.pooled, pooled.detach())
    _agree('dfeat', ref.dfeat, grads[0])
    _agree('dw', ref.dw, grads[1])
    if bias:
        _agree('db', ref.db, grads[2])
    else:
        assert ref.db is None
    r32 = V.head(feat, w, b, ds, R, dtype=F32)
    _spread_lines('head', '{}-{}-{}'.format(V.head_case_id(case), io_name,
                                            'bias' if bias else 'nobias'),
                  V.HeadOut._fields, r32, ref)


def test_head_lds_case_is_over_the_stage():
    N, R, C, H, W, J = V.HEAD_LDS_CASE
    assert N * J * 4 > 64 * 1024 >= (N - 7) * J * 4


# ----------------------------------------------------------------- clip+SGD
def test_clip_sgd_ref_matches_torch():
    params, grads, bufs = V.sgd_inputs()
    R, h = V.SGD_R, V.SGD_HYPER
    ref = V.clip_sgd(params, grads, bufs, R, steps=V.SGD_STEPS, dtype=F64,
                     **h)
    # one torch optimizer per client over that client's slices
    cl = [[torch.nn.Parameter(p.double().reshape(R, -1)[r].clone())
           for p in params] for r in range(R)]
    opts = [torch.optim.SGD(ps, lr=h['lr'], momentum=h['mom'],
                            weight_decay=h['wd']) for ps in cl]
    for step in range(V.SGD_STEPS):
        for r in range(R):
            for p, g in zip(cl[r], grads[step]):
                p.grad = g.double().reshape(R, -1)[r].clone()
            norm = torch.nn.utils.clip_grad_norm_(cl[r], h['max_norm'])
            _agree(('norm', step, r), ref[step][2][r], norm.double())
            opts[r].step()
        for i in range(len(params)):
            want = torch.cat([cl[r][i].detach() for r in range(R)])
            _agree(('param', step, i), ref[step][0][i], want)
            if step == 0:
                continue
            buf = torch.cat([opts[r].state[cl[r][i]]['momentum_buffer']
                             for r in range(R)])
            _agree(('buf', step, i), ref[step][1][i], buf)
    n0 = ref[0][2]
    assert abs(n0[0].item() - 50) < 1e-4 and abs(n0[1].item() - 0.1) < 1e-6
    assert n0[2].item() == 0
    r32 = V.clip_sgd(params, grads, bufs, R, steps=V.SGD_STEPS, dtype=F32,
                     **h)
    for step in range(V.SGD_STEPS):
        for name, k in (('param', 0), ('buf', 1)):
            mx = max(V.max_abs(a, c)
                     for a, c in zip(r32[step][k], ref[step][k]))
            top = max(c.abs().max().item() for c in ref[step][k])
            print('VSPREAD sgd step{} {} maxabs={:.3e} maxref={:.3e}'.format(
                step, name, mx, top))
            assert mx < 2.0 ** -8 * top
