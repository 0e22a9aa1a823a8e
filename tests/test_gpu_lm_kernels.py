"""GPU tests of the LM training kernels (attention.hip, layernorm.hip,
lm_ce.hip, lm_fused.hip) at edge shapes against the fp64 references of
tests/lm_refs.py.  Every case runs forward and backward with a random
upstream gradient; every test prints `LMK <kernel> <case> <output> err=
bound=` lines before it asserts (pytest -s shows them).

What each tolerance rests on
----------------------------
attention (relative Frobenius error against the fp64 emulation that rounds
where the kernel rounds): 10 x ATTN_EMUL_SPREAD, the fp32-vs-fp64 spread of
that emulation on the CPU, maximum over the case list and both io dtypes.
The margin of 10 covers __expf against exp and the handful of P / dS entries
that land on the other side of a bf16 rounding boundary.  Measured on the
CPU (test_lm_refs.py prints them):

    emulation  output  rel Frobenius  max abs    x10 = tolerance
    small      out     7.1e-05        2.8e-04    7.1e-04
    small      dq      2.6e-05        1.2e-04    2.6e-04
    small      dk      2.1e-05        1.0e-04    2.1e-04
    small      dv      5.0e-05        2.4e-04    5.0e-04
    block      out     9.9e-05        3.1e-03    9.9e-04
    block      dq      5.5e-04        5.2e-03    5.5e-03
    block      dk      1.2e-04        3.5e-03    1.2e-03
    block      dv      7.5e-05        2.4e-03    7.5e-04

(a case without a flipped entry sits at ~5e-8; the block rows are set by the
stable_first case, whose softmax mass sits on six keys).  bf16 outputs add
half a bf16 ulp of the result, 2^-8 of its norm.  A 1 % error in inv_temp
moves out/dq/dk/dv of the first case by 1.1e-2 .. 1.7e-2.  Largest fp32
figures seen on an MI355X: small 2.6e-05 (dq), block 5.2e-04 (dq,
stable_first), 1.9e-05 (out); the GPU flips the entries the fp32 emulation
flips in most cases.

attention (max abs): lm_refs.attn_rounding_bound, derived from 2^-8 relative
rounding of P and dS; 2^-8 max|v| for out.
attention (sanity): the looser comparison with the unquantised reference
that tests/test_gpu.py makes, 0.03 / 0.05 (fp32) and 0.06 / 0.12 (bf16).

layernorm, lm_ce (fp32), embed_pos gradients: 16 x the error of torch's own
fp32 path against fp64 on the same input, computed inside the test.
bf16 outputs: one bf16 ulp of the fp64 reference value (layernorm: half an
ulp on top of the fp32 tolerance).
dropout glue, fp32: 1e-5 (1 + |ref|), the 1e-5 of the existing p = 0 test as
absolute plus relative tolerance (erf-form GELU in fp32 cannot be relatively
accurate in its left tail: 1 + erf cancels).
mask statistics: 6 sigma of the binomial.
"""
import math

import pytest
import torch

from tests import lm_refs as R

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

DEV = 'cuda:0'
IOS = ['fp32', 'bf16']
U = R.U_BF16


def _report(kernel, case, name, err, bound):
    print('LMK {} {} {} err={:.3e} bound={:.3e}'.format(kernel, case, name,
                                                        err, bound))


def _finite(t):
    return bool(torch.isfinite(t.float()).all())


# ================================================================ attention
def _run_attention(path, x, temp):
    """Kernel outputs of a case as CPU tensors in the io dtype."""
    from heterofl_amd.ops import require_native
    from heterofl_amd.ops.fused import fused_attention
    q, k, v, g = (t.to(DEV) for t in x)
    if path == 'block1':
        ext = require_native()
        out, lse = ext.attn_fwd_block(q, k, v, temp)
        dq, dk, dv = ext.attn_bwd_block(g, q, k, v, out, lse, temp)
    else:
        assert (q.size(1) <= 64) == (path == 'small')
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        out = fused_attention(q, k, v, temp)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), g)
    return {'out': out.detach().cpu(), 'dq': dq.cpu(), 'dk': dk.cpu(),
            'dv': dv.cpu()}


def _check_attention(case, io_name, got, x):
    io = R.IO_DTYPES[io_name]
    cid = R.attn_case_id(case) + '-' + io_name
    em = R.attn_emul(case, x, torch.float64, io)
    spread = R.attn_emul_spread(case[0])
    hard = R.attn_rounding_bound(em, io)
    exact = R.attn_exact(*x, R.attn_temperature(case))
    loose = {'fp32': (0.03, 0.05), 'bf16': (0.06, 0.12)}[io_name]
    fails = []
    for name in R.ATTN_OUTPUTS:
        assert _finite(got[name]), (cid, name)
        fro = R.rel_fro(got[name], em[name])
        tol = 10 * max(spread[name][0], 1e-6) + (U if io_name == 'bf16' else 0)
        mx = R.max_abs(got[name], em[name])
        sane = R.max_abs(got[name], exact[name])
        # the absolute sanity tolerances were set for unit-scale outputs; the
        # +-60-score cases have gradients of up to 24, so theirs scale with
        # the largest reference value
        lax = loose[0 if name == 'out' else 1]
        if case[5] != 'randn':
            lax *= max(1.0, exact[name].abs().max().item())
        _report('attn', cid, name + '.relfro', fro, tol)
        _report('attn', cid, name + '.maxabs', mx, hard[name])
        _report('attn', cid, name + '.sanity', sane, lax)
        if fro > tol:
            fails.append((name, 'relfro', fro, tol))
        if mx > hard[name]:
            fails.append((name, 'maxabs', mx, hard[name]))
        if sane >= lax:
            fails.append((name, 'sanity', sane, lax))
    assert not fails, (cid, fails)


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', R.ATTN_CASES,
                         ids=[R.attn_case_id(c) for c in R.ATTN_CASES])
def test_attention_matches_emulation(case, io_name):
    """Both attention paths, random and +-60-score inputs, against the fp64
    emulation of their own rounding scheme."""
    x = R.attn_inputs(case, R.IO_DTYPES[io_name])
    got = _run_attention(case[0], x, R.attn_temperature(case))
    _check_attention(case, io_name, got, x)


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('shape', [(2, 64, 32), (2, 17, 5)])
def test_attention_one_block_agrees_with_small_path(shape, io_name):
    """The blockwise kernels at S <= 64 against the small-S kernels on the
    same inputs, gradients included: the two schemes round P at different
    points, so they may differ by the sum of their rounding bounds."""
    io = R.IO_DTYPES[io_name]
    case = ('block1',) + shape + (None, 'randn')
    x = R.attn_inputs(case, io)
    temp = R.attn_temperature(case)
    small = _run_attention('small', x, temp)
    block = _run_attention('block1', x, temp)
    bs = R.attn_rounding_bound(R.attn_small_emul(*x, temp), io)
    bb = R.attn_rounding_bound(R.attn_block_emul(*x, temp, io_dtype=io), io)
    for name in R.ATTN_OUTPUTS:
        err = R.max_abs(small[name], block[name])
        _report('attn', 'paths-{}-{}'.format('x'.join(map(str, shape)),
                                             io_name), name, err,
                bs[name] + bb[name])
        assert err <= bs[name] + bb[name], (name, err)


def _structured(B, S, d, jstars, io):
    """q_i = k[j*] = 16 u (u = +-1), every other key 0: the score gap is
    256 sqrt(d) >= 256, so P is exactly one-hot at j* after rounding
    (exp(-256) is 0 in fp32 and in bf16).  v in [-4, 4] and dO in {-1, 0, 1}
    are integers: every product and sum is exact in fp32, and in bf16."""
    gen = torch.Generator().manual_seed(S * 100 + d)
    u = torch.randint(0, 2, (d,), generator=gen).float() * 2 - 1
    q = (16 * u).expand(B, S, d).clone()
    k = torch.zeros(B, S, d)
    for b, j in enumerate(jstars):
        k[b, j] = 16 * u
    v = torch.randint(-4, 5, (B, S, d), generator=gen).float()
    g = torch.randint(-1, 2, (B, S, d), generator=gen).float()
    return tuple(t.to(io) for t in (q, k, v, g))


@needs_gpu
@pytest.mark.parametrize('d', [1, 8, 32])
@pytest.mark.parametrize('S', [33, 64, 65, 130])
def test_attention_structured_exact(S, d):
    """One-hot softmax with integer values: out, dV exact, dQ = dK = 0.
    Pins row/column indexing, the zero padding and the tail blocks with no
    tolerance to hide behind."""
    js = sorted({j for j in (0, 15, 16, 31, 32, 63, 64, S - 1) if j < S})
    for io_name in IOS:
        io = R.IO_DTYPES[io_name]
        for n, j in enumerate(js):
            jstars = (j, js[(n + 1) % len(js)])      # one j* per batch row
            x = _structured(2, S, d, jstars, io)
            got = _run_attention('small' if S <= 64 else 'block', x,
                                 float(d) ** 0.5)
            v, g = x[2].float(), x[3].float()
            for b, jb in enumerate(jstars):
                tag = (S, d, io_name, b, jb)
                assert torch.equal(got['out'][b].float(),
                                   v[b, jb].expand(S, d)), tag
                want = torch.zeros(S, d)
                want[jb] = g[b].sum(0)
                assert torch.equal(got['dv'][b].float(), want), tag
                assert got['dq'][b].float().abs().max().item() <= 1e-6, tag
                assert got['dk'][b].float().abs().max().item() <= 1e-6, tag


# ================================================================ layernorm
def _ln_check(tag, x, w, b, g, io_name):
    from heterofl_amd.ops.fused import fused_layernorm
    io = R.IO_DTYPES[io_name]
    Rn = w.size(0)
    x, g = x.to(io), g.to(io)
    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True)
    y = fused_layernorm(xg, wg, bg, Rn)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), g.to(DEV))
    got = {'y': y.detach().cpu(), 'dx': dx.cpu(), 'dgamma': dw.cpu(),
           'dbeta': db.cpu()}
    ref = R.layernorm_ref(x, w, b, g, dtype=torch.float64)
    r32 = R.layernorm_ref(x, w, b, g, dtype=torch.float32)
    fails = []
    for name in ('y', 'dx', 'dgamma', 'dbeta'):
        tol = 16 * R.max_abs(r32[name], ref[name])
        err = (got[name].double() - ref[name]).abs()
        if io_name == 'bf16' and name in ('y', 'dx'):
            err = (err - R.bf16_ulp(ref[name]) / 2).clamp_min(0)
        err = err.max().item()
        _report('ln', tag + '-' + io_name, name, err, tol)
        assert math.isfinite(err)
        if err > tol:
            fails.append((name, err, tol))
    assert not fails, (tag, io_name, fails)


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('shape', [(5, 3, 64, 256), (2, 1, 3, 16),
                                   (3, 2, 5, 96), (1, 1, 7, 1024),
                                   (2, 3, 1, 65)])
def test_layernorm_matches_fp64(shape, io_name):
    Rn, B, S, E = shape
    gen = torch.Generator().manual_seed(E)
    x = torch.randn(Rn, B, S, E, generator=gen)
    w = torch.rand(Rn, E, generator=gen) + 0.5
    b = torch.randn(Rn, E, generator=gen)
    g = torch.randn(Rn, B, S, E, generator=gen)
    _ln_check('x'.join(map(str, shape)), x, w, b, g, io_name)


@needs_gpu
@pytest.mark.parametrize('mean', [10.0, 100.0])
def test_layernorm_conditioning(mean):
    """Rows with mean/std of 10 and 100: the variance must not be taken as
    E[x^2] - mu^2 in fp32, which loses mean^2 * 2^-24 absolute.  With that
    formula the kernel missed this test on an MI355X: y off by 4.7e-5 at 10
    and 4.8e-3 at 100 (tolerances 3.0e-5 and 2.0e-4; torch's fp32 error is
    1.9e-6 and 1.3e-5), dx and dgamma alike.  ln_fwd_kernel now takes the
    variance from sum (x - mu)^2 after the mean pass: 1.7e-6 and 9.7e-6."""
    Rn, B, S, E = 2, 2, 8, 256
    gen = torch.Generator().manual_seed(int(mean))
    x = torch.randn(Rn, B, S, E, generator=gen) + mean
    w = torch.rand(Rn, E, generator=gen) + 0.5
    b = torch.randn(Rn, E, generator=gen)
    g = torch.randn(Rn, B, S, E, generator=gen)
    _ln_check('mean{:g}'.format(mean), x, w, b, g, 'fp32')


@needs_gpu
def test_layernorm_rejects_wide_rows():
    from heterofl_amd.ops.fused import fused_layernorm
    x = torch.randn(1, 1, 2, 1025, device=DEV)
    w = torch.ones(1, 1025, device=DEV)
    with pytest.raises(RuntimeError):
        fused_layernorm(x, w, torch.zeros_like(w), 1)


# ==================================================================== lm_ce
@needs_gpu
@pytest.mark.parametrize('scale', [1.0, 20.0])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('shape', [(4, 2, 16, 1000), (2, 1, 3, 37),
                                   (3, 5, 26, 300), (1, 1, 1, 2049)])
def test_lm_ce_matches_fp64(shape, io_name, masked, scale):
    """Vocab-masked CE with a distinct upstream gradient per client, so that
    a backward that reads up[0] for everyone cannot pass.  At logit scale 20
    the backward used to compute exp(v - lse) from the saved fp32 lse =
    max + log(sum); with |max| ~ 64 that sum drops 4e-6 of log(sum), and
    dlogits missed the fp32 tolerance at (2, 1, 3, 37) by 1.04e-6 and
    1.14e-6 against 1e-6.  lm_ce_bwd_kernel now gets max and log(sum) apart
    and the largest fp32 error is 4.4e-8."""
    from heterofl_amd.ops.fused import fused_lm_ce
    Rn, B, S, V = shape
    io = R.IO_DTYPES[io_name]
    gen = torch.Generator().manual_seed(V + int(scale))
    logits = (torch.randn(Rn, B, S, V, generator=gen) * scale).to(io)
    tokens = torch.randint(0, V, (Rn, B, S), generator=gen)
    tokens.view(Rn, -1)[:, 0] = 0
    tokens.view(Rn, -1)[:, -1] = V - 1
    mask = (torch.rand(Rn, V, generator=gen) > 0.2).float() if masked \
        else None
    w = torch.rand(Rn, generator=gen) + 0.25 + torch.arange(Rn)
    lg = logits.to(DEV).requires_grad_(True)
    losses = fused_lm_ce(lg, tokens.to(DEV),
                         mask.to(DEV) if masked else None, Rn)
    (losses * w.to(DEV)).sum().backward()
    got_l, got_d = losses.detach().cpu(), lg.grad.cpu()
    ref = R.lm_ce_ref(logits, tokens, mask, w, dtype=torch.float64)
    r32 = R.lm_ce_ref(logits.float(), tokens, mask, w, dtype=torch.float32)
    tag = '{}-{}-{}-s{:g}'.format('x'.join(map(str, shape)), io_name,
                                  'mask' if masked else 'nomask', scale)
    tol_l = max(16 * R.max_abs(r32['losses'], ref['losses']), 1e-6)
    err_l = R.max_abs(got_l, ref['losses'])
    _report('lm_ce', tag, 'losses', err_l, tol_l)
    tol_d = max(16 * R.max_abs(r32['dlogits'], ref['dlogits']), 1e-6)
    err = (got_d.double() - ref['dlogits']).abs()
    if io_name == 'bf16':
        # one bf16 ulp of the reference value; values under the smallest
        # normal number may be flushed to zero
        err_d = (err - R.bf16_ulp(ref['dlogits']) - 2.0 ** -126) \
            .clamp_min(0).max().item()
        tol_d = 0.0
    else:
        err_d = err.max().item()
    _report('lm_ce', tag, 'dlogits', err_d, tol_d)
    assert _finite(got_l) and _finite(got_d)
    assert err_l <= tol_l, (tag, err_l, tol_l)
    assert err_d <= tol_d, (tag, err_d, tol_d)
    if masked:
        dead = (mask == 0).view(Rn, 1, 1, V).expand(Rn, B, S, V)
        assert bool((got_d[dead] == 0).all()), tag


# ============================================================= dropout glue
def _glue_close(tag, name, got, ref, io_name):
    """fp32: 1e-5 (1 + |ref|); bf16: one bf16 ulp of ref on top of that."""
    tol = 1e-5 * (1 + ref.abs())
    if io_name == 'bf16':
        tol = tol + R.bf16_ulp(ref)
    excess = ((got.double() - ref).abs() / tol).max().item()
    _report('glue', tag + '-' + io_name, name, excess, 1.0)
    assert excess <= 1.0, (tag, io_name, name, excess)


def _gelu_drop_case(tag, n, p, io_name, dev_ref=False):
    from heterofl_amd.ops.fused import fused_gelu_dropout
    io = R.IO_DTYPES[io_name]
    rate = 0.5
    gen = torch.Generator().manual_seed(n + int(100 * p))
    x = torch.randn(n, generator=gen).to(io).to(DEV).requires_grad_(True)
    dy = torch.randn(n, generator=gen).to(io).to(DEV)
    y = fused_gelu_dropout(x, rate, p)
    (dx,) = torch.autograd.grad(y, x, dy)
    t = (lambda a: a.detach()) if dev_ref else (lambda a: a.detach().cpu())
    x, dy, y, dx = t(x), t(dy), t(y), t(dx)
    # fp32 erf saturates at -1 below x/rate ~ -5.6, where a kept y is -0;
    # its derivative is still non-zero there
    keep = (y != 0) | (dx != 0)
    ok = (x != 0) & (dy != 0)
    assert bool(((y == 0) | (dx != 0))[ok].all()), tag
    frac = keep[ok].double().mean().item()
    sigma = math.sqrt(p * (1 - p) / int(ok.sum()))
    _report('glue', tag + '-' + io_name, 'gelu.keepfrac',
            abs(frac - (1 - p)), 6 * sigma)
    assert abs(frac - (1 - p)) <= 6 * sigma, (tag, frac)
    ref = R.gelu_drop_ref(x, keep, dy, rate, p)
    _glue_close(tag, 'gelu.y', y[ok], ref['y'][ok], io_name)
    _glue_close(tag, 'gelu.dx', dx[ok], ref['dx'][ok], io_name)
    assert bool((dx[~keep] == 0).all()) and bool((y[~keep] == 0).all())


def _res_drop_case(tag, n, p, io_name, dev_ref=False):
    from heterofl_amd.ops.fused import fused_res_dropout
    io = R.IO_DTYPES[io_name]
    rate = 0.5
    gen = torch.Generator().manual_seed(n + int(100 * p) + 1)
    src = torch.randn(n, generator=gen).to(io).to(DEV).requires_grad_(True)
    h = torch.randn(n, generator=gen).to(io).to(DEV).requires_grad_(True)
    dt = torch.randn(n, generator=gen).to(io).to(DEV)
    out = fused_res_dropout(src, h, rate, p)
    dsrc, dh = torch.autograd.grad(out, (src, h), dt)
    t = (lambda a: a.detach()) if dev_ref else (lambda a: a.detach().cpu())
    src, h, dt, out, dsrc, dh = (t(a) for a in (src, h, dt, out, dsrc, dh))
    ok = dt != 0
    keep = dh != 0                  # dh = dt * keep / (rate (1 - p))
    frac = keep[ok].double().mean().item()
    sigma = math.sqrt(p * (1 - p) / int(ok.sum()))
    _report('glue', tag + '-' + io_name, 'res.keepfrac',
            abs(frac - (1 - p)), 6 * sigma)
    assert abs(frac - (1 - p)) <= 6 * sigma, (tag, frac)
    ref = R.res_drop_ref(src, h, keep, dt, rate, p)
    _glue_close(tag, 'res.t', out[ok], ref['t'][ok], io_name)
    _glue_close(tag, 'res.dh', dh[ok], ref['dh'][ok], io_name)
    assert torch.equal(dsrc, dt), tag
    # a dropped position passes src through untouched
    assert torch.equal(out[ok & ~keep], src[ok & ~keep]), tag


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_glue_kept_values(p, io_name):
    """The 1/(1-p) scale on kept values, forward and backward, with the keep
    mask read back from the outputs."""
    n = 4 * 3 * 64 * 128 + 5
    _gelu_drop_case('p{}'.format(p), n, p, io_name)
    _res_drop_case('p{}'.format(p), n, p, io_name)


@needs_gpu
def test_dropout_glue_grid_stride():
    """More elements than 4096 blocks x 256 threads x 8: the grid-stride
    loop of every elementwise kernel runs more than once."""
    n = 4096 * 2048 + 777
    _gelu_drop_case('stride', n, 0.1, 'fp32', dev_ref=True)
    _res_drop_case('stride', n, 0.1, 'fp32', dev_ref=True)


@needs_gpu
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_mask_statistics(p):
    """Keep fraction, lag-1 agreement of neighbouring indices and agreement
    of two sites of one step (different salts), each within 6 sigma.  The
    agreement of two Bernoulli(1-p) bits is a = p^2 + (1-p)^2.  Neighbouring
    pairs share a bit, so their indicators are 1-dependent:
    var(mean) <= (a(1-a) + 2 a(1-a)) / n."""
    from heterofl_amd.ops.fused import fused_gelu_dropout
    n = 200_000
    x = torch.randn(n, generator=torch.Generator().manual_seed(7)).to(DEV)
    x = torch.where(x == 0, torch.ones_like(x), x)
    m1 = (fused_gelu_dropout(x, 1.0, p) != 0).cpu()
    m2 = (fused_gelu_dropout(x, 1.0, p) != 0).cpu()
    a = p * p + (1 - p) * (1 - p)
    for name, got, want, sigma in [
            ('keep1', m1.double().mean().item(), 1 - p,
             math.sqrt(p * (1 - p) / n)),
            ('keep2', m2.double().mean().item(), 1 - p,
             math.sqrt(p * (1 - p) / n)),
            ('lag1', (m1[1:] == m1[:-1]).double().mean().item(), a,
             math.sqrt(3 * a * (1 - a) / (n - 1))),
            ('sites', (m1 == m2).double().mean().item(), a,
             math.sqrt(a * (1 - a) / n))]:
        _report('glue', 'stats-p{}'.format(p), name, abs(got - want),
                6 * sigma)
        assert abs(got - want) <= 6 * sigma, (name, got, want)


@needs_gpu
def test_token_mask_rates():
    from heterofl_amd.ops.fused import fused_token_mask
    n = 200_000
    toks = torch.randint(0, 1000, (10, 100, 200),
                         generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(fused_token_mask(toks, 0.0, 1000), toks)
    out = fused_token_mask(toks, 0.15, 1000)
    masked = out == 1000
    frac = masked.double().mean().item()
    sigma = math.sqrt(0.15 * 0.85 / n)
    _report('glue', 'token_mask', 'frac', abs(frac - 0.15), 6 * sigma)
    assert abs(frac - 0.15) <= 6 * sigma, frac
    assert torch.equal(out[~masked], toks[~masked])


# ================================================================ embed_pos
@needs_gpu
@pytest.mark.parametrize('shadows', [False, True])
@pytest.mark.parametrize('shape', [(3, 2, 64, 96, 300, 64),
                                   (2, 1, 5, 16, 50, 9),
                                   (1, 2, 3, 1024, 7, 3),
                                   (1, 1, 8, 16, 20000, 8)])
def test_embed_pos_matches_fp64(shape, shadows):
    """Gather + positional add + Scaler and both table gradients, fp32 and
    bf16-shadow routes, for random, all-identical and {0, V-1}-only ids.
    rate = 0.5 multiplies exactly, so the fp32 forward is one rounding of
    (a + b) away from fp64: half an fp32 ulp, 2^-24 |ref|."""
    from heterofl_amd.ops.fused import fused_embed_pos
    Rn, B, S, E, V, P = shape
    rate = 0.5
    gen = torch.Generator().manual_seed(V)
    table = torch.randn(Rn, V, E, generator=gen)
    pos = torch.randn(Rn, P, E, generator=gen)
    dy = torch.randn(Rn, B, S, E, generator=gen)
    patterns = {
        'random': torch.randint(0, V, (Rn, B, S), generator=gen),
        'same': torch.full((Rn, B, S), V // 2),
        'ends': torch.randint(0, 2, (Rn, B, S), generator=gen) * (V - 1)}
    tag0 = 'x'.join(map(str, shape)) + ('-bf16' if shadows else '-fp32')
    for pname, ids in patterns.items():
        tag = tag0 + '-' + pname
        tg = table.to(DEV).requires_grad_(True)
        pg = pos.to(DEV).requires_grad_(True)
        t16 = tg.detach().to(torch.bfloat16) if shadows else None
        p16 = pg.detach().to(torch.bfloat16) if shadows else None
        y = fused_embed_pos(ids.to(DEV), tg, pg, t16, p16, rate)
        g = dy.to(y.dtype)
        dtab, dpos = torch.autograd.grad(y, (tg, pg), g.to(DEV))
        assert y.dtype == (torch.bfloat16 if shadows else torch.float32)
        assert dtab.dtype == dpos.dtype == torch.float32
        t_eff = R.bf16r(table) if shadows else table
        p_eff = R.bf16r(pos) if shadows else pos
        ref = R.embed_pos_ref(ids, t_eff, p_eff, g, rate)
        r32 = R.embed_pos_ref(ids, t_eff, p_eff, g, rate,
                              dtype=torch.float32)
        err = (y.cpu().double() - ref['out']).abs()
        unit = R.bf16_ulp(ref['out']) if shadows \
            else 2.0 ** -24 * ref['out'].abs()
        excess = (err - unit).max().item()
        _report('embed', tag, 'out.excess', excess, 0.0)
        assert excess <= 0, (tag, excess)
        for name, got in (('dtable', dtab.cpu()), ('dpos', dpos.cpu())):
            tol = 16 * R.max_abs(r32[name], ref[name])
            e = R.max_abs(got, ref[name])
            _report('embed', tag, name, e, tol)
            assert e <= tol, (tag, name, e, tol)
        hit = torch.zeros(Rn, V, dtype=torch.bool)
        hit[torch.arange(Rn).view(Rn, 1, 1).expand_as(ids), ids] = True
        assert bool((dtab.cpu()[~hit] == 0).all()), tag
        assert bool((dpos.cpu()[:, S:] == 0).all()), tag


@needs_gpu
def test_embed_pos_rejects_wide_rows():
    from heterofl_amd.ops.fused import fused_embed_pos
    table = torch.randn(1, 3, 1025, device=DEV)
    pos = torch.randn(1, 2, 1025, device=DEV)
    ids = torch.zeros(1, 1, 2, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        fused_embed_pos(ids, table, pos, None, None, 1.0)
