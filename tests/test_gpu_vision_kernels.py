"""GPU tests of the vision training kernels (fused_norm.hip, masked_ce.hip,
head.hip, clip_sgd.hip) at edge shapes against the fp64 references of
tests/vision_refs.py.  Every case runs forward and backward with a random
upstream gradient, in fp32 and in bf16 io where the kernel has both; BN and
clip+SGD run with HETEROFL_STREAM_VEC on and off.  Every test prints
`VK <kernel> <case> <output> err= bound=` lines before it asserts (pytest -s
shows them).  Run with: pytest tests -m gpu

What each tolerance rests on
----------------------------
fp32 outputs (every kernel): max |got - ref64| <= 16 x max |ref32 - ref64|,
the same reference run in fp32 and in fp64 on the same input inside the test
(vision_refs.fp32_tol), at least 2^-23 max|ref64|.  The 16 is the factor of
tests/test_gpu_lm_kernels.py.  For BN / GN the reference runs one_pass=True:
the variance as E[x^2] - mean^2, and for BN the affine folded into x * scale
+ shift, as in the kernels; both lose precision with mean / sigma of the
data, so the yardstick has to lose it too.
bf16 outputs (y, dx of BN / GN, dfeat of the head): half a bf16 ulp of the
fp64 reference value is taken off each element's error first.
Largest fp32-vs-fp64 spread of the references over the case lists (printed by
tests/test_vision_refs.py, which also checks every fp64 reference against
torch's own fp64 ops to 1e-12):

    kernel  output   max abs   rel Frobenius  set by
    bn      y        1.4e-05   2.8e-06        special (mean = +-8 sigma)
    bn      mean     3.1e-06   2.9e-08        special (sigma = 1e3)
    bn      invstd   1.3e-05   4.2e-08        m1 (invstd = eps^-1/2 = 316)
    bn      dx       1.3e-04   8.4e-08        special (|dx| up to 1e3)
    bn      dgamma   1.4e-04   2.1e-07        split3 (66560 terms)
    bn      dbeta    2.3e-04   1.7e-07        split3
    gn      y        9.1e-07   6.1e-08        gn20
    gn      invstd   1.3e-05   4.2e-08        m1
    gn      dx       7.4e-07   7.5e-08        gn20
    gn      dgamma   9.2e-06   8.1e-08        big33
    gn      dbeta    1.1e-05   9.9e-08        big33
    ce      losses   4.4e-06   4.7e-08        130x2x100, scores x 30
    ce      dscores  3.8e-08   4.3e-08        10x5x10
    head    scores   1.0e-06   1.3e-07        37x2x512x2x2x100
    head    pooled   1.5e-07   4.0e-08        "
    head    dfeat    2.2e-07   1.8e-07        "
    head    dw       3.9e-06   1.1e-07        "
    head    db       2.7e-06   8.4e-08        "
    sgd     param    2.8e-07   (max|p| 4.7)   step 2
    sgd     buf      3.4e-09   (max|b| 0.04)  step 2

(an ordinary case sits at 5e-8 .. 1e-7 relative: p4 has y 2.7e-7, dx 4.2e-7,
dgamma 2.6e-6 at max|dgamma| = 20.)

ReLU boundary.  The BN forward stores relu(x * scale + shift), the backward
rebuilds the mask from (x - mean) * invstd * g + b > 0, and the reference
decides in fp64: an element whose pre-activation lies within rounding of 0
may fall on either side, and a flipped mask moves dx by the whole of
invstd * g * dy.  Every BN / GN case therefore has a seed for which no
element lies within tau = 16 x spread(pre) (at least 2^-23 max|pre|, about
1e-6 .. 2e-5) of 0; test_vision_refs.py asserts it for every variant.
split3 (8.5 M elements) is the exception: its 92 (fp32) / 63 (bf16) such
elements, a share of 1.1e-5 / 7.4e-6 <= 1e-4, are left out of the y / dx
comparison, and dgamma, dbeta and dx get what flipping them can change at
most added to their tolerance: sum |dy xhat| and sum |dy| over the excluded
elements of the channel (vision_refs.bn_flip_slack).  Elements with pre = 0
exactly (an all-zero or constant channel without affine) are on the false
side in the reference and in both kernels' masks.  m1 without affine is not a
variant, see vision_refs.BN_VARIANTS.

masked CE adds what __expf and __logf may add to correctly rounded fp32,
from the documented accuracy of the instructions they compile to (V_EXP_F32
and V_LOG_F32: base 2, 1 ulp): (1 + |v - max|) 2^-22 relative per
exponential, 2^-22 |log sum| for the logarithm, propagated through the
softmax elementwise; the derivation is the docstring of
vision_refs.masked_ce_intrinsic_slack.  Nothing in it is sized from what the
kernel produces.  It comes to at most 1.3e-6 on a sample's NLL and 4.6e-7 on
a dscores element over the case list.
correct, count, the zero gradient of masked classes: exact (scores without
ties among live classes).
bf16 shadows of clip+SGD equal param.to(bfloat16) of the kernel's own fp32
result bit for bit; GraphClipSGD.bind + launch equals FusedClipSGD.step on
clones bit for bit.

Largest err / bound seen on an MI355X, fp32 (bf16 in brackets): bn 0.41
(0.34) dbeta of n10; gn 0.41 (0.43) dbeta of big17; ce 0.26 losses of
130x2x100 x 30; head 0.82 (0.47) scores of 10x5x512x4x4x10, whose kernel
sums 512 products one after the other where torch's blocked sum sets the
yardstick; sgd 0.06.

What this suite found.  GroupNorm with one element per group (`in` on 1x1
planes): the compiler contracted s2 / M - mean * mean into one fma, which
keeps the rounding residual of mean^2, up to 6e-8 x^2 against eps = 1e-5, and
d * g - k1 likewise: invstd came out 0.203 off 316.2 (bound 2.1e-4) and dx
1.8e-5 where it is exactly 0.  gn_relu_fwd_kernel / gn_relu_bwd_kernel now
round those products on their own; invstd is 1.7e-5 off, dx is 0.
"""
import contextlib
import math
import os

import pytest
import torch

from tests import vision_refs as V

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

DEV = 'cuda:0'
IOS = list(V.IO_DTYPES)
F64, F32 = torch.float64, torch.float32
NONE = torch.Tensor()


@contextlib.contextmanager
def stream_vec(on):
    prev = os.environ.get('HETEROFL_STREAM_VEC')
    os.environ['HETEROFL_STREAM_VEC'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_STREAM_VEC']
        else:
            os.environ['HETEROFL_STREAM_VEC'] = prev


def ext():
    from heterofl_amd.ops import require_native
    return require_native()


def _report(kernel, case, name, err, bound):
    print('VK {} {} {} err={:.3e} bound={:.3e}'.format(kernel, case, name,
                                                       err, bound))


def _dev(t):
    return NONE if t is None else t.to(DEV)


def _excess(got, ref, io_name=None, slack=None, keep=None):
    """max |got - ref| after taking off what is allowed elementwise: half a
    bf16 ulp of the reference for a bf16 output, `slack`; over `keep`."""
    err = (got.double() - ref.double()).abs()
    if io_name == 'bf16':
        err = err - V.bf16_ulp(ref) / 2
    if slack is not None:
        err = err - slack
    if keep is not None:
        err = err[keep]
    if err.numel() == 0:
        return 0.0
    return err.clamp_min(0).max().item()


def _judge(kernel, cid, rows):
    """rows: (name, err, bound).  Print all, then fail on any."""
    fails = []
    for name, err, bound in rows:
        _report(kernel, cid, name, err, bound)
        if not (math.isfinite(err) and err <= bound):
            fails.append((name, err, bound))
    assert not fails, (kernel, cid, fails)


# =================================================================== BN+ReLU
_BN_REFS = {}


def _bn_refs(case, io_name, affine):
    """(inputs on DEV, r64, r32, excluded set or None, flip slack), computed
    once per (case, io, affine) and never written to.  split3 is computed on
    the device: 8.5 M elements."""
    key = (case, io_name, affine)
    if key not in _BN_REFS:
        x, dy, w, b = V.bn_inputs(case, io_name, affine)
        where = DEV if case == 'split3' else 'cpu'
        args = [None if t is None else t.to(where) for t in (x, w, b, dy)]
        r64 = V.bn_relu(*args, dtype=F64)
        r32 = V.bn_relu(*args, dtype=F32)
        near, slack = None, None
        if case == 'split3':
            tau = V.boundary_tau(r32.pre, r64.pre)
            near = V.relu_boundary(r64.pre, tau) & (r64.pre != 0)
            assert near.double().mean().item() <= V.SPLIT3_MAX_SHARE
            slack = V.bn_flip_slack(args[0], args[1], args[3], r64, near)
        if case == 'split3':
            # a few hundred MB on the device: keep one variant at a time
            for k in [k for k in _BN_REFS if k[0] == 'split3']:
                del _BN_REFS[k]
        _BN_REFS[key] = (tuple(_dev(t) for t in (x, dy, w, b)), r64, r32,
                         near, slack)
    return _BN_REFS[key]


def _norm_rows(got, r64, r32, io_name, near=None, slack=None):
    rows = []
    for name in V.NORM_OUTPUTS:
        ref, lo = getattr(r64, name), getattr(r32, name)
        g = got[name].to(ref.device)
        tol = V.fp32_tol(lo, ref)
        io = io_name if name in ('y', 'dx') else None
        sl, keep = None, None
        if near is not None:
            keep = ~near if name in ('y', 'dx') else None
            sl = {'dgamma': slack[0], 'dbeta': slack[1],
                  'dx': slack[2]}.get(name)
        rows.append((name, _excess(g, ref, io, sl, keep), tol))
    return rows


def _bn_kernels(x, dy, w, b):
    e = ext()
    y, mean, invstd = e.bn_relu_fwd(x, w, b, V.EPS)
    dx, dgamma, dbeta = e.bn_relu_bwd(dy, x, w, b, mean, invstd)
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, dx=dx, dgamma=dgamma,
                dbeta=dbeta)


def _expect_routes(case, io_name, vec, aligned=True):
    from heterofl_amd.ops.fused import bn_relu_route
    (N, C, H, W), _, routes = V.BN_CASES[case]
    esz = 4 if io_name == 'fp32' else 2
    want = [r if (vec and aligned) or r != 'vec' else 'staged'
            for r in routes[io_name]]
    with stream_vec(vec):
        have = [bn_relu_route(d, N, C, H * W, esz, aligned)
                for d in ('fwd', 'bwd')]
    assert have == want, (case, io_name, vec, have, want)


@needs_gpu
@pytest.mark.parametrize('vec', [True, False], ids=['vec', 'novec'])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('variant', V.BN_VARIANTS,
                         ids=[V.bn_variant_id(v) for v in V.BN_VARIANTS])
def test_bn_relu_matches_fp64(variant, io_name, vec):
    case, affine = variant
    _expect_routes(case, io_name, vec)
    (x, dy, w, b), r64, r32, near, slack = _bn_refs(case, io_name, affine)
    assert x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    with stream_vec(vec):
        got = _bn_kernels(x, dy, w, b)
    cid = '{}-{}-{}'.format(V.bn_variant_id(variant), io_name,
                            'vec' if vec else 'novec')
    assert got['y'].dtype == x.dtype and got['dx'].dtype == x.dtype
    _judge('bn', cid, _norm_rows(got, r64, r32, io_name, near, slack))
    if x.numel() == x.size(1):
        # one value per channel: nothing to normalise, no gradient to x
        assert bool((got['dx'] == 0).all()) and bool((got['dgamma'] == 0).all())
    if case == 'special':
        # the all-zero and the constant channel come out of the statistics
        # exactly
        assert got['mean'][:2].tolist() == [0.0, 0.5]


@needs_gpu
@pytest.mark.parametrize('vec', [True, False], ids=['vec', 'novec'])
@pytest.mark.parametrize('io_name', IOS)
def test_bn_relu_offset_view(io_name, vec):
    """x starts 4 bytes into its buffer: no 16-byte rows, the staged kernel
    whatever HETEROFL_STREAM_VEC says."""
    case = 'e192'
    _expect_routes(case, io_name, vec, aligned=False)
    (x, dy, w, b), r64, r32, _, _ = _bn_refs(case, io_name, True)
    skip = 4 // x.element_size()
    flat = torch.empty(x.numel() + skip, dtype=x.dtype, device=DEV)
    xo = flat[skip:].view(x.shape)
    xo.copy_(x)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4
    with stream_vec(vec):
        got = _bn_kernels(xo, dy, w, b)
    _judge('bn', 'e192-offset4-{}-{}'.format(io_name,
                                             'vec' if vec else 'novec'),
           _norm_rows(got, r64, r32, io_name))


def _expanded_dy(dy):
    """dy's first plane element repeated over the plane: a stride-0 view on
    the device, and the same values materialised on the CPU."""
    view = dy.to(DEV)[:, :, :1, :1].expand(dy.shape)
    assert not view.is_contiguous()
    return view, dy[:, :, :1, :1].expand(dy.shape).contiguous()


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
def test_bn_relu_noncontiguous_dy(io_name):
    from heterofl_amd.ops.fused import fused_norm_relu
    x, dy, w, b = V.bn_inputs('hw24', io_name, True)
    view, full = _expanded_dy(dy)
    r64 = V.bn_relu(x, w, b, full, dtype=F64)
    r32 = V.bn_relu(x, w, b, full, dtype=F32)
    xg = x.to(DEV).requires_grad_(True)
    wg, bg = (t.to(DEV).requires_grad_(True) for t in (w, b))
    y = fused_norm_relu(xg, wg, bg, 'bn')
    dx, dg, db = torch.autograd.grad(y, (xg, wg, bg), view)
    rows = []
    for name, g in (('y', y.detach()), ('dx', dx), ('dgamma', dg),
                    ('dbeta', db)):
        ref = getattr(r64, name)
        rows.append((name, _excess(g.cpu(), ref,
                                   io_name if name in ('y', 'dx') else None),
                     V.fp32_tol(getattr(r32, name), ref)))
    _judge('bn', 'hw24-expanded-dy-' + io_name, rows)


# =================================================================== GN+ReLU
@needs_gpu
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', list(V.GN_CASES))
def test_gn_relu_matches_fp64(case, io_name, affine):
    # the launcher has no route query for GN; the case list pins the byte
    # count its `gsb <= 64 KB` test sees
    assert V.gn_unstaged(case, io_name) == {
        ('big17', 'fp32'): True, ('big33', 'fp32'): True,
        ('big33', 'bf16'): True}.get((case, io_name), False)
    x, dy, w, b, G = V.gn_inputs(case, io_name, affine)
    r64 = V.gn_relu(x, w, b, dy, G, dtype=F64)
    r32 = V.gn_relu(x, w, b, dy, G, dtype=F32)
    e = ext()
    xd, dyd, wd, bd = (_dev(t) for t in (x, dy, w, b))
    y, mean, invstd = e.gn_relu_fwd(xd, wd, bd, G, V.EPS)
    dx, dgamma, dbeta = e.gn_relu_bwd(dyd, xd, wd, bd, mean, invstd, G)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in dict(
        y=y, mean=mean, invstd=invstd, dx=dx, dgamma=dgamma,
        dbeta=dbeta).items()}
    assert got['y'].dtype == x.dtype and got['dx'].dtype == x.dtype
    assert got['mean'].shape == (x.size(0) * G,)
    _judge('gn', '{}-{}-{}'.format(case, io_name,
                                   'affine' if affine else 'plain'),
           _norm_rows(got, r64, r32, io_name))


@needs_gpu
@pytest.mark.parametrize('io_name', IOS)
def test_gn_relu_noncontiguous_dy(io_name):
    from heterofl_amd.ops.fused import fused_norm_relu
    x, dy, w, b, G = V.gn_inputs('ln', io_name, True)
    view, full = _expanded_dy(dy)
    r64 = V.gn_relu(x, w, b, full, G, dtype=F64)
    r32 = V.gn_relu(x, w, b, full, G, dtype=F32)
    xg = x.to(DEV).requires_grad_(True)
    wg, bg = (t.to(DEV).requires_grad_(True) for t in (w, b))
    y = fused_norm_relu(xg, wg, bg, 'gn', G)
    dx, dg, db = torch.autograd.grad(y, (xg, wg, bg), view)
    rows = []
    for name, g in (('y', y.detach()), ('dx', dx), ('dgamma', dg),
                    ('dbeta', db)):
        ref = getattr(r64, name)
        rows.append((name, _excess(g.cpu(), ref,
                                   io_name if name in ('y', 'dx') else None),
                     V.fp32_tol(getattr(r32, name), ref)))
    _judge('gn', 'ln-expanded-dy-' + io_name, rows)


@needs_gpu
def test_gn_relu_rejects_bad_grouping():
    x = torch.randn(2, 6, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match='divisible'):
        ext().gn_relu_fwd(x, NONE, NONE, 4, V.EPS)


# ================================================================= masked CE
@needs_gpu
@pytest.mark.parametrize('case', V.CE_CASES,
                         ids=[V.ce_case_id(c) for c in V.CE_CASES])
def test_masked_ce_matches_fp64(case):
    """Two calls into one metrics buffer; the backward goes through
    (losses * weights).sum() with a distinct weight per client."""
    from heterofl_amd.ops.fused import fused_masked_ce
    (N, R, C), variant, _ = case
    cid = V.ce_case_id(case)
    metrics = torch.zeros(R, 3, device=DEV)
    m64 = torch.zeros(R, 3, dtype=F64)
    m32 = torch.zeros(R, 3, dtype=F32)
    m_slack = torch.zeros(R, dtype=F64)
    rows = []
    for call in range(2):
        scores, labels, mask, up = V.ce_inputs(case, call)
        r64 = V.masked_ce(scores, labels, mask, up, dtype=F64)
        r32 = V.masked_ce(scores, labels, mask, up, dtype=F32)
        nll_slack, d_slack = V.masked_ce_intrinsic_slack(scores, labels,
                                                         mask, up)
        sg = scores.to(DEV).requires_grad_(True)
        losses = fused_masked_ce(sg, labels.to(DEV),
                                 None if mask is None else mask.to(DEV),
                                 metrics)
        (losses * up.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        got_l, got_d = losses.detach().cpu(), sg.grad.cpu()
        rows.append(('losses.{}'.format(call),
                     _excess(got_l, r64.losses, slack=nll_slack.mean(0)),
                     V.fp32_tol(r32.losses, r64.losses)))
        rows.append(('dscores.{}'.format(call),
                     _excess(got_d, r64.dscores, slack=d_slack),
                     V.fp32_tol(r32.dscores, r64.dscores)))
        if mask is not None:
            dead = (mask == 0).unsqueeze(0).expand(N, R, C)
            assert bool((got_d[dead] == 0).all()), cid
        m64 += r64.metrics
        m32 += r32.metrics
        m_slack += nll_slack.sum(0)
    got_m = metrics.cpu()
    rows.append(('metrics.sum_nll',
                 _excess(got_m[:, 0], m64[:, 0], slack=m_slack),
                 V.fp32_tol(m32[:, 0], m64[:, 0])))
    _judge('ce', cid, rows)
    assert torch.equal(got_m[:, 1].double(), m64[:, 1]), cid
    assert torch.equal(got_m[:, 2].double(), m64[:, 2]), cid
    assert bool((got_m[:, 2] == 2 * N).all())


@needs_gpu
def test_masked_ce_without_metrics():
    from heterofl_amd.ops.fused import fused_masked_ce
    case = ((65, 3, 10), 'random', 1.0)
    scores, labels, mask, up = V.ce_inputs(case)
    r64 = V.masked_ce(scores, labels, mask, up, dtype=F64)
    r32 = V.masked_ce(scores, labels, mask, up, dtype=F32)
    nll_slack, _ = V.masked_ce_intrinsic_slack(scores, labels, mask, up)
    losses = fused_masked_ce(scores.to(DEV), labels.to(DEV), mask.to(DEV))
    _judge('ce', V.ce_case_id(case) + '-nometrics',
           [('losses', _excess(losses.cpu(), r64.losses,
                               slack=nll_slack.mean(0)),
             V.fp32_tol(r32.losses, r64.losses))])


# ====================================================================== head
@needs_gpu
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('io_name', IOS)
@pytest.mark.parametrize('case', V.HEAD_CASES,
                         ids=[V.head_case_id(c) for c in V.HEAD_CASES])
def test_head_matches_fp64(case, io_name, bias):
    from heterofl_amd.ops.fused import fused_head
    N, R, C, H, W, J = case
    feat, w, b, ds = V.head_inputs(case, io_name, bias)
    r64 = V.head(feat, w, b, ds, R, dtype=F64)
    r32 = V.head(feat, w, b, ds, R, dtype=F32)
    fg = feat.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if bias else None
    scores = fused_head(fg, wg, bg, R)
    leaves = (fg, wg, bg) if bias else (fg, wg)
    grads = torch.autograd.grad(scores, leaves, ds.to(DEV))
    _, pooled = ext().head_fwd(fg.detach(), wg.detach(),
                               bg.detach() if bias else NONE, R)
    torch.cuda.synchronize()
    assert grads[0].dtype == feat.dtype and scores.dtype == torch.float32
    got = dict(scores=scores.detach(), pooled=pooled, dfeat=grads[0],
               dw=grads[1])
    if bias:
        got['db'] = grads[2]
    rows = []
    for name, g in got.items():
        ref = getattr(r64, name)
        io = io_name if name == 'dfeat' else None
        rows.append((name, _excess(g.cpu(), ref, io),
                     V.fp32_tol(getattr(r32, name), ref)))
    _judge('head', '{}-{}-{}'.format(V.head_case_id(case), io_name,
                                     'bias' if bias else 'nobias'), rows)


@needs_gpu
def test_head_bwd_rejects_oversized_stage():
    """N * J * 4 bytes over the 64 KB LDS stage: the check precedes the
    launch, nothing runs on the device."""
    N, R, C, H, W, J = V.HEAD_LDS_CASE
    feat, w, b, ds = V.head_inputs(V.HEAD_LDS_CASE, 'fp32')
    e = ext()
    scores, pooled = e.head_fwd(feat.to(DEV), w.to(DEV), b.to(DEV), R)
    r64 = V.head(feat, w, b, ds, R, dtype=F64)
    r32 = V.head(feat, w, b, ds, R, dtype=F32)
    _judge('head', V.head_case_id(V.HEAD_LDS_CASE) + '-fwd',
           [('scores', _excess(scores.cpu(), r64.scores),
             V.fp32_tol(r32.scores, r64.scores))])
    with pytest.raises(RuntimeError, match='LDS'):
        e.head_bwd(ds.to(DEV), pooled, w.to(DEV), R, H, W, False, True)
    torch.cuda.synchronize()


# ================================================================== clip+SGD
def _sgd_device_state():
    params, grads, bufs = V.sgd_inputs()
    dp = [p.to(DEV) for p in params]
    db = [b.to(DEV) for b in bufs]
    cur = [torch.zeros_like(p) for p in dp]
    shadows = []
    for i, p in enumerate(dp):
        kind = V.SGD_SHADOWS.get(i)
        if kind is None:
            shadows.append(None)
        elif kind == 'aligned':
            shadows.append(p.to(torch.bfloat16))
            assert shadows[-1].data_ptr() % 8 == 0
        else:
            flat = torch.zeros(p.numel() + 1, dtype=torch.bfloat16,
                               device=DEV)
            sh = flat[1:]
            sh.copy_(p)
            # 2 bytes off an aligned base: no 8-byte shadow stores, the
            # scalar loop for every chunk of this tensor
            assert sh.is_contiguous() and sh.data_ptr() % 8 == 2
            shadows.append(sh)
    return dp, grads, db, cur, shadows


class _Table1024:
    """ext.build_chunk_table with chunk_elems = 1024: multi-chunk slices and
    ragged last chunks (4100 = 4 x 1024 + 4, 4099 = ... + 3) at tiny sizes."""

    def __init__(self, params, grads, bufs, R, shadows):
        e = ext()
        self.keep = (params, grads, bufs, shadows)
        self.table, n, self.chunk_client = e.build_chunk_table(
            grads, params, bufs, R, 1024,
            [NONE if s is None else s for s in shadows])
        self.n_chunks = int(n.item())
        assert self.n_chunks == R * sum(-(-per // 1024) for per in V.SGD_PER)
        self.partials = torch.zeros(self.n_chunks, device=DEV)
        self.normsq = torch.zeros(R, device=DEV)

    def step(self, max_norm, lr, momentum, weight_decay):
        ext().clip_sgd_step(self.table, self.n_chunks, self.chunk_client,
                            self.partials, self.normsq, max_norm, lr,
                            momentum, weight_decay)


def _cat(ts):
    return torch.cat([t.reshape(-1).double().cpu() for t in ts])


@needs_gpu
@pytest.mark.parametrize('vec', [True, False], ids=['vec', 'novec'])
@pytest.mark.parametrize('how', ['table1024', 'fused'])
def test_clip_sgd_matches_fp64(how, vec):
    from heterofl_amd.ops.fused import FusedClipSGD
    R, h = V.SGD_R, V.SGD_HYPER
    params, grads, bufs = V.sgd_inputs()
    r64 = V.clip_sgd(params, grads, bufs, R, steps=V.SGD_STEPS, dtype=F64, **h)
    r32 = V.clip_sgd(params, grads, bufs, R, steps=V.SGD_STEPS, dtype=F32, **h)
    dp, grads, db, cur, shadows = _sgd_device_state()
    if how == 'fused':
        opt = FusedClipSGD(dp, cur, db, R, DEV, shadows)
    else:
        opt = _Table1024(dp, cur, db, R, shadows)
    cid = '{}-{}'.format(how, 'vec' if vec else 'novec')
    rows = []
    with stream_vec(vec):
        for step in range(V.SGD_STEPS):
            for c, g in zip(cur, grads[step]):
                c.copy_(g)
            opt.step(h['max_norm'], h['lr'], h['mom'], h['wd'])
            torch.cuda.synchronize()
            p64, b64, n64 = r64[step]
            p32, b32, n32 = r32[step]
            rows.append(('param.{}'.format(step),
                         _excess(_cat(dp), _cat(p64)),
                         V.fp32_tol(_cat(p32), _cat(p64))))
            rows.append(('buf.{}'.format(step), _excess(_cat(db), _cat(b64)),
                         V.fp32_tol(_cat(b32), _cat(b64))))
            rows.append(('norm.{}'.format(step),
                         _excess(opt.normsq.sqrt().cpu(), n64),
                         V.fp32_tol(n32, n64)))
            for p, s in zip(dp, shadows):
                if s is not None:
                    assert torch.equal(s, p.to(torch.bfloat16)), (cid, step)
    # client 0 clipped, client 1 not, client 2 without a gradient
    ns = opt.normsq.cpu()
    assert ns[0].item() > 1.0 > ns[1].item() > 0.0 and ns[2].item() == 0.0
    _judge('sgd', cid, rows)
    # with no gradient a client's step is weight decay alone: exact zeros
    # would mean the scale blew up
    for p in dp:
        assert bool(torch.isfinite(p).all())


@needs_gpu
@pytest.mark.parametrize('chunk', [65536, 1024])
@pytest.mark.parametrize('vec', [True, False], ids=['vec', 'novec'])
def test_graph_clip_sgd_bit_equal_to_fused(vec, chunk):
    """GraphClipSGD.bind + launch (no capture needed) against
    FusedClipSGD.step on clones: the same table, the same kernels."""
    from heterofl_amd.ops import fused
    R, h = V.SGD_R, V.SGD_HYPER
    Fused = type('Fused', (fused.FusedClipSGD,), {'CHUNK': chunk})
    Graph = type('Graph', (fused.GraphClipSGD,), {'CHUNK': chunk})
    a = _sgd_device_state()
    b = _sgd_device_state()
    fo = Fused(a[0], a[3], a[2], R, DEV, a[4])
    go = Graph(b[0], b[2], R, DEV, b[4])
    go.bind(b[3])
    assert go.n_chunks == fo.n_chunks
    assert torch.equal(go.chunk_client.cpu(), fo.chunk_client.cpu())
    with stream_vec(vec):
        for step in range(V.SGD_STEPS):
            for st in (a, b):
                for c, g in zip(st[3], st[1][step]):
                    c.copy_(g)
            fo.step(h['max_norm'], h['lr'], h['mom'], h['wd'])
            go.launch(h['max_norm'], h['lr'], h['mom'], h['wd'])
            torch.cuda.synchronize()
            assert torch.equal(fo.normsq, go.normsq)
            assert torch.equal(fo.partials, go.partials)
            for i in range(len(V.SGD_PER)):
                assert torch.equal(a[0][i], b[0][i]), ('param', step, i)
                assert torch.equal(a[2][i], b[2][i]), ('buf', step, i)
                if a[4][i] is not None:
                    assert torch.equal(a[4][i], b[4][i]), ('shadow', step, i)
