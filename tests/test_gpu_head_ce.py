"""The two-launch classifier tail (ops/csrc/head_ce.hip) against the four
kernels it replaces and against the fp64 references.

Bit-equality: head_ce_fwd / head_ce_bwd keep every value's arithmetic chain,
so losses, pooled, scores, metrics (after two accumulating calls), dW, db and
dfeat are compared with torch.equal against head_fwd -> masked_ce_fwd and
masked_ce_bwd -> head_bwd on the same inputs.

fp64: V.head and V.masked_ce with the bounds tests/test_gpu_vision_kernels.py
uses for the old kernels (16 x the reference's own fp32-vs-fp64 spread, half a
bf16 ulp for a bf16 output, the __expf / __logf slack).  The fused kernel
feeds its CE with its own fp32 scores and its head backward with its own fp32
dscores, so each stage's reference starts from what the stage before handed
on (the kernel's scores; the chain's dscores, bit-equal to the fused kernel's
by the first test): every stage then answers for its own arithmetic with the
bound of its own test there, and the error of a stage is not counted twice.
"""
import contextlib
import os

import pytest
import torch

from tests import vision_refs as V

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
NONE = torch.Tensor()

# (N, R, C, H, W, J) -> route per io dtype with the switch on
NARROW = (10, 5, 32, 4, 4, 10)
N1 = (1, 2, 20, 2, 2, 7)
N65 = (65, 2, 24, 2, 4, 10)
# inside the envelope with many classes and an odd batch (forward stage
# 50420 bytes): the e / J and e / cs splits, the padded w rows, a label-only
# mask over more classes than a wave has lanes
J100 = (37, 2, 64, 2, 2, 100)
ROUTES = {
    V.HEAD_CASES[0]: {'fp32': 'vec', 'bf16': 'vec'},       # flagship
    V.HEAD_CASES[1]: {'fp32': 'elem', 'bf16': 'elem'},     # 1x1 plane
    V.HEAD_CASES[2]: {'fp32': 'chain', 'bf16': 'chain'},   # J = 100: w stage
    V.HEAD_CASES[3]: {'fp32': 'elem', 'bf16': 'elem'},     # 24 / 12 bytes
    V.HEAD_CASES[4]: {'fp32': 'vec', 'bf16': 'elem'},      # 16 / 8 bytes
    NARROW: {'fp32': 'vec', 'bf16': 'vec'},
    N1: {'fp32': 'vec', 'bf16': 'elem'},
    N65: {'fp32': 'vec', 'bf16': 'vec'},
    J100: {'fp32': 'vec', 'bf16': 'elem'},
}
CASES = list(ROUTES)
# forward stage ((N + J) * (C + 1) + N * J) * 4 bytes against 64 KB = 65536:
# C = 813 -> 65520, C = 818 -> 65920
EDGE_IN = (10, 1, 813, 2, 2, 10)
EDGE_OUT = (10, 1, 818, 2, 2, 10)
MASKS = ['none', 'random', 'label_only']


def ext():
    from heterofl_amd.ops import require_native
    return require_native()


@contextlib.contextmanager
def step_fused(on):
    prev = os.environ.get('HETEROFL_STEP_FUSED')
    os.environ['HETEROFL_STEP_FUSED'] = '1' if on else '0'
    try:
        yield
    finally:
        if prev is None:
            del os.environ['HETEROFL_STEP_FUSED']
        else:
            os.environ['HETEROFL_STEP_FUSED'] = prev


def ce_side(case, variant, call=0):
    """labels (N, R) with 0 and J - 1 present, mask (R, J) or None, up (R,)"""
    N, R, C, H, W, J = case
    gen = torch.Generator().manual_seed(31 * N + 7 * J + R + 7919 * call)
    labels = torch.randint(0, J, (N, R), generator=gen)
    labels[0, :] = 0
    labels[-1, :] = J - 1
    mask = None
    if variant == 'random':
        mask = (torch.rand(R, J, generator=gen) > 0.4).float()
    elif variant == 'label_only':
        lab = torch.randint(0, J, (R,), generator=gen)
        lab[0] = J - 1
        labels = lab.unsqueeze(0).expand(N, R).contiguous()
        mask = torch.zeros(R, J).scatter_(1, lab.unsqueeze(1), 1.0)
    up = torch.rand(R, generator=gen) + 0.25 + torch.arange(R)
    return labels, mask, up


def _d(t):
    return NONE if t is None else t.to(DEV)


def chain(feat, w, b, labels, mask, metrics, up, case):
    """today's four kernels"""
    N, R, C, H, W, J = case
    e = ext()
    scores, pooled = e.head_fwd(feat, w, b, R)
    (losses,) = e.masked_ce_fwd(scores, labels, mask, metrics)
    dsc = e.masked_ce_bwd(scores, labels, mask, up)
    dw, db, dfeat = e.head_bwd(dsc, pooled, w, R, H, W,
                               feat.dtype == torch.bfloat16, b.numel() > 0)
    return dict(losses=losses, pooled=pooled, scores=scores, dw=dw, db=db,
                dfeat=dfeat, dscores=dsc)


def fused(feat, w, b, labels, mask, metrics, up, case):
    N, R, C, H, W, J = case
    e = ext()
    losses, pooled, scores = e.head_ce_fwd(feat, w, b, labels, mask, metrics,
                                           R)
    dw, db, dfeat = e.head_ce_bwd(up, scores, labels, mask, pooled, w, R, H,
                                  W, feat.dtype == torch.bfloat16,
                                  b.numel() > 0)
    return dict(losses=losses, pooled=pooled, scores=scores, dw=dw, db=db,
                dfeat=dfeat)


def assert_same(a, b, what):
    for k in ('losses', 'pooled', 'scores', 'dw', 'db', 'dfeat'):
        x, y = a[k], b[k]
        if k == 'db' and x is None and y is None:     # no bias
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert torch.equal(x, y), (what, k, (x.float() - y.float()).abs()
                                   .max().item())


def ups(up):
    """dense unit-stride, stride-0 expand, dense non-unit stride"""
    R = up.numel()
    wide = torch.zeros(R, 3, device=up.device)
    wide[:, 1] = up
    one = torch.ones(1, device=up.device)
    return [('dense', up), ('expand', one.expand(R)),
            ('strided', wide[:, 1])]


@needs_gpu
@pytest.mark.parametrize('variant', MASKS)
@pytest.mark.parametrize('io_name', list(V.IO_DTYPES))
@pytest.mark.parametrize('case', CASES,
                         ids=[V.head_case_id(c) for c in CASES])
def test_bit_equal_to_chain(case, io_name, variant):
    from heterofl_amd.ops.fused import head_ce_route
    N, R, C, H, W, J = case
    esz = 4 if io_name == 'fp32' else 2
    assert head_ce_route(N, R, C, H * W, J, esz) == ROUTES[case][io_name]
    for bias in (True, False):
        feat, w, b, _ = V.head_inputs(case, io_name, bias)
        feat, w, b = feat.to(DEV), w.to(DEV), _d(b)
        assert feat.data_ptr() % 16 == 0
        m_old = torch.zeros(R, 3, device=DEV)
        m_new = torch.zeros(R, 3, device=DEV)
        for call in range(2):
            labels, mask, up = ce_side(case, variant, call)
            labels, mask, up = labels.to(DEV), _d(mask), up.to(DEV)
            for name, u in ups(up):
                # metrics accumulate once per call: the first `up` only
                mo = m_old if name == 'dense' else NONE
                mn = m_new if name == 'dense' else NONE
                old = chain(feat, w, b, labels, mask, mo, u, case)
                new = fused(feat, w, b, labels, mask, mn, u, case)
                assert_same(old, new, (bias, call, name))
        torch.cuda.synchronize()
        assert torch.equal(m_old, m_new), (bias, m_old, m_new)
        assert bool((m_new[:, 2] == 2 * N).all())


@needs_gpu
@pytest.mark.parametrize('io_name', list(V.IO_DTYPES))
def test_offset_view_takes_element_path(io_name):
    """feat that starts one element into its buffer: contiguous, not 16-byte
    aligned"""
    from heterofl_amd.ops.fused import head_ce_route
    case = V.HEAD_CASES[0]
    N, R, C, H, W, J = case
    feat, w, b, _ = V.head_inputs(case, io_name)
    esz = feat.element_size()
    buf = torch.zeros(feat.numel() + 1, dtype=feat.dtype, device=DEV)
    view = buf[1:].view(feat.shape)
    view.copy_(feat)
    assert view.is_contiguous() and view.data_ptr() % 16 == esz
    assert head_ce_route(N, R, C, H * W, J, esz, False) == 'elem'
    labels, mask, up = ce_side(case, 'random')
    args = (w.to(DEV), b.to(DEV), labels.to(DEV), mask.to(DEV))
    m_old = torch.zeros(R, 3, device=DEV)
    m_new = torch.zeros(R, 3, device=DEV)
    old = chain(view, *args, m_old, up.to(DEV), case)
    new = fused(view, *args, m_new, up.to(DEV), case)
    aligned = fused(feat.to(DEV), *args, NONE, up.to(DEV), case)
    torch.cuda.synchronize()
    assert_same(old, new, 'offset')
    assert_same(new, aligned, 'offset vs aligned')
    assert torch.equal(m_old, m_new)


@needs_gpu
@pytest.mark.parametrize('case', [EDGE_IN, EDGE_OUT],
                         ids=['inside', 'outside'])
def test_envelope_edge(case):
    """The largest C inside the forward LDS stage and the first one outside:
    the route is pinned and both sides are right."""
    from heterofl_amd.ops.fused import head_ce_route
    N, R, C, H, W, J = case
    want = 'vec' if case == EDGE_IN else 'chain'
    assert head_ce_route(N, R, C, H * W, J, 4) == want
    _fp64_check(case, 'fp32', 'random', 'edge-' + want)


@needs_gpu
@pytest.mark.parametrize('io_name', list(V.IO_DTYPES))
def test_switch_off_runs_old_chain(io_name):
    from heterofl_amd.ops.fused import head_ce_route
    case = V.HEAD_CASES[0]
    N, R, C, H, W, J = case
    feat, w, b, _ = V.head_inputs(case, io_name)
    labels, mask, up = ce_side(case, 'random')
    args = (feat.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV), mask.to(DEV))
    m_old = torch.zeros(R, 3, device=DEV)
    m_off = torch.zeros(R, 3, device=DEV)
    old = chain(*args, m_old, up.to(DEV), case)
    with step_fused(False):
        assert head_ce_route(N, R, C, H * W, J, feat.element_size()) \
            == 'chain'
        off = fused(*args, m_off, up.to(DEV), case)
    assert head_ce_route(N, R, C, H * W, J, feat.element_size()) == 'vec'
    torch.cuda.synchronize()
    assert_same(old, off, 'switch off')
    assert torch.equal(m_old, m_off)


def _excess(got, ref, io_name=None, slack=None):
    err = (got.double().cpu() - ref.double()).abs()
    if io_name == 'bf16':
        err = err - V.bf16_ulp(ref) / 2
    if slack is not None:
        err = err - slack
    return err.clamp_min(0).max().item() if err.numel() else 0.0


def _fp64_check(case, io_name, variant, cid, with_metrics=True):
    N, R, C, H, W, J = case
    feat, w, b, _ = V.head_inputs(case, io_name)
    labels, mask, up = ce_side(case, variant)
    metrics = torch.zeros(R, 3, device=DEV) if with_metrics else NONE
    args = (feat.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV), _d(mask))
    got = fused(*args, metrics, up.to(DEV), case)
    dsc = ext().masked_ce_bwd(got['scores'], labels.to(DEV), _d(mask),
                              up.to(DEV)).cpu()
    torch.cuda.synchronize()
    scores = got['scores'].cpu()
    h64 = V.head(feat, w, b, dsc, R, dtype=F64)
    h32 = V.head(feat, w, b, dsc, R, dtype=F32)
    c64 = V.masked_ce(scores, labels, mask, up, dtype=F64)
    c32 = V.masked_ce(scores, labels, mask, up, dtype=F32)
    nll_slack, _ = V.masked_ce_intrinsic_slack(scores, labels, mask, up)
    rows = []
    for name in ('scores', 'pooled', 'dfeat', 'dw', 'db'):
        ref = getattr(h64, name)
        io = io_name if name == 'dfeat' else None
        rows.append((name, _excess(got[name], ref, io),
                     V.fp32_tol(getattr(h32, name), ref)))
    rows.append(('losses', _excess(got['losses'], c64.losses,
                                   slack=nll_slack.mean(0)),
                 V.fp32_tol(c32.losses, c64.losses)))
    if with_metrics:
        m = metrics.cpu()
        rows.append(('metrics.sum_nll',
                     _excess(m[:, 0], c64.metrics[:, 0],
                             slack=nll_slack.sum(0)),
                     V.fp32_tol(c32.metrics[:, 0], c64.metrics[:, 0])))
        assert torch.equal(m[:, 1].double(), c64.metrics[:, 1]), cid
        assert torch.equal(m[:, 2].double(), c64.metrics[:, 2]), cid
    fails = []
    for name, err, bound in rows:
        print('VK head_ce {} {} err={:.3e} bound={:.3e}'.format(cid, name,
                                                                err, bound))
        if not err <= bound:
            fails.append((name, err, bound))
    assert not fails, (cid, fails)
    assert got['dfeat'].dtype == feat.dtype


@needs_gpu
@pytest.mark.parametrize('variant', MASKS)
@pytest.mark.parametrize('io_name', list(V.IO_DTYPES))
@pytest.mark.parametrize('case', CASES,
                         ids=[V.head_case_id(c) for c in CASES])
def test_matches_fp64(case, io_name, variant):
    _fp64_check(case, io_name, variant,
                '{}-{}-{}'.format(V.head_case_id(case), io_name, variant))


@needs_gpu
def test_without_metrics_and_autograd_wrapper():
    """fused_head_ce through autograd with a stride-0 upstream gradient (what
    losses.sum().backward() hands down) equals the entries called directly;
    no metrics buffer."""
    from heterofl_amd.ops.fused import fused_head_ce
    case = V.HEAD_CASES[0]
    N, R, C, H, W, J = case
    feat, w, b, _ = V.head_inputs(case, 'bf16')
    labels, mask, _ = ce_side(case, 'random')
    fg = feat.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True)
    losses, scores = fused_head_ce(fg, wg, bg, labels.to(DEV), mask.to(DEV),
                                   R)
    assert not scores.requires_grad
    grads = torch.autograd.grad(losses.sum(), (fg, wg, bg))
    ones = torch.ones(R, device=DEV)
    want = fused(fg.detach(), wg.detach(), bg.detach(), labels.to(DEV),
                 mask.to(DEV), NONE, ones, case)
    _fp64_check(case, 'bf16', 'random', 'nometrics', with_metrics=False)
    torch.cuda.synchronize()
    assert torch.equal(losses.detach(), want['losses'])
    assert torch.equal(scores, want['scores'])
    assert torch.equal(grads[0], want['dfeat'])
    assert torch.equal(grads[1], want['dw'])
    assert torch.equal(grads[2], want['db'])


@needs_gpu
def test_wrong_arguments_are_refused_before_the_launch():
    case = NARROW
    N, R, C, H, W, J = case
    feat, w, b, _ = V.head_inputs(case, 'fp32')
    labels, mask, up = ce_side(case, 'random')
    feat, w, b = feat.to(DEV), w.to(DEV), b.to(DEV)
    labels, mask, up = labels.to(DEV), mask.to(DEV), up.to(DEV)
    e = ext()
    with pytest.raises(RuntimeError, match='w must be'):
        e.head_ce_fwd(feat, w[:, :, :C - 1].contiguous(), b, labels, mask,
                      NONE, R)
    with pytest.raises(RuntimeError, match='labels must be'):
        e.head_ce_fwd(feat, w, b, labels.cpu(), mask, NONE, R)
    with pytest.raises(RuntimeError, match='feat channels'):
        e.head_ce_fwd(feat[:, :R * C - 1].contiguous(), w, b, labels, mask,
                      NONE, R)
    losses, pooled, scores = e.head_ce_fwd(feat, w, b, labels, mask, NONE, R)
    with pytest.raises(RuntimeError, match='pooled must be'):
        e.head_ce_bwd(up, scores, labels, mask, pooled[:N - 1].contiguous(),
                      w, R, H, W, False, True)
    with pytest.raises(RuntimeError, match='scores must be'):
        e.head_ce_bwd(up, scores.double(), labels, mask, pooled, w, R, H, W,
                      False, True)
    torch.cuda.synchronize()
