"""Plain-torch references for the vision training kernels (fused_norm.hip,
masked_ce.hip, head.hip, clip_sgd.hip), the case lists of their tests and
the input generators both test files share.

Every reference takes a `dtype` (torch.float64 for the oracle, torch.float32
to measure what fp32 arithmetic alone costs) and runs on whatever device its
inputs live on; bf16 inputs are upcast exactly.  Nothing goes through
autograd: the pre-activation and the ReLU mask are visible, and the fp32 run
of a reference has the same kind of arithmetic error as a kernel.

`one_pass=True` is the arithmetic the norm kernels use (read from
fused_norm.hip): the variance as E[x^2] - mean^2 clamped at 0, and for
BatchNorm the affine folded into y = x * scale + shift with scale = invstd *
g, shift = b - mean * scale (GroupNorm keeps (x - mean) * invstd * g + b, as
its kernel does).  Both lose precision with the offset mean / sigma of the
data; the fp32-vs-fp64 spread of a one-pass reference is therefore the
yardstick for a one-pass kernel.  `one_pass=False` sums (x - mean)^2 and
never folds: what torch does.  eps enters as its fp32 value in either dtype,
because that is what the launchers hand the kernels.
"""
import collections

import torch

from tests.lm_refs import bf16r, bf16_ulp, rel_fro, max_abs  # noqa: F401

IO_DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
EPS = 1e-5
TOL_FACTOR = 16            # tests/test_gpu_lm_kernels.py: layernorm, lm_ce
FLOOR = 2.0 ** -23         # one fp32 ulp of the largest reference value

NormOut = collections.namedtuple(
    'NormOut', 'y mean invstd pre dx dgamma dbeta')
CEOut = collections.namedtuple('CEOut', 'losses dscores metrics')
HeadOut = collections.namedtuple('HeadOut', 'scores pooled dfeat dw db')

NORM_OUTPUTS = ('y', 'mean', 'invstd', 'dx', 'dgamma', 'dbeta')


def _up(t, dtype):
    return t.detach().to(dtype)


def eps32(eps, dtype):
    return torch.tensor(eps, dtype=torch.float32).to(dtype).item()


def fp32_tol(r32, r64):
    """16 x the fp32-vs-fp64 spread of the reference, at least one fp32 ulp
    of the largest reference value."""
    return max(TOL_FACTOR * max_abs(r32, r64),
               FLOOR * r64.double().abs().max().item())


def relu_boundary(pre, tau):
    """Elements whose ReLU decision an error of tau in `pre` could flip."""
    return pre.abs() < tau


def boundary_tau(pre32, pre64):
    """16 x the fp32-vs-fp64 spread of pre, at least 2^-23 max|pre|."""
    return fp32_tol(pre32, pre64)


# ------------------------------------------------------------------ BN+ReLU
def bn_relu(x, w, b, dy, eps=EPS, dtype=torch.float64, one_pass=True):
    """relu(batch_norm(x) * w + b) over (N, C, H, W) with batch statistics,
    and its gradients for the upstream dy.  w / b None: no affine."""
    x, dy = _up(x, dtype), _up(dy, dtype)
    C = x.size(1)
    M = x.numel() // C
    e = eps32(eps, dtype)
    dims = (0, 2, 3)
    cv = (1, C, 1, 1)
    mean = x.mean(dims)
    if one_pass:
        var = ((x * x).mean(dims) - mean * mean).clamp_min(0)
    else:
        var = ((x - mean.view(cv)) ** 2).mean(dims)
    invstd = 1.0 / torch.sqrt(var + e)
    g = _up(w, dtype) if w is not None else torch.ones_like(mean)
    bb = _up(b, dtype) if b is not None else torch.zeros_like(mean)
    xh = (x - mean.view(cv)) * invstd.view(cv)
    if one_pass:
        scale = invstd * g
        shift = bb - mean * scale
        pre = x * scale.view(cv) + shift.view(cv)
    else:
        pre = xh * g.view(cv) + bb.view(cv)
    y = pre.clamp_min(0)
    d = torch.where(pre > 0, dy, torch.zeros_like(dy))
    dbeta = d.sum(dims)
    dgamma = (d * xh).sum(dims)
    dx = (g * invstd).view(cv) * (d - (dbeta / M).view(cv)
                                  - xh * (dgamma / M).view(cv))
    return NormOut(y, mean, invstd, pre, dx, dgamma, dbeta)


def bn_flip_slack(x, w, dy, ref, excluded):
    """What flipping the ReLU decision of the `excluded` elements can change
    at most: (dgamma, dbeta) per channel and dx elementwise, exact bounds
    from sum |dy xhat| and sum |dy| over the excluded set."""
    dtype = ref.pre.dtype
    x, dy = _up(x, dtype), _up(dy, dtype)
    C = x.size(1)
    M = x.numel() // C
    cv = (1, C, 1, 1)
    g = _up(w, dtype) if w is not None else torch.ones_like(ref.mean)
    xh = (x - ref.mean.view(cv)) * ref.invstd.view(cv)
    a = torch.where(excluded, dy.abs(), torch.zeros_like(dy))
    s_beta = a.sum((0, 2, 3))
    s_gamma = (a * xh.abs()).sum((0, 2, 3))
    s_dx = (g.abs() * ref.invstd).view(cv) * (
        (s_beta / M).view(cv) + xh.abs() * (s_gamma / M).view(cv))
    return s_gamma, s_beta, s_dx


# ------------------------------------------------------------------ GN+ReLU
def gn_relu(x, w, b, dy, G, eps=EPS, dtype=torch.float64, one_pass=True):
    """relu(group_norm(x, G) * w + b); mean / invstd come back flat (N * G)."""
    x, dy = _up(x, dtype), _up(dy, dtype)
    N, C = x.size(0), x.size(1)
    if C % G:
        raise ValueError('channels not divisible by groups')
    e = eps32(eps, dtype)
    xg = x.reshape(N, G, -1)
    M = xg.size(2)
    mean = xg.mean(2)
    if one_pass:
        var = ((xg * xg).mean(2) - mean * mean).clamp_min(0)
    else:
        var = ((xg - mean.unsqueeze(2)) ** 2).mean(2)
    invstd = 1.0 / torch.sqrt(var + e)
    cv = (1, C, 1, 1)
    g = _up(w, dtype) if w is not None else x.new_ones(C)
    bb = _up(b, dtype) if b is not None else x.new_zeros(C)
    xh = ((xg - mean.unsqueeze(2)) * invstd.unsqueeze(2)).reshape(x.shape)
    pre = xh * g.view(cv) + bb.view(cv)
    y = pre.clamp_min(0)
    d = torch.where(pre > 0, dy, torch.zeros_like(dy))
    dbeta = d.sum((0, 2, 3))
    dgamma = (d * xh).sum((0, 2, 3))
    dg = (d * g.view(cv)).reshape(N, G, -1)
    k1 = dg.mean(2, keepdim=True)
    k2 = (dg * xh.reshape(N, G, -1)).mean(2, keepdim=True)
    dx = (invstd.unsqueeze(2) * (dg - k1 - xh.reshape(N, G, -1) * k2)) \
        .reshape(x.shape)
    assert M == (C // G) * (x.numel() // (N * C))
    return NormOut(y, mean.reshape(-1), invstd.reshape(-1), pre, dx, dgamma,
                   dbeta)


# ---------------------------------------------------------------- masked CE
def _masked(scores, mask, dtype):
    s = _up(scores, dtype)
    if mask is not None:
        s = s.masked_fill(mask.unsqueeze(0) == 0, 0)
    return s


def masked_ce(scores, labels, mask, up, dtype=torch.float64):
    """scores (N, R, C), labels (N, R), mask (R, C) in {0, 1} or None, up (R,)
    the upstream gradient of losses.  masked_fill(mask == 0, 0): a masked
    class stays in the softmax at score 0 and gets no gradient.  Returns
    losses (R,) (mean NLL), dscores, metrics (R, 3) = (sum NLL, correct,
    count); the prediction is the lowest index holding the maximum."""
    s = _masked(scores, mask, dtype)
    N, R, C = s.shape
    mx = s.max(-1, keepdim=True).values
    ex = torch.exp(s - mx)
    den = ex.sum(-1, keepdim=True)
    lse = (mx + torch.log(den)).squeeze(-1)
    nll = lse - s.gather(2, labels.unsqueeze(-1)).squeeze(-1)
    losses = nll.mean(0)
    onehot = torch.zeros_like(s).scatter_(2, labels.unsqueeze(-1), 1.0)
    dscores = (ex / den - onehot) * (_up(up, dtype) / N).view(1, R, 1)
    if mask is not None:
        dscores = dscores.masked_fill(mask.unsqueeze(0) == 0, 0)
    cls = torch.arange(C, device=s.device).expand_as(s)
    pred = torch.where(s == mx, cls, torch.full_like(cls, C)).min(-1).values
    metrics = torch.stack([nll.sum(0), (pred == labels).to(dtype).sum(0),
                           torch.full_like(losses, float(N))], 1)
    return CEOut(losses, dscores, metrics)


U_EXP = 2.0 ** -22   # see masked_ce_intrinsic_slack


def masked_ce_intrinsic_slack(scores, labels, mask, up):
    """What __expf / __logf may add on top of correctly rounded fp32, from the
    documented accuracy of the hardware instructions they compile to (AMD
    CDNA ISA guide: V_EXP_F32 and V_LOG_F32 are base-2 and accurate to 1 ulp):
      __expf(t) = exp2(t * log2(e)).  Rounding the product t * log2(e) to
        fp32 moves the result by |t| 2^-24 relative, the constant log2(e) by
        as much again, the instruction by 1 ulp = 2^-23: together under
        (1 + |t|) 2^-22 =: r(t) relative, t = v - max.
      __logf(s) = log2(s) * ln(2): 1 ulp for the instruction, half an ulp
        each for the constant and the product: under 2^-22 |log s| absolute.
    The denominator sum e_j then carries sum p_j r(t_j) =: rd relative, which
    is rd absolute in its logarithm, so
      NLL per sample:  rd + 2^-22 |log sum e_j|
      p_c = e_c / den: p_c (r(t_c) + rd) absolute,  dscores: x |up_r| / N.
    Returns (nll_slack (N, R), dscores_slack (N, R, C)) in fp64."""
    s = _masked(scores, mask, torch.float64)
    N, R, C = s.shape
    t = s - s.max(-1, keepdim=True).values
    ex = torch.exp(t)
    den = ex.sum(-1, keepdim=True)
    p = ex / den
    r = (1 + t.abs()) * U_EXP
    rd = (p * r).sum(-1, keepdim=True)
    nll_slack = (rd + U_EXP * torch.log(den).abs()).squeeze(-1)
    d_slack = p * (r + rd) * (up.double().abs() / N).view(1, R, 1)
    return nll_slack, d_slack


# --------------------------------------------------------------------- head
def head(feat, w, b, dscores, R, dtype=torch.float64):
    """feat (N, R*C, H, W) -> pooled (N, R, C) = mean over the plane,
    scores (N, R, J) = pooled @ w[r]^T + b[r]; w (R, J, C), b (R, J) or None.
    Gradients for the upstream dscores; db is None without a bias."""
    f = _up(feat, dtype)
    N, H, W = f.size(0), f.size(2), f.size(3)
    C = f.size(1) // R
    wd = _up(w, dtype)
    ds = _up(dscores, dtype)
    pooled = f.reshape(N, R, C, H * W).mean(-1)
    scores = torch.einsum('nrc,rjc->nrj', pooled, wd)
    if b is not None:
        scores = scores + _up(b, dtype).unsqueeze(0)
    dw = torch.einsum('nrj,nrc->rjc', ds, pooled)
    db = ds.sum(0) if b is not None else None
    dpool = torch.einsum('nrj,rjc->nrc', ds, wd) / (H * W)
    dfeat = dpool.reshape(N, R * C, 1, 1).expand(N, R * C, H, W).contiguous()
    return HeadOut(scores, pooled, dfeat, dw, db)


# ----------------------------------------------------------------- clip+SGD
def clip_sgd(params, grads, bufs, R, max_norm, lr, mom, wd, steps,
             dtype=torch.float64):
    """Per-client clip + momentum SGD.  params / bufs: lists of tensors whose
    flat storage is R equal client slices; grads[step] the same list for each
    step.  norm_r over client r's slice of every tensor; scale_r = min(1,
    max_norm / (norm_r + 1e-6)); g = grad * scale_r + wd * p; buf = mom * buf
    + g (dampening 0); p -= lr * buf.  Returns [(params, bufs, norms)] after
    each step."""
    ps = [_up(p, dtype).reshape(R, -1).clone() for p in params]
    bs = [_up(b, dtype).reshape(R, -1).clone() for b in bufs]
    out = []
    for step in range(steps):
        gs = [_up(g, dtype).reshape(R, -1) for g in grads[step]]
        norm = torch.sqrt(sum((g * g).sum(1) for g in gs))
        scale = (max_norm / (norm + 1e-6)).clamp_max(1.0).unsqueeze(1)
        for p, g, bf in zip(ps, gs, bs):
            bf.mul_(mom).add_(g * scale + wd * p)
            p.sub_(lr * bf)
        out.append(([p.reshape(-1).clone() for p in ps],
                    [b.reshape(-1).clone() for b in bs], norm))
    return out


# ================================================================= BN cases
# name -> (N, C, H, W), seed, routes with HETEROFL_STREAM_VEC on as
# {io: (fwd, bwd)}.  With the vector routes off 'vec' reads 'staged'.  The
# seeds are the first for which no element of any variant (io dtype, affine on
# and off) lies within boundary_tau of the ReLU boundary: test_vision_refs.py
# asserts it.  split3 is the exception, see there.
_V, _S, _D, _3 = 'vec', 'staged', 'direct', 'split3'
BN_CASES = collections.OrderedDict([
    ('p4', ((10, 8, 4, 4), 1, {'fp32': (_V, _V), 'bf16': (_V, _V)})),
    ('e192', ((3, 5, 8, 8), 1, {'fp32': (_V, _V), 'bf16': (_V, _V)})),
    ('hw24', ((2, 3, 4, 6), 1, {'fp32': (_V, _V), 'bf16': (_V, _V)})),
    ('hw12', ((7, 4, 2, 6), 1, {'fp32': (_V, _V), 'bf16': (_S, _S)})),
    ('p7', ((4, 3, 7, 7), 1, {'fp32': (_S, _S), 'bf16': (_S, _S)})),
    ('m1', ((1, 3, 1, 1), 1, {'fp32': (_S, _S), 'bf16': (_S, _S)})),
    ('m2', ((2, 2, 1, 1), 1, {'fp32': (_S, _S), 'bf16': (_S, _S)})),
    ('n10', ((10, 2, 32, 32), 1, {'fp32': (_V, _D), 'bf16': (_V, _V)})),
    ('n20', ((20, 2, 32, 32), 2, {'fp32': (_D, _D), 'bf16': (_V, _D)})),
    ('split3', ((65, 128, 32, 32), 1, {'fp32': (_3, _D), 'bf16': (_3, _D)})),
    ('special', ((10, 6, 4, 4), 2, {'fp32': (_V, _V), 'bf16': (_V, _V)})),
])
BN_BOUNDARY_FREE = [c for c in BN_CASES if c != 'split3']
# (case, affine) pairs the tests run.  m1 runs with affine only: without it
# every pre-activation is exactly 0, on the ReLU boundary for any seed, and
# the exact y is 0, which leaves a bound relative to max|y| nothing to stand
# on.  (The kernels' y = x * scale + shift is then the rounding residual of
# x * scale: 9.0e-8 in fp32, 7.5e-6 in bf16 on an MI355X, with |x * scale| up
# to 209.)  In `special` without affine the all-zero and the constant channel
# have pre = 0 exactly too, among four ordinary channels.
BN_VARIANTS = [(c, a) for c in BN_CASES for a in (True, False)
               if (c, a) != ('m1', False)]


def bn_variant_id(v):
    return '{}-{}'.format(v[0], 'affine' if v[1] else 'plain')
SPLIT3_MAX_SHARE = 1e-4


def _affine(C, gen, affine):
    if not affine:
        return None, None
    return (torch.rand(C, generator=gen) + 0.5,
            torch.randn(C, generator=gen))


def bn_inputs(case, io_name, affine=True):
    """x, dy in the io dtype, w, b fp32 (None without affine), on the CPU."""
    shape, seed, _ = BN_CASES[case]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen)
    dy = torch.randn(shape, generator=gen)
    w, b = _affine(shape[1], gen, affine)
    if case == 'special':
        x[:, 0] = 0.0              # a dead ReLU channel upstream
        x[:, 1] = 0.5              # constant
        x[:, 2] *= 1e-3            # eps dominates invstd
        x[:, 3] *= 1e3
        x[:, 4] += 8.0             # mean = +8 sigma
        x[:, 5] -= 8.0
    io = IO_DTYPES[io_name]
    return x.to(io), dy.to(io), w, b


# ================================================================= GN cases
# name -> (N, C, H, G), seed; planes are H x H
GN_CASES = collections.OrderedDict([
    ('gn20', ((10, 40, 8, 20), 1)),
    ('in', ((4, 16, 4, 16), 1)),          # cpg = 1
    ('ln', ((3, 12, 4, 1), 1)),
    ('m1', ((2, 6, 1, 6), 1)),            # one element per group
    ('cpg300', ((1, 600, 1, 2), 1)),      # more channels than lanes
    ('big17', ((2, 17, 32, 1), 2)),       # 68 KB in fp32: unstaged forward
    ('big33', ((2, 33, 32, 1), 4)),       # 66 KB in bf16: unstaged forward
])
GN_STAGE_BYTES = 64 * 1024


def gn_unstaged(case, io_name):
    (N, C, H, G), _ = GN_CASES[case]
    esz = 4 if io_name == 'fp32' else 2
    return (C // G) * H * H * esz > GN_STAGE_BYTES


def gn_inputs(case, io_name, affine=True):
    (N, C, H, G), seed = GN_CASES[case]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, H, generator=gen)
    dy = torch.randn(N, C, H, H, generator=gen)
    w, b = _affine(C, gen, affine)
    io = IO_DTYPES[io_name]
    return x.to(io), dy.to(io), w, b, G


# ================================================================= CE cases
CE_SHAPES = [(10, 5, 10), (1, 1, 1), (64, 1, 2), (65, 3, 10), (130, 2, 100)]
CE_MASKS = ['none', 'random', 'label_only']
# (shape, mask variant, score scale)
CE_CASES = [(s, m, 1.0) for s in CE_SHAPES for m in CE_MASKS] \
    + [((65, 3, 10), 'random', 30.0), ((130, 2, 100), 'none', 30.0)]


def ce_case_id(case):
    (N, R, C), m, scale = case
    return '{}x{}x{}-{}-s{:g}'.format(N, R, C, m, scale)


def ce_inputs(case, call=0):
    """scores, labels, mask, up.  Labels 0 and C-1 occur; random masks keep
    the label columns of a client live or not as they fall; 'label_only'
    needs one label per client, so every sample of a client shares it."""
    (N, R, C), variant, scale = case
    gen = torch.Generator().manual_seed(1000 * N + 10 * C + R + 7919 * call)
    scores = torch.randn(N, R, C, generator=gen) * scale
    labels = torch.randint(0, C, (N, R), generator=gen)
    labels[0, :] = 0
    labels[-1, :] = C - 1
    mask = None
    if variant == 'random':
        mask = (torch.rand(R, C, generator=gen) > 0.4).float()
    elif variant == 'label_only':
        lab = torch.randint(0, C, (R,), generator=gen)
        lab[0] = C - 1
        labels = lab.unsqueeze(0).expand(N, R).contiguous()
        mask = torch.zeros(R, C).scatter_(1, lab.unsqueeze(1), 1.0)
    up = torch.rand(R, generator=gen) + 0.25 + torch.arange(R)
    return scores, labels, mask, up


# =============================================================== head cases
# (N, R, C, H, W, J)
HEAD_CASES = [(10, 5, 512, 4, 4, 10), (3, 2, 20, 1, 1, 7),
              (37, 2, 512, 2, 2, 100), (2, 3, 5, 2, 3, 4), (4, 1, 1, 2, 2, 1)]
HEAD_LDS_CASE = (170, 1, 8, 1, 1, 100)   # N * J * 4 = 68000 > 64 KB


def head_case_id(case):
    return 'x'.join(map(str, case))


def head_inputs(case, io_name, bias=True):
    N, R, C, H, W, J = case
    gen = torch.Generator().manual_seed(N * 1000 + C + J)
    feat = torch.randn(N, R * C, H, W, generator=gen).to(IO_DTYPES[io_name])
    w = torch.randn(R, J, C, generator=gen) / max(C, 1) ** 0.5
    b = torch.randn(R, J, generator=gen) if bias else None
    ds = torch.randn(N, R, J, generator=gen)
    return feat, w, b, ds


# =========================================================== clip+SGD cases
SGD_R = 3
SGD_PER = [288, 10, 1, 4100, 4099, 2052, 4096, 4097, 8191]
SGD_SHADOWS = {0: 'aligned', 3: 'aligned', 5: 'offset2'}   # index into PER
SGD_NORMS = (50.0, 0.1, 0.0)      # clipped, not clipped, all-zero gradient
SGD_HYPER = dict(max_norm=1.0, lr=0.1, mom=0.9, wd=5e-4)
SGD_STEPS = 2


def sgd_inputs():
    """params, grads[step], bufs (zeros) as flat fp32 tensors of R * per
    elements; client r's gradient over all tensors has norm SGD_NORMS[r]."""
    gen = torch.Generator().manual_seed(5)
    R = SGD_R
    params = [torch.randn(R * per, generator=gen) for per in SGD_PER]
    bufs = [torch.zeros(R * per) for per in SGD_PER]
    grads = []
    for _ in range(SGD_STEPS):
        gs = [torch.randn(R, per, generator=gen).double() for per in SGD_PER]
        norm = torch.sqrt(sum((g * g).sum(1) for g in gs))
        want = torch.tensor(SGD_NORMS, dtype=torch.float64)
        grads.append([(g * (want / norm).unsqueeze(1)).float().reshape(-1)
                      for g in gs])
    return params, grads, bufs
