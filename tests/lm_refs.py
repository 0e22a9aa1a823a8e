"""Plain-torch references for the LM training kernels (attention.hip,
layernorm.hip, lm_ce.hip, lm_fused.hip).

Every function takes a `dtype` (torch.float64 for the oracle, torch.float32
to measure what fp32 arithmetic alone costs) and runs on whatever device its
inputs live on.  The attention emulations round where the kernels round
(read from attention.hip):

  small-S path (attn_fwd_kernel / attn_bwd_kernel)
    q, k, v, dO -> bf16;  P = bf16(softmax(Q K^T * inv_temp));  out = P V
    dP = dO V^T;  rd = sum_j dP*P;  dS = bf16(P (dP - rd) inv_temp)
    dQ = dS K;  dK = dS^T Q;  dV = P^T dO
  blockwise path (attn_fwd_block_kernel, attn_bwd_{d,dq,dkv}_kernel)
    same input rounding; 64-row KV blocks with running max m and sum l;
    P~ = bf16(exp(s - m_run)) feeds the MFMA while l sums the unrounded
    exponentials;  out = acc / l;  lse = m + log l
    D = rowsum(dO * out) with dO as given and out as stored (io dtype)
    P = bf16(exp(s - lse));  dS = bf16(P (dP - D) inv_temp)
  inv_temp is the fp32 value of 1/temperature in both.

Accumulation is in `dtype`; MFMA accumulates in fp32, so the fp32 run of an
emulation has the kernel's kind of arithmetic error, and the fp32-vs-fp64
spread of an emulation (ATTN_SPREAD below) is the yardstick the GPU tests'
tolerances hang on.
"""
import math

import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8     # relative error of one round-to-nearest bf16 rounding
KV_BLOCK = 64          # SMAX of attention.hip


def bf16r(x):
    """Round to bf16, keep the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (fp64 tensor in, fp64 out)."""
    _, ex = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 8)


def rel_fro(a, ref):
    """||a - ref||_F / ||ref||_F in fp64 (0/0 -> 0)."""
    a, ref = a.double(), ref.double()
    den = ref.norm().item()
    num = (a - ref).norm().item()
    return num / den if den > 0 else (0.0 if num == 0 else float('inf'))


def max_abs(a, ref):
    return (a.double() - ref.double()).abs().max().item()


def _inv_temp(temperature, dtype):
    return torch.tensor(1.0 / temperature, dtype=torch.float32).to(dtype).item()


# ------------------------------------------------------------- attention
def attn_exact(q, k, v, dout, temperature, dtype=torch.float64):
    """softmax(Q K^T / temperature) V and its gradients through autograd, no
    rounding anywhere."""
    q, k, v = (t.detach().to(dtype).clone().requires_grad_(True)
               for t in (q, k, v))
    out = torch.softmax(q @ k.transpose(1, 2) / temperature, dim=-1) @ v
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.to(dtype))
    return {'out': out.detach(), 'dq': dq, 'dk': dk, 'dv': dv}


def attn_small_emul(q, k, v, dout, temperature, dtype=torch.float64):
    """attn_fwd_kernel + attn_bwd_kernel with their rounding points."""
    it = _inv_temp(temperature, dtype)
    qb, kb, vb, gb = (bf16r(t.detach().to(dtype)) for t in (q, k, v, dout))
    s = (qb @ kb.transpose(1, 2)) * it
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    P = bf16r(e * (1.0 / e.sum(-1, keepdim=True)))
    out = P @ vb
    dP = gb @ vb.transpose(1, 2)
    rd = (dP * P).sum(-1, keepdim=True)
    t = P * (dP - rd) * it
    dS = bf16r(t)
    return {'out': out, 'dq': dS @ kb, 'dk': dS.transpose(1, 2) @ qb,
            'dv': P.transpose(1, 2) @ gb,
            # what attn_rounding_bound needs
            'P': P, 't': t, 'dD': U_BF16 * (P * dP.abs()).sum(-1), 'it': it,
            'q': qb, 'k': kb, 'v': vb, 'g': gb}


def attn_block_emul(q, k, v, dout, temperature, dtype=torch.float64,
                    io_dtype=torch.float32):
    """attn_fwd_block_kernel + the three blockwise backward kernels."""
    it = _inv_temp(temperature, dtype)
    qb, kb, vb, gb = (bf16r(t.detach().to(dtype)) for t in (q, k, v, dout))
    g_raw = dout.detach().to(io_dtype).to(dtype)
    B, S, d = qb.shape
    m = torch.full((B, S), -1e30, dtype=dtype, device=qb.device)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(qb)
    for j0 in range(0, S, KV_BLOCK):
        j1 = min(S, j0 + KV_BLOCK)
        sb = (qb @ kb[:, j0:j1].transpose(1, 2)) * it
        mx = torch.maximum(m, sb.max(-1).values)
        scale = torch.exp(m - mx)
        e = torch.exp(sb - mx.unsqueeze(-1))
        l = l * scale + e.sum(-1)
        acc = acc * scale.unsqueeze(-1) + bf16r(e) @ vb[:, j0:j1]
        m = mx
    out = acc / l.unsqueeze(-1)
    lse = m + torch.log(l)
    out_st = out.to(io_dtype).to(dtype)
    D = (g_raw * out_st).sum(-1, keepdim=True)
    s = (qb @ kb.transpose(1, 2)) * it
    P = bf16r(torch.exp(s - lse.unsqueeze(-1)))
    dP = gb @ vb.transpose(1, 2)
    t = P * (dP - D) * it
    dS = bf16r(t)
    # |D - rowsum(dP * P_exact)|: out is off by one P~ rounding (and one
    # output rounding when stored as bf16), and D reads dO unrounded while
    # dP reads bf16(dO)
    vmax = vb.abs().amax(dim=(1, 2), keepdim=True)
    io_u = U_BF16 if io_dtype == torch.bfloat16 else 0.0
    dD = (g_raw.abs() * (U_BF16 * vmax + io_u * out.abs())
          + (g_raw - gb).abs() * out.abs()).sum(-1)
    return {'out': out, 'lse': lse, 'dq': dS @ kb,
            'dk': dS.transpose(1, 2) @ qb, 'dv': P.transpose(1, 2) @ gb,
            'P': P, 't': t, 'dD': dD, 'it': it,
            'q': qb, 'k': kb, 'v': vb, 'g': gb}


def attn_rounding_bound(em, io_dtype=torch.float32):
    """First-order bound on what the bf16 roundings of P and dS can move each
    output, u = 2^-8 relative per rounding, from an emulation's own values:

      out : |d out_ic| <= sum_j u P_ij |v_jc|          <= u max|v|  (sum P = 1)
      dV  : |d dV_jc|  <= sum_i u P_ij |dO_ic|         <= u max_j(sum_i P_ij) max|dO|
      dS  : pre-rounding t = P (dP - D) inv_temp moves by u|t| (from P_ij)
            + P_ij inv_temp |dD_i| (from the row term D or rd), and is then
            rounded itself: |d dS_ij| <= G_ij = 2u|t_ij| + inv_temp P_ij dD_i
      dQ  : |d dQ_ic|  <= sum_j G_ij |k_jc|            <= max_i(sum_j G_ij) max|k|
      dK  : |d dK_jc|  <= sum_i G_ij |q_ic|            <= max_j(sum_i G_ij) max|q|

    dD_i is u sum_j P_ij |dP_ij| on the small-S path and the D bound of
    attn_block_emul on the blockwise one.  For bf16 outputs half an ulp of
    the result (<= u |result|) is added.  The same expression bounds (a) an
    emulation against exact arithmetic on the same bf16 inputs and (b) two
    correct implementations of the same rounding scheme against each other:
    there an entry that lands on the other side of a rounding boundary moves
    by a whole ulp, 2u, but only entries within fp32 round-off of a boundary
    can, and the bound is reached only if half a row's mass does."""
    u = U_BF16
    P, t = em['P'].double(), em['t'].double().abs()
    G = 2 * u * t + em['it'] * P * em['dD'].double().unsqueeze(-1)
    amax = lambda x: x.double().abs().max().item()
    b = {'out': u * amax(em['v']),
         'dv': u * P.sum(1).max().item() * amax(em['g']),
         'dq': G.sum(2).max().item() * amax(em['k']),
         'dk': G.sum(1).max().item() * amax(em['q'])}
    if io_dtype == torch.bfloat16:
        for name in b:
            b[name] += u * amax(em[name])
    return b


# (path, B, S, d, temperature or None for sqrt(d), kind)
#   path : 'small' (S <= 64 kernels), 'block' (S > 64), 'block1' (the
#          blockwise kernels called directly at S <= 64)
#   kind : 'randn', 'stable' (scores reach +-60), 'stable_first' /
#          'stable_last' (the dominant keys sit in the first / last KV block)
ATTN_CASES = [
    ('small', 3, 64, 32, None, 'randn'),
    ('small', 3, 64, 2, None, 'randn'),
    ('small', 2, 63, 31, None, 'randn'),
    ('small', 2, 17, 5, None, 'randn'),
    ('small', 2, 1, 1, None, 'randn'),
    ('small', 2, 16, 8, None, 'randn'),
    ('small', 2, 63, 31, 7.3, 'randn'),
    ('small', 2, 64, 32, None, 'stable'),
    ('block', 2, 65, 32, None, 'randn'),
    ('block', 2, 128, 16, None, 'randn'),
    ('block', 2, 100, 5, None, 'randn'),
    ('block', 2, 129, 2, None, 'randn'),
    ('block', 2, 100, 5, 1.7, 'randn'),
    ('block', 2, 140, 32, None, 'stable_first'),
    ('block', 2, 140, 32, None, 'stable_last'),
    ('block1', 2, 64, 32, None, 'randn'),
    ('block1', 2, 17, 5, None, 'randn'),
]
IO_DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def attn_case_id(case):
    path, B, S, d, temp, kind = case
    return '{}-{}x{}x{}-t{}-{}'.format(path, B, S, d,
                                       'sqrt' if temp is None else temp, kind)


def attn_temperature(case):
    return float(case[3]) ** 0.5 if case[4] is None else float(case[4])


def attn_inputs(case, io_dtype):
    """Seeded CPU inputs (q, k, v, dO) of a case, in io_dtype.  The stable
    kinds are bf16-representable in fp32 too, so that the unquantised sanity
    reference sees the scores the kernel sees."""
    path, B, S, d, _, kind = case
    temp = attn_temperature(case)
    gen = torch.Generator().manual_seed(1000 * S + 10 * d + B)
    q, k, v, g = (torch.randn(B, S, d, generator=gen) for _ in range(4))
    if kind != 'randn':
        # a group of keys along u gets scores near +60 (spread over a few
        # units, so the softmax stays non-degenerate), one key gets -60
        u = torch.ones(d) / math.sqrt(d)
        amp = math.sqrt(60.0 * temp)
        first = kind != 'stable_last'
        group = list(range(3, 9)) if first else list(range(S - 7, S - 1))
        q = q + amp * u
        k[:, group] += amp * u
        k[:, 40 if S > 40 else 0] = -amp * u
        s = (bf16r(q) @ bf16r(k).transpose(1, 2)) / temp
        q = q * (60.0 / s.abs().amax(dim=(1, 2), keepdim=True))
        q, k, v, g = (bf16r(t) for t in (q, k, v, g))
    return tuple(t.to(io_dtype) for t in (q, k, v, g))


def attn_emul(case, tensors, dtype, io_dtype):
    fn = attn_small_emul if case[0] == 'small' else attn_block_emul
    kw = {} if case[0] == 'small' else {'io_dtype': io_dtype}
    return fn(*tensors, attn_temperature(case), dtype=dtype, **kw)


ATTN_OUTPUTS = ('out', 'dq', 'dk', 'dv')
# {(case id, 'fp32'|'bf16'): {output: (rel Frobenius, max abs)}} of the fp32
# emulation against the fp64 one.  Filled by attn_spread(); test_lm_refs.py
# fills and checks every entry.
ATTN_SPREAD = {}
# {'small'|'block': {output: (rel Frobenius, max abs)}}: per emulation and
# output, the largest entry of ATTN_SPREAD over the whole case list and both
# io dtypes.  This is the table the GPU tolerances hang on.  It is taken over
# the case list and not per case because a case's own spread is either pure
# fp32 round-off (~5e-8, no P or dS entry landed on the other side of a bf16
# rounding boundary) or one or more such flips (~1e-5 .. 5e-4): which of the
# two a small case shows is chance, a correct kernel flips other entries
# than the fp32 emulation does, and only the flips are what the margin is
# meant to cover.
ATTN_EMUL_SPREAD = {}


def attn_spread(case, io_name):
    key = (attn_case_id(case), io_name)
    if key not in ATTN_SPREAD:
        io = IO_DTYPES[io_name]
        x = attn_inputs(case, io)
        e64 = attn_emul(case, x, torch.float64, io)
        e32 = attn_emul(case, x, torch.float32, io)
        ATTN_SPREAD[key] = {n: (rel_fro(e32[n], e64[n]),
                                max_abs(e32[n], e64[n]))
                            for n in ATTN_OUTPUTS}
    return ATTN_SPREAD[key]


def attn_emul_spread(path):
    """ATTN_EMUL_SPREAD row of the emulation that `path` is compared with."""
    emul = 'small' if path == 'small' else 'block'
    if emul not in ATTN_EMUL_SPREAD:
        rows = [attn_spread(c, io) for c in ATTN_CASES for io in IO_DTYPES
                if (c[0] == 'small') == (emul == 'small')]
        ATTN_EMUL_SPREAD[emul] = {
            n: (max(r[n][0] for r in rows), max(r[n][1] for r in rows))
            for n in ATTN_OUTPUTS}
    return ATTN_EMUL_SPREAD[emul]


# ------------------------------------------------------------- layernorm
def layernorm_ref(x, gamma, beta, dy, eps=1e-5, dtype=torch.float64):
    """Per-client LayerNorm over the last dim: x (R, B, S, E), gamma/beta
    (R, E).  torch's own F.layer_norm in `dtype`; returns y, dx, dgamma,
    dbeta."""
    R, E = gamma.shape
    x, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True)
                      for t in (x, gamma, beta))
    y = F.layer_norm(x, (E,), None, None, eps) * gamma.view(R, 1, 1, E) \
        + beta.view(R, 1, 1, E)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy.to(dtype))
    return {'y': y.detach(), 'dx': dx, 'dgamma': dg, 'dbeta': db}


# ------------------------------------------------------------------ lm_ce
def lm_ce_ref(logits, tokens, mask, w, dtype=torch.float64):
    """Vocab-masked CE: logits (R, B, S, V), tokens (R, B, S), mask (R, V) or
    None, w (R,) upstream gradient of the per-client mean NLL.  Masked logits
    become 0 (not -inf) and still take part in the softmax."""
    R, V = logits.size(0), logits.size(-1)
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    z = x if mask is None else \
        x.masked_fill(mask.view(R, 1, 1, V) == 0, 0)
    logp = F.log_softmax(z, dim=-1)
    losses = -logp.gather(3, tokens.unsqueeze(3)).squeeze(3) \
        .reshape(R, -1).mean(1)
    (dx,) = torch.autograd.grad(losses, x, w.to(dtype))
    return {'losses': losses.detach(), 'dlogits': dx}


# ------------------------------------------------------------ dropout glue
def gelu_drop_ref(x, keep, dy, rate, p, dtype=torch.float64):
    """y = keep * gelu(x / rate) / (1 - p) and dx, erf-form GELU."""
    v = x.detach().to(dtype) / rate
    k = keep.to(dtype)
    cdf = 0.5 * (1 + torch.erf(v / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    return {'y': k * v * cdf / (1 - p),
            'dx': dy.to(dtype) * k * (cdf + v * pdf) / (rate * (1 - p))}


def res_drop_ref(src, h, keep, dt, rate, p, dtype=torch.float64):
    """t = src + keep * h / (rate (1 - p)); dsrc = dt; dh = dt keep / (...)"""
    k = keep.to(dtype) / (rate * (1 - p))
    return {'t': src.detach().to(dtype) + k * h.detach().to(dtype),
            'dsrc': dt.to(dtype), 'dh': dt.to(dtype) * k}


# --------------------------------------------------------------- embed_pos
def embed_pos_ref(ids, table, pos, dy, rate, dtype=torch.float64):
    """out[r,b,s] = (table[r, ids[r,b,s]] + pos[r, s]) / rate and the
    gradients of both tables: table (R, V, E), pos (R, P, E), P >= S."""
    R, B, S = ids.shape
    table, pos = (t.detach().to(dtype).clone().requires_grad_(True)
                  for t in (table, pos))
    r = torch.arange(R, device=ids.device).view(R, 1, 1)
    s = torch.arange(S, device=ids.device).view(1, 1, S)
    out = (table[r, ids] + pos[r, s]) / rate
    dt, dp = torch.autograd.grad(out, (table, pos), dy.to(dtype))
    return {'out': out.detach(), 'dtable': dt, 'dpos': dp}
