"""Autograd wrappers for the hand-written gfx950 kernels, with pure-torch
reference implementations (the CPU path and the numerics oracle in tests).

Semantics mirrored from the reference:
- Scaler -> norm -> ReLU prefix of every block (src/models/resnet.py:44-50,
  src/models/conv.py:29-33).  With a train-mode norm the Scaler division
  cancels exactly (norm(x/r) == norm(x)), so the fused kernels omit it; the
  eager path keeps the explicit division as the oracle.
- masked cross-entropy (src/models/resnet.py:152-157).
- per-client clip(1.0) + momentum-SGD (src/train_classifier_fed.py:205-206).
"""
import torch
import torch.nn.functional as F

from . import require_native, use_native, large_conv_enabled


class _FusedNormReLU(torch.autograd.Function):
    """y = relu(norm(x) * w + b) with batch (kind='bn') or group stats."""

    @staticmethod
    def forward(ctx, x, weight, bias, kind, groups, eps):
        ext = require_native()
        x = x.contiguous()
        if kind == 'bn':
            y, mean, invstd = ext.bn_relu_fwd(x, weight, bias, eps)
        else:
            y, mean, invstd = ext.gn_relu_fwd(x, weight, bias, groups, eps)
        ctx.save_for_backward(x, weight, bias, mean, invstd)
        ctx.kind = kind
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        x, weight, bias, mean, invstd = ctx.saved_tensors
        if ctx.kind == 'bn':
            dx, dgamma, dbeta = ext.bn_relu_bwd(dy, x, weight, bias, mean,
                                                invstd)
        else:
            dx, dgamma, dbeta = ext.gn_relu_bwd(dy, x, weight, bias, mean,
                                                invstd, ctx.groups)
        return dx, dgamma, dbeta, None, None, None


def fused_norm_relu(x, weight, bias, kind, groups=1, eps=1e-5):
    return _FusedNormReLU.apply(x, weight, bias, kind, groups, eps)


class _FusedNormReLUAlias(torch.autograd.Function):
    """BN+ReLU that also hands its input back: (y, x_alias) = f(x).  A block
    without a shortcut conv uses x_alias as its residual, so x has this one
    consumer and the residual branch's gradient arrives here as dx_alias and
    is added inside the BN backward kernel's dx store (bn_relu_bwd_add)
    instead of by the autograd engine in a launch of its own.  The sum has
    the bits of that separate add.  Off the GPU the same function runs in
    torch ops (the oracle of the wiring and of gradcheck)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ctx.set_materialize_grads(False)
        ctx.native = use_native(x)
        if ctx.native:
            ext = require_native()
            xc = x.contiguous()
            y, mean, invstd = ext.bn_relu_fwd(xc, weight, bias, eps)
        else:
            xc = x
            mean = x.mean(dim=(0, 2, 3))
            var = x.var(dim=(0, 2, 3), unbiased=False)
            invstd = (var + eps).rsqrt()
            cv = (1, -1, 1, 1)
            y = F.relu((x - mean.view(cv)) * (invstd * weight).view(cv)
                       + bias.view(cv))
        ctx.save_for_backward(xc, weight, bias, mean, invstd)
        return y, x

    @staticmethod
    def backward(ctx, dy, dalias):
        x, weight, bias, mean, invstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(x)
        if ctx.native:
            ext = require_native()
            if dalias is None:
                dx, dgamma, dbeta = ext.bn_relu_bwd(dy, x, weight, bias, mean,
                                                    invstd)
            else:
                dx, dgamma, dbeta = ext.bn_relu_bwd_add(
                    dy, x, weight, bias, mean, invstd, dalias.to(x.dtype))
            return dx, dgamma, dbeta, None
        cv = (1, -1, 1, 1)
        M = x.numel() // x.size(1)
        xh = (x - mean.view(cv)) * invstd.view(cv)
        pre = xh * weight.view(cv) + bias.view(cv)
        d = torch.where(pre > 0, dy, torch.zeros_like(dy))
        dbeta = d.sum((0, 2, 3))
        dgamma = (d * xh).sum((0, 2, 3))
        dx = (weight * invstd).view(cv) * (d - (dbeta / M).view(cv)
                                           - xh * (dgamma / M).view(cv))
        if dalias is not None:
            dx = dx + dalias
        return dx, dgamma, dbeta, None


def fused_norm_relu_alias(x, weight, bias, eps=1e-5):
    """(relu(bn(x) * w + b), x_alias): see _FusedNormReLUAlias."""
    return _FusedNormReLUAlias.apply(x, weight, bias, eps)


def bn_relu_route(direction, N, C, HW, elem_size, aligned=True):
    """Route bn_relu_fwd / bn_relu_bwd (direction 'fwd' / 'bwd') take for an
    (N, C, HW) tensor of elem_size bytes per element; the launchers' own rule,
    nothing is launched.  'vec': the staged kernel with 16-byte global and
    LDS accesses (HW * elem_size a multiple of 16, every base 16-byte
    aligned - pass aligned=False for a view that is not;
    HETEROFL_STREAM_VEC=0 turns it off); 'staged': the element-wise staged
    kernel; 'direct': the channel is over the 64 KB LDS stage; 'split3': the
    large-batch 3-kernel forward."""
    ext = require_native()
    return ext.bn_relu_route(direction, N, C, HW, elem_size, aligned)


def eager_scaler_norm_relu(x, weight, bias, kind, groups, rate, eps=1e-5):
    """Reference path: scaler -> norm -> relu with explicit torch ops."""
    if rate != 1.0:
        x = x / rate
    if kind == 'bn':
        x = F.batch_norm(x, None, None, weight, bias, training=True, eps=eps)
    else:
        x = F.group_norm(x, groups, weight, bias, eps=eps)
    return F.relu(x)


class _FusedMaskedCE(torch.autograd.Function):
    """Per-client mean masked-CE over scores (N, R, C); optionally
    accumulates (sum-loss, correct, count) into a device metrics buffer."""

    @staticmethod
    def forward(ctx, scores, labels, mask, metrics):
        ext = require_native()
        scores = scores.contiguous().float()
        (losses,) = ext.masked_ce_fwd(
            scores, labels.contiguous(),
            mask if mask is not None else torch.Tensor(),
            metrics if metrics is not None else torch.Tensor())
        ctx.save_for_backward(scores, labels,
                              mask if mask is not None else torch.Tensor())
        ctx.has_mask = mask is not None
        return losses

    @staticmethod
    def backward(ctx, up):
        ext = require_native()
        scores, labels, mask = ctx.saved_tensors
        dscores = ext.masked_ce_bwd(scores, labels,
                                    mask if ctx.has_mask else torch.Tensor(),
                                    up)
        return dscores, None, None, None


def fused_masked_ce(scores, labels, mask=None, metrics=None):
    return _FusedMaskedCE.apply(scores, labels, mask, metrics)


class FusedClipSGD:
    """Chunk-table driven per-client clip + momentum-SGD over the batched
    model's parameters.  Build once per captured graph (pointer stability is
    guaranteed by holding refs to grads/params/bufs)."""

    CHUNK = 65536

    def __init__(self, params, grads, bufs, R, device, shadows=None):
        ext = require_native()
        self.params = list(params)
        self.grads = list(grads)
        self.bufs = list(bufs)
        self.shadows = [s if s is not None else torch.Tensor()
                        for s in (shadows or [])]
        blob, n, clients = ext.build_chunk_table(
            self.grads, self.params, self.bufs, R, self.CHUNK, self.shadows)
        self.table = blob
        self.n_chunks = int(n.item())
        self.chunk_client = clients
        self.partials = torch.zeros(self.n_chunks, dtype=torch.float32,
                                    device=device)
        self.normsq = torch.zeros(R, dtype=torch.float32, device=device)

    def step(self, max_norm, lr, momentum, weight_decay):
        ext = require_native()
        ext.clip_sgd_step(self.table, self.n_chunks, self.chunk_client,
                          self.partials, self.normsq, max_norm, lr, momentum,
                          weight_decay)


class _GroupedConv(torch.autograd.Function):
    """MFMA implicit-GEMM grouped conv (ops/csrc/conv_mfma.hip): bf16/fp32
    activations, fp32 master weights, fp32 weight gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, groups, stride, pad):
        from . import fp8_enabled
        ext = require_native()
        fp8 = 1 if fp8_enabled() else 0
        x = x.contiguous()
        y = ext.conv_fwd(x, weight,
                         bias if bias is not None else torch.Tensor(),
                         residual.contiguous() if residual is not None
                         else torch.Tensor(),
                         groups, stride, pad, fp8)
        ctx.save_for_backward(x, weight)
        ctx.meta = (groups, stride, pad, bias is not None, fp8)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        x, w = ctx.saved_tensors
        groups, stride, pad, has_bias, fp8 = ctx.meta
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ext.conv_bwd_data(dy, w, groups, stride, pad,
                                   x.size(2), x.size(3), fp8)
        if ctx.needs_input_grad[1]:
            dw = ext.conv_bwd_weight(dy, x, groups, stride, pad, w.size(2),
                                     fp8)
        if has_bias and ctx.needs_input_grad[2]:
            db = dy.float().sum(dim=(0, 2, 3))
        # residual gradient is dy itself (identity add in the epilogue)
        dres = dy if ctx.needs_input_grad[3] else None
        return dx, dw, db, dres, None, None, None


def grouped_conv(x, weight, bias, groups, stride, pad, residual=None):
    from . import fp8_enabled
    if large_conv_enabled() and groups == 1 and x.dtype == torch.bfloat16 \
            and not fp8_enabled() and not (torch.is_grad_enabled() and (
                x.requires_grad or weight.requires_grad
                or (bias is not None and bias.requires_grad)
                or (residual is not None and residual.requires_grad))) \
            and large_conv_route(x.size(0), weight.size(1), x.size(2),
                                 x.size(3), weight.size(0), weight.size(2),
                                 stride, pad):
        # forward-only large-batch route; the weight is packed per call here
        # (NativeInference packs once per model instead)
        return conv_fwd_large(x, conv_pack_weight(weight.detach()),
                              None if bias is None else bias.detach(),
                              residual, stride, pad, weight.size(1),
                              weight.size(0), weight.size(2))
    return _GroupedConv.apply(x, weight, bias, residual, groups, stride, pad)


def conv_plan(direction, G, N, Cin, H, W, Cout, khw, stride, pad, elem_size,
              fp8):
    """(route, split, dyn_lds_bytes) that conv_fwd / conv_bwd_data /
    conv_bwd_weight (direction 'fwd' / 'bwd_data' / 'bwd_weight') take for
    this shape; the launchers' own plan functions, nothing is launched.
    route is 'resident', 'staged', 'gather' or 'gather_s2', with '_fp8'
    appended where the fp8 tile instantiation runs."""
    ext = require_native()
    return ext.conv_plan(direction, G, N, Cin, H, W, Cout, khw, stride, pad,
                         elem_size, fp8)


def conv_plan_variant(direction, G, N, Cin, H, W, Cout, khw, stride, pad,
                      elem_size, fp8):
    """Name of the kernel that launcher would launch for this shape, e.g.
    'conv_fwd_tabled_kernel' or 'conv_bwd_data_s2_kernel' ('<fp8>' appended
    for the fp8 tile instantiation).  Tells the tabled gather kernels
    (HETEROFL_CONV_TABLED, on by default) from the untabled ones, which
    conv_plan's route string does not."""
    ext = require_native()
    return ext.conv_plan_variant(direction, G, N, Cin, H, W, Cout, khw,
                                 stride, pad, elem_size, fp8)


# ------------------------------------------------- large-batch inference ops
def large_conv_supported(k, stride, pad):
    """Shapes conv_fwd_large implements: 3x3/pad 1 and 1x1/pad 0, stride 1
    or 2."""
    return ((k == 3 and pad == 1) or (k == 1 and pad == 0)) \
        and stride in (1, 2)


def large_conv_route(N, Cin, H, W, Cout, k, stride, pad):
    """Router: a shape goes to conv_fwd_large only where that kernel
    measured faster than conv_fwd (profiles/inferbench.txt, both tables).
    Between the measured shapes a two-line cost model fitted to those tables
    decides:
      conv_fwd        ~50 TFLOP/s on its 64-row tile (Cout rounds up to 64);
      conv_fwd_large  a latency floor of 15 us + 1.2 us per K-slab, and
                      ~150 TFLOP/s on its padded problem (cin rounds up to
                      32 per tap, Cout to its 64- or 128-row tile).
    The model is conservative: every measured shape it routes measured
    faster on the large kernel; some marginal wins (within ~1.4x) stay on
    conv_fwd."""
    if not large_conv_supported(k, stride, pad):
        return False
    OH = (H + 2 * pad - k) // stride + 1
    OW = (W + 2 * pad - k) // stride + 1
    P = N * OH * OW
    slabs = k * k * ((Cin + 31) // 32)
    old_us = 2.0 * P * (-(-Cout // 64) * 64) * Cin * k * k / 50e6
    cout_pad = 64 if Cout <= 64 else -(-Cout // 128) * 128
    large_us = max(15.0 + 1.2 * slabs,
                   2.0 * P * cout_pad * 32 * slabs / 150e6)
    return old_us > large_us


def conv_pack_weight(weight):
    """One-time tap-major bf16 repack of an (Cout, Cin, k, k) weight for
    conv_fwd_large."""
    ext = require_native()
    return ext.conv_pack_weight(weight.contiguous())


def conv_fwd_large(x, packed, bias, residual, stride, pad, Cin, Cout, k):
    """Forward-only groups=1 conv on bf16 NCHW with a packed weight; bias
    (fp32) and residual (bf16) are applied in the epilogue."""
    ext = require_native()
    return ext.conv_fwd_large(
        x.contiguous(), packed,
        bias.float().contiguous() if bias is not None else torch.Tensor(),
        residual.contiguous() if residual is not None else torch.Tensor(),
        stride, pad, Cin, Cout, k)


def bn_relu_infer(x, scale, shift):
    """relu(x * scale[c] + shift[c]) — eval-mode BN+ReLU with the running
    statistics folded into scale/shift (fold_bn).  HIP kernel on GPU, torch
    on CPU."""
    if use_native(x):
        ext = require_native()
        return ext.bn_relu_infer(x.contiguous(), scale.float().contiguous(),
                                 shift.float().contiguous())
    shape = [1, -1] + [1] * (x.dim() - 2)
    y = x.float() * scale.view(shape) + shift.view(shape)
    return F.relu(y).to(x.dtype)


def fold_bn(weight, bias, mean, var, eps=1e-5):
    """scale = w*rsqrt(var+eps), shift = b - mean*scale (fp32)."""
    scale = weight.float() * torch.rsqrt(var.float() + eps)
    return scale, bias.float() - mean.float() * scale


def eval_metrics(scores, labels, user_ptr, user_samples, label_mask):
    """Per-user Local and the Global evaluation sums from one logit matrix.

    scores (N, C) fp32, labels (N,), users as CSR (user_ptr (U+1,),
    user_samples (nnz,)), label_mask (U, C) in {0, 1}.  Returns
    (local (U, 3), global (3,)), each row (loss sum, correct count, sample
    count).  Local rows use the reference's mask-then-CE order (masked logits
    are 0, models/functional.py); the Global row uses the raw logits.  The
    prediction is the lowest index holding the maximum."""
    scores = scores.float().contiguous()
    labels = labels.long().contiguous()
    user_ptr = user_ptr.long().contiguous()
    user_samples = user_samples.long().contiguous()
    label_mask = label_mask.float().contiguous()
    if use_native(scores):
        ext = require_native()
        local, glob = ext.eval_metrics(scores, labels, user_ptr, user_samples,
                                       label_mask)
        return local, glob
    U = user_ptr.numel() - 1
    C = scores.size(1)
    counts = user_ptr[1:] - user_ptr[:-1]
    owner = torch.repeat_interleave(torch.arange(U, device=scores.device),
                                    counts)

    def terms(sc, y):
        nll = F.cross_entropy(sc, y, reduction='none')
        mx = sc.max(dim=1, keepdim=True).values
        cls = torch.arange(C, device=sc.device).expand_as(sc)
        pred = torch.where(sc == mx, cls, torch.full_like(cls, C)).min(1).values
        return torch.stack([nll, (pred == y).float(),
                            torch.ones_like(nll)], 1)

    sc = scores[user_samples].masked_fill(label_mask[owner] == 0, 0)
    local = torch.zeros(U, 3, dtype=torch.float32, device=scores.device)
    if owner.numel():
        local.index_add_(0, owner, terms(sc, labels[user_samples]))
    glob = terms(scores, labels).sum(0) if scores.size(0) else \
        torch.zeros(3, device=scores.device)
    return local, glob


# ------------------------------------------------ LM evaluation head (K7/K10)
LM_HEAD_KPAD = 32   # E padding of the packed head (MFMA K)
LM_HEAD_VPAD = 64   # V padding of the packed head (column tile)


def lm_head_pack(weight, bias=None):
    """One-time repack of the decoder's vocabulary projection (V, E) for
    lm_head_ce: E zero-padded to a multiple of 32, V to a multiple of 64.
    bf16 from the HIP kernel on GPU; on CPU the same layout in fp32 (the
    oracle path does not round).  `bias` is only checked against V: it stays
    fp32 and is handed to lm_head_ce as it is."""
    V, E = weight.shape
    if bias is not None and tuple(bias.shape) != (V,):
        raise ValueError('lm_head_pack: bias must be (V,)')
    if not 1 <= E <= 256:
        raise ValueError('lm_head_pack: 1 <= E <= 256')
    if use_native(weight):
        ext = require_native()
        return ext.lm_head_pack(weight.detach().float().contiguous())
    Vp = -(-V // LM_HEAD_VPAD) * LM_HEAD_VPAD
    Ep = -(-E // LM_HEAD_KPAD) * LM_HEAD_KPAD
    out = torch.zeros(Vp, Ep, dtype=torch.float32, device=weight.device)
    out[:V, :E] = weight.detach().float()
    return out


def lm_head_ce(x, packed, bias, labels, vocab_mask, V, E, splits=0):
    """Vocabulary projection fused with cross-entropy: x (M, E), packed from
    lm_head_pack, bias (V,) fp32 or None, labels (M,) int64 in [0, V),
    vocab_mask (V,) fp32 or None -> (row_nll (M,), row_lse (M,)) fp32.

    logit = x . W^T + b in fp32; a vocab-masked column's logit is exactly 0
    (bias included) and still takes part in the softmax, as in
    models/functional.py; the (M, V) logits are never written on the GPU
    path (ops/csrc/lm_head.hip, KC = 0, bf16 x).  `splits` cuts the
    vocabulary over that many blocks per row tile (0: the host fills the
    GPU); for a given value the result is bit-reproducible."""
    if use_native(x):
        ext = require_native()
        none = torch.Tensor()
        nll, lse = ext.lm_head_ce(
            x.contiguous(), packed,
            bias.float().contiguous() if bias is not None else none,
            labels.long().contiguous(),
            vocab_mask.float().contiguous() if vocab_mask is not None
            else none, V, E, splits)
        return nll, lse
    logits = x.float() @ packed[:V, :E].float().t()
    if bias is not None:
        logits = logits + bias.float()
    if vocab_mask is not None:
        logits = logits.masked_fill(vocab_mask.view(1, V) == 0, 0)
    lse = torch.logsumexp(logits, dim=1)
    return lse - logits.gather(1, labels.long().view(-1, 1)).squeeze(1), lse


LM_HEAD_MAX_K = 8   # capacity of lm_head_topk's per-lane lists


def lm_head_topk(x, packed, bias, labels, vocab_mask, V, E, k, splits=0):
    """Vocabulary projection fused with top-k: x (M, E), packed from
    lm_head_pack, bias (V,) fp32 or None, labels (M,) int64 or None,
    vocab_mask (V,) fp32 or None, 1 <= k <= min(8, V) -> (top_val (M, k)
    fp32, top_idx (M, k) int64, row_lse (M,) fp32, row_nll (M,) fp32; empty
    without labels).

    The logits are lm_head_ce's (fp32, a vocab-masked column exactly 0 and
    still a candidate, padded columns never returned).  Row i holds its k
    largest logits in descending order, among equal logits the lower column
    first; log-probabilities are top_val - row_lse[:, None].  On the GPU one
    pass over the vocabulary keeps a running top-k next to the running
    log-sum-exp (ops/csrc/lm_head.hip, lm_head_ce's kernel with per-lane
    lists of capacity KC >= k); `splits` as in lm_head_ce, and
    for a given value the four outputs are bit-reproducible.  On the CPU, and
    under HETEROFL_FORCE_EAGER=1, fp32 logits and a stable descending sort:
    the numerics oracle.

    Measured on MI355X (profiles/lm_inferbench.txt, V = 33278, E in {256,
    64, 16}, M in {640, 32768}): 1.11x - 1.30x of lm_head_ce's time at k = 1,
    1.78x - 2.83x at k = 5, 2.45x - 4.63x at k = 8, and 0.05x - 0.61x of the
    two-step bf16 F.linear + torch.topk + lm_ce_fwd at every point, which is
    why there is no router next to lm_head_route for it."""
    if not 1 <= k <= min(LM_HEAD_MAX_K, V):
        raise ValueError('lm_head_topk: 1 <= k <= 8 and k <= V, got k={} '
                         'for V={}'.format(k, V))
    if use_native(x):
        ext = require_native()
        none = torch.Tensor()
        val, idx, lse, nll = ext.lm_head_topk(
            x.contiguous(), packed,
            bias.float().contiguous() if bias is not None else none,
            labels.long().contiguous() if labels is not None else none,
            vocab_mask.float().contiguous() if vocab_mask is not None
            else none, V, E, k, splits)
        return val, idx, lse, nll
    logits = x.float() @ packed[:V, :E].float().t()
    if bias is not None:
        logits = logits + bias.float()
    if vocab_mask is not None:
        logits = logits.masked_fill(vocab_mask.view(1, V) == 0, 0)
    lse = torch.logsumexp(logits, dim=1)
    nll = logits.new_empty(0)
    if labels is not None:
        nll = lse - logits.gather(1, labels.long().view(-1, 1)).squeeze(1)
    # torch.sort(logits, descending=True, stable=True)[:, :k], with the
    # columns under the row's k-th value dropped before the sort (they can
    # not be returned, and sorting the whole vocabulary costs seconds per
    # window set).  nonzero lists the rest by row, then ascending column;
    # two stable sorts order them by row, then value descending, and keep
    # the ascending columns among equal values.
    kth = torch.topk(logits, k, dim=1).values[:, -1:]
    keep = logits >= kth
    row, col = keep.nonzero(as_tuple=True)
    v = logits[row, col]
    o = torch.sort(v, descending=True, stable=True).indices
    o = o[torch.sort(row[o], stable=True).indices]
    first = keep.sum(1).cumsum(0) - keep.sum(1)
    pick = o[first.view(-1, 1) + torch.arange(k, device=x.device)]
    return v[pick], col[pick], lse, nll


def lm_head_route(M, E, V):
    """Router of NativeLMInference(head='auto'): True sends the head to
    lm_head_ce, False to the two-step bf16 F.linear + lm_ce_fwd.  The sweep
    in profiles/lm_inferbench.txt (V = 33278, E in {256, 64, 16}, M in {640,
    32768}) measured the fused kernel at 0.16x - 0.64x of the two-step time
    at every point, so that envelope is routed: at least one full window of
    rows and at least the WikiText2 vocabulary (more rows or more columns
    only lengthen the loops the kernel amortises its prologue over).
    Smaller problems were not measured and stay on the two-step head."""
    return M >= 640 and V >= 33278 and E <= 256


class _FusedHead(torch.autograd.Function):
    """AdaptiveAvgPool(1) + flatten + per-client Linear in one kernel each
    way (ops/csrc/head.hip).  scores come back fp32 (they feed masked-CE)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, R):
        ext = require_native()
        feat = feat.contiguous()
        scores, pooled = ext.head_fwd(feat, weight,
                                      bias if bias is not None
                                      else torch.Tensor(), R)
        ctx.save_for_backward(pooled, weight)
        ctx.meta = (R, feat.size(2), feat.size(3),
                    feat.dtype == torch.bfloat16, bias is not None)
        return scores

    @staticmethod
    def backward(ctx, dscores):
        ext = require_native()
        pooled, weight = ctx.saved_tensors
        R, H, W, bf16_feat, has_bias = ctx.meta
        dw, db, dfeat = ext.head_bwd(dscores.contiguous().float(), pooled,
                                     weight, R, H, W, bf16_feat, has_bias)
        return dfeat, dw, (db if has_bias else None), None


def fused_head(feat, weight, bias, R):
    return _FusedHead.apply(feat, weight, bias, R)


class _FusedHeadCE(torch.autograd.Function):
    """The vision step's classifier tail, one launch each way
    (ops/csrc/head_ce.hip): avg-pool + per-client linear + masked CE with the
    device-side metrics forward; masked-CE backward + head backward.  Returns
    (losses (R,), scores (N, R, J)); only losses carries a gradient.  Outside
    the kernels' envelope (head_ce_route 'chain') the entries run
    head_fwd -> masked_ce_fwd and masked_ce_bwd -> head_bwd themselves."""

    @staticmethod
    def forward(ctx, feat, weight, bias, labels, mask, metrics, R):
        ext = require_native()
        feat = feat.contiguous()
        none = torch.Tensor()
        labels = labels.contiguous()
        losses, pooled, scores = ext.head_ce_fwd(
            feat, weight, bias if bias is not None else none, labels,
            mask if mask is not None else none,
            metrics if metrics is not None else none, R)
        ctx.save_for_backward(scores, labels,
                              mask if mask is not None else none, pooled,
                              weight)
        ctx.meta = (R, feat.size(2), feat.size(3),
                    feat.dtype == torch.bfloat16, bias is not None,
                    mask is not None)
        ctx.mark_non_differentiable(scores)
        return losses, scores

    @staticmethod
    def backward(ctx, up, _dscores):
        ext = require_native()
        scores, labels, mask, pooled, weight = ctx.saved_tensors
        R, H, W, bf16_feat, has_bias, has_mask = ctx.meta
        # up goes in as it comes: the kernel reads it through its stride
        dw, db, dfeat = ext.head_ce_bwd(
            up, scores, labels, mask if has_mask else torch.Tensor(), pooled,
            weight, R, H, W, bf16_feat, has_bias)
        return (dfeat, dw, (db if has_bias else None), None, None, None,
                None)


def fused_head_ce(feat, weight, bias, labels, mask, R, metrics=None):
    """feat (N, R*C, H, W) -> (losses (R,), scores (N, R, J)): pool, per-client
    linear and masked CE.  On the GPU the two-launch kernels; elsewhere today's
    functions composed (fused_head's torch twin and batched_masked_ce)."""
    if use_native(feat):
        return _FusedHeadCE.apply(feat, weight, bias, labels, mask, metrics,
                                  R)
    from ..fed.batched import batched_masked_ce
    pooled = F.adaptive_avg_pool2d(feat, 1).view(feat.size(0), R, -1)
    scores = torch.einsum('nri,roi->nro', pooled, weight)
    if bias is not None:
        scores = scores + bias
    losses = batched_masked_ce(scores.float(), labels, mask, metrics=metrics)
    return losses, scores


def head_ce_route(N, R, C, HW, J, elem_size, aligned=True):
    """Route head_ce_fwd / head_ce_bwd take: 'vec' (16-byte feat / dfeat
    accesses: HW * elem_size a multiple of 16, aligned bases), 'elem', or
    'chain' (the old four kernels: HETEROFL_STEP_FUSED=0, or an LDS stage
    over 64 KB: forward ((N + J) * (C + 1) + N * J) * 4 bytes, backward
    (N * J + 32 * J) * 4).  Launches nothing."""
    ext = require_native()
    return ext.head_ce_route(N, R, C, HW, J, elem_size, aligned)


def batch_gather(x_all, y_all, counter, B, ticket):
    """(x_all[c*B:(c+1)*B], y_all[c*B:(c+1)*B]) for c = counter[0], in one
    launch that also leaves counter at c + 1 (ops/csrc/batch_gather.hip).
    ticket: an int32 cell holding 0, back at 0 afterwards."""
    ext = require_native()
    xb, yb = ext.batch_gather(x_all, y_all, counter, ticket, B)
    return xb, yb


class GraphClipSGD:
    """hipGraph-capture variant of FusedClipSGD: the chunk LAYOUT is fixed by
    parameter shapes, so the device table is preallocated and the kernels are
    recorded against it; the grad POINTERS (graph-pool addresses captured by
    autograd.grad) are filled in afterwards with fill_chunk_table."""

    CHUNK = 65536
    CHUNK_BYTES = 40  # sizeof(Chunk): 4 pointers + 2 ints

    def __init__(self, params, bufs, R, device, shadows=None):
        require_native()
        self.params = list(params)
        self.bufs = list(bufs)
        self.shadows = [s if s is not None else torch.Tensor()
                        for s in (shadows or [])]
        self.R = R
        clients = []
        for p in self.params:
            per = p.numel() // R
            nch = (per + self.CHUNK - 1) // self.CHUNK
            for r in range(R):
                clients.extend([r] * nch)
        self.n_chunks = len(clients)
        self.table = torch.zeros(self.n_chunks * self.CHUNK_BYTES,
                                 dtype=torch.uint8, device=device)
        self.chunk_client = torch.tensor(clients, dtype=torch.int32).to(device)
        self.partials = torch.zeros(self.n_chunks, dtype=torch.float32,
                                    device=device)
        self.normsq = torch.zeros(R, dtype=torch.float32, device=device)

    def bind(self, grads):
        """Write (grad, param, buf, shadow) pointers into the device table."""
        ext = require_native()
        ext.fill_chunk_table(self.table, list(grads), self.params, self.bufs,
                             self.R, self.CHUNK, self.shadows)

    def launch(self, max_norm, lr, momentum, weight_decay):
        ext = require_native()
        ext.clip_sgd_step(self.table, self.n_chunks, self.chunk_client,
                          self.partials, self.normsq, max_norm, lr, momentum,
                          weight_decay)


class _FusedAttention(torch.autograd.Function):
    """Fused attention (ops/csrc/attention.hip), head_dim<=32.  S<=64 runs
    the whole-(batch*head) single-kernel path saving the bf16 softmax
    matrix; larger S runs the blockwise (flash-style) path — 64-row KV
    tiles with an online softmax, per-row LSE saved, and a deterministic
    two-pass backward that recomputes P (SURVEY §5 long-context
    readiness)."""

    @staticmethod
    def forward(ctx, q, k, v, temperature):
        ext = require_native()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if q.size(1) <= 64:
            out, p = ext.attn_fwd(q, k, v, temperature)
            ctx.save_for_backward(q, k, v, p)
            ctx.blockwise = False
        else:
            out, lse = ext.attn_fwd_block(q, k, v, temperature)
            ctx.save_for_backward(q, k, v, out, lse)
            ctx.blockwise = True
        ctx.temperature = temperature
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = require_native()
        if ctx.blockwise:
            q, k, v, out, lse = ctx.saved_tensors
            dq, dk, dv = ext.attn_bwd_block(dout, q, k, v, out, lse,
                                            ctx.temperature)
        else:
            q, k, v, p = ctx.saved_tensors
            dq, dk, dv = ext.attn_bwd(dout, q, k, v, p, ctx.temperature)
        return dq, dk, dv, None


def fused_attention(q, k, v, temperature):
    return _FusedAttention.apply(q, k, v, temperature)


class _FusedLayerNorm(torch.autograd.Function):
    """Per-client LayerNorm over the last dim (ops/csrc/layernorm.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, R, eps):
        ext = require_native()
        x = x.contiguous()
        y, mean, invstd = ext.ln_fwd(x, weight, bias, R, eps)
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.R = R
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        x, weight, mean, invstd = ctx.saved_tensors
        dx, dgamma, dbeta = ext.ln_bwd(dy, x, weight, mean, invstd, ctx.R)
        return dx, dgamma, dbeta, None, None


def fused_layernorm(x, weight, bias, R, eps=1e-5):
    return _FusedLayerNorm.apply(x, weight, bias, R, eps)


class _FusedLMCE(torch.autograd.Function):
    """Vocab-masked LM cross-entropy over (R, B, S, V) bf16/fp32 logits;
    per-client mean NLL over every position (ops/csrc/lm_ce.hip)."""

    @staticmethod
    def forward(ctx, logits, tokens, mask, R):
        ext = require_native()
        logits = logits.contiguous()
        labels = tokens.reshape(-1)
        losses, _, row_max, row_logsum = ext.lm_ce_fwd(
            logits, labels, mask if mask is not None else torch.Tensor(), R)
        ctx.save_for_backward(logits, labels, row_max, row_logsum,
                              mask if mask is not None else torch.Tensor())
        ctx.R = R
        ctx.has_mask = mask is not None
        return losses

    @staticmethod
    def backward(ctx, up):
        ext = require_native()
        logits, labels, row_max, row_logsum, mask = ctx.saved_tensors
        d = ext.lm_ce_bwd(logits, labels,
                          mask if ctx.has_mask else torch.Tensor(), row_max,
                          row_logsum, up, ctx.R)
        return d, None, None, None


def fused_lm_ce(logits, tokens, mask, R):
    return _FusedLMCE.apply(logits, tokens, mask, R)


# ------------------------------------------------------- LM glue fusions
_rng_cells = {}
_rng_salt = [0]


def _next_salt():
    """Per-call-site salt: decorrelates the many dropout sites inside one
    step without a bump launch per call.  In eager mode the counter also
    advances across steps; in a captured graph the salts freeze at capture
    and the per-step rng_bump (launched by the step driver) moves the seed
    cell instead."""
    _rng_salt[0] = (_rng_salt[0] + 1) & 0x7FFFFFFF
    return _rng_salt[0]


def bump_rng(device):
    """Advance the device RNG seed cell (once per training step)."""
    ext = require_native()
    ext.rng_bump(_rng_cell(device))


def _rng_cell(device):
    """Per-device u64 seed cell read by the fused dropout kernels and bumped
    device-side after each draw — a stable pointer, so hipGraph replays draw
    fresh masks (torch's philox handles its own ops; these are ours)."""
    key = str(device)
    if key not in _rng_cells:
        _rng_cells[key] = torch.tensor(
            [torch.initial_seed() & 0x7FFFFFFFFFFFFFFF],
            dtype=torch.int64, device=device)
    return _rng_cells[key]


class _FusedGeluDropout(torch.autograd.Function):
    """dropout(gelu(x / rate), p) in one kernel each way, mask saved
    (reference chain: src/models/transformer.py:116 —
    dropout1(GELU(scaler(linear1(src)))))."""

    @staticmethod
    def forward(ctx, x, rate, p):
        ext = require_native()
        x = x.contiguous()
        y, mask = ext.gelu_drop_fwd(x, _rng_cell(x.device), _next_salt(),
                                    rate, p)
        ctx.save_for_backward(x, mask)
        ctx.meta = (rate, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        x, mask = ctx.saved_tensors
        rate, p = ctx.meta
        return ext.gelu_drop_bwd(dy, x, mask, rate, p), None, None


def fused_gelu_dropout(x, rate, p):
    return _FusedGeluDropout.apply(x, rate, p)


class _FusedResDropout(torch.autograd.Function):
    """src + dropout(h / rate, p) in one kernel; backward is dt for src and
    one mask-scale kernel for h (the LN that follows is already fused)."""

    @staticmethod
    def forward(ctx, src, h, rate, p):
        ext = require_native()
        t, mask = ext.res_drop_fwd(src.contiguous(), h.contiguous(),
                                   _rng_cell(src.device), _next_salt(),
                                   rate, p)
        ctx.save_for_backward(mask)
        ctx.meta = (rate, p)
        return t

    @staticmethod
    def backward(ctx, dt):
        ext = require_native()
        (mask,) = ctx.saved_tensors
        rate, p = ctx.meta
        dh = ext.drop_scale_bwd(dt, mask, rate, p)
        return dt, dh, None, None


def fused_res_dropout(src, h, rate, p):
    return _FusedResDropout.apply(src, h, rate, p)


class _FusedScaler(torch.autograd.Function):
    """Standalone Scaler kernel (K5 of SURVEY §2b; reference
    src/modules/modules.py:9-11): y = x / rate in training.  Runs the
    drop_scale kernel with p=0 (pure 1/rate scale) both directions — used
    by the norm='none' ablation, where the Scaler cannot cancel into a
    following train-mode norm."""

    @staticmethod
    def forward(ctx, x, rate):
        ext = require_native()
        ctx.rate = rate
        return ext.drop_scale_bwd(x.contiguous(), torch.Tensor(), rate, 0.0)

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        return ext.drop_scale_bwd(dy.contiguous(), torch.Tensor(),
                                  ctx.rate, 0.0), None


def fused_scaler(x, rate):
    return _FusedScaler.apply(x, rate)


def fused_token_mask(tokens, rate, mask_id):
    """Bernoulli(rate) token masking in one kernel (K11; reference:
    src/models/transformer.py:149-151) — (seed, salt, index)-keyed RNG,
    graph-replay safe."""
    ext = require_native()
    return ext.token_mask(tokens.contiguous(), _rng_cell(tokens.device),
                          _next_salt(), rate, mask_id)


class _FusedMaxPool2(torch.autograd.Function):
    """2x2/stride-2 MaxPool (K6; reference src/models/conv.py:33): forward
    saves the winning-corner index, backward scatters to it."""

    @staticmethod
    def forward(ctx, x):
        ext = require_native()
        y, arg = ext.maxpool2_fwd(x.contiguous())
        ctx.save_for_backward(arg)
        ctx.hw = (x.size(2), x.size(3))
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        (arg,) = ctx.saved_tensors
        return ext.maxpool2_bwd(dy, arg, *ctx.hw)


def fused_maxpool2(x):
    return _FusedMaxPool2.apply(x)


class _FusedEmbedPos(torch.autograd.Function):
    """Fused token-embedding + positional-embedding gather with the Scaler
    folded in (K9; reference: src/models/transformer.py:29-37).  Reads the
    bf16 shadow tables when present; the deterministic backward writes fp32
    grads straight for the fp32 masters (no shadow-upcast kernels, no
    atomics — bit-stable under graph replay)."""

    @staticmethod
    def forward(ctx, ids, table, pos, t16, p16, rate):
        ext = require_native()
        use16 = t16 is not None and p16 is not None
        t = t16 if use16 else table
        p = p16 if use16 else pos
        out = ext.embed_pos_fwd(ids.contiguous(), t.contiguous(),
                                p.contiguous(), rate)
        ctx.save_for_backward(ids)
        ctx.meta = (table.size(1), pos.size(1), rate)
        return out

    @staticmethod
    def backward(ctx, dy):
        ext = require_native()
        (ids,) = ctx.saved_tensors
        V, P, rate = ctx.meta
        dtable, dpos = ext.embed_pos_bwd(dy, ids, V, P, rate)
        return None, dtable, dpos, None, None, None


def fused_embed_pos(ids, table, pos, t16, p16, rate):
    return _FusedEmbedPos.apply(ids, table, pos, t16, p16, rate)


# ------------------------------------------------- combine accumulate (K14)
COMBINE_PER_BLOCK = 1024   # elements per block (combine.hip)
_COMBINE_BLOCKS = {}       # (device, shapes) -> (n_blocks, 2) int32 table


def _check_window(win, size, what):
    period, shift, take = win
    if not (period >= 1 and size % period == 0 and 0 <= shift < period
            and 1 <= take <= period):
        raise ValueError('combine_accumulate: bad {} window {} over an axis '
                         'of {}'.format(what, win, size))
    return (size // period) * take


def combine_accumulate(shapes, clients, device):
    """The accumulator and count of Federation.accumulate for a set of
    global tensors from ONE kernel launch (ops/csrc/combine.hip).

    shapes[i] is the global tensor's shape; its dim 0 is the out axis, dim 1
    (if any) the in axis and the rest `inner`.  clients[i] lists the
    reporting clients of tensor i in ascending slot order, each
    (val, out_window, in_window, row_mask): val the client's fp32 slice on
    `device`, a window (period, shift, take) mapping local index j to global
    (j // take) * period + (shift + j % take) % period (in_window None for
    1-D tensors), row_mask None or a uint8 array over the local out rows
    (the label-split filter of output layers; 0 drops the row).

    Returns ([tmp_i], [cnt_i]), global-shaped fp32, every element written
    (zeros where nobody contributes).  Clients are added one at a time in
    list order, so the sums are bit-identical to the torch loop's."""
    import numpy as np
    ext = require_native()
    if ext is None:
        raise RuntimeError('combine_accumulate is the native route; use '
                           'Federation.accumulate under HETEROFL_FORCE_EAGER')
    device = torch.device(device)
    t_dt = np.dtype([('tmp', 'u8'), ('cnt', 'u8'), ('O', 'i4'), ('I', 'i4'),
                     ('inner', 'i4'), ('ent_start', 'i4'),
                     ('ent_count', 'i4'), ('pad', 'i4')])
    e_dt = np.dtype([('val', 'u8'), ('mask', 'u8'), ('out', 'i4', 3),
                     ('inp', 'i4', 3), ('n_in', 'i4'), ('pad', 'i4')])
    assert t_dt.itemsize == 40 and e_dt.itemsize == 48
    dims, numels = [], []
    for shape in shapes:
        shape = tuple(int(s) for s in shape)
        if len(shape) == 0:
            shape = (1,)
        O = shape[0]
        I = shape[1] if len(shape) > 1 else 1
        inner = 1
        for s in shape[2:]:
            inner *= s
        if O * I * inner >= 2 ** 31:
            raise ValueError('combine_accumulate: tensor too large')
        dims.append((O, I, inner))
        numels.append(O * I * inner)
    total = sum(numels)
    flat_tmp = torch.empty(total, dtype=torch.float32, device=device)
    flat_cnt = torch.empty(total, dtype=torch.float32, device=device)
    tensors = np.zeros(len(dims), dtype=t_dt)
    n_entries = sum(len(c) for c in clients)
    entries = np.zeros(n_entries, dtype=e_dt)
    masks, mask_off, keep = [], 0, []
    mask_rel = np.full(n_entries, -1, dtype=np.int64)
    e = off = 0
    tmp_out, cnt_out = [], []
    for i, ((O, I, inner), shape) in enumerate(zip(dims, shapes)):
        tmp = flat_tmp[off:off + numels[i]].view(tuple(shape))
        cnt = flat_cnt[off:off + numels[i]].view(tuple(shape))
        tmp_out.append(tmp)
        cnt_out.append(cnt)
        tensors[i] = (tmp.data_ptr(), cnt.data_ptr(), O, I, inner, e,
                      len(clients[i]), 0)
        off += numels[i]
        for val, ow, iw, mask in clients[i]:
            if iw is None:
                iw = (I, 0, I)
            n_out = _check_window(ow, O, 'out')
            n_in = _check_window(iw, I, 'in')
            if not (val.dtype == torch.float32 and val.device == device):
                raise ValueError('combine_accumulate: client values must be '
                                 'fp32 on {}'.format(device))
            if val.numel() != n_out * n_in * inner:
                raise ValueError(
                    'combine_accumulate: client slice of {} elements does '
                    'not match its windows ({} x {} x {})'.format(
                        val.numel(), n_out, n_in, inner))
            val = val.contiguous()
            keep.append(val)
            if mask is not None:
                mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
                if mask.size != n_out:
                    raise ValueError('combine_accumulate: row mask of {} '
                                     'for {} rows'.format(mask.size, n_out))
                mask_rel[e] = mask_off
                masks.append(mask)
                mask_off += mask.size
            entries[e] = (val.data_ptr(), 0, tuple(ow), tuple(iw), n_in, 0)
            e += 1
    bkey = (str(device), tuple(dims))
    blocks = _COMBINE_BLOCKS.get(bkey)
    if blocks is None:
        rows = [np.stack([np.full((n + COMBINE_PER_BLOCK - 1)
                                  // COMBINE_PER_BLOCK, i, dtype=np.int32),
                          np.arange(0, n, COMBINE_PER_BLOCK,
                                    dtype=np.int32)], 1)
                for i, n in enumerate(numels) if n]
        tab = np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)
        if len(_COMBINE_BLOCKS) >= 16:
            _COMBINE_BLOCKS.clear()
        blocks = _COMBINE_BLOCKS[bkey] = \
            torch.from_numpy(np.ascontiguousarray(tab)).to(device)
    # one upload: [tensor table | entry table | row masks]
    mask_base = tensors.nbytes + entries.nbytes
    table = torch.empty(mask_base + mask_off, dtype=torch.uint8,
                        device=device)
    has = mask_rel >= 0
    entries['mask'][has] = (table.data_ptr() + mask_base
                            + mask_rel[has]).astype(np.uint64)
    host = np.concatenate([tensors.view(np.uint8), entries.view(np.uint8)]
                          + masks)
    table.copy_(torch.from_numpy(host))
    ext.combine_accumulate(table, len(dims), n_entries, blocks)
    del keep
    return tmp_out, cnt_out
