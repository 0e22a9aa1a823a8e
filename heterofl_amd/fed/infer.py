"""Native inference engine for the vision models (conv, resnet*).

NativeInference walks an eager *tracked* model (the one runner.stats()
returns: BatchNorm with running statistics, or gn/in/ln/none) once, packs the
conv weights for the large-batch forward kernel and folds every BatchNorm's
running statistics into a per-channel scale/shift, then evaluates batches
with the hand-written kernels only:

    conv          conv_fwd_large (ops/csrc/conv_infer.hip) where the router
                  admits the shape, the training-family conv_fwd otherwise
    bn            bn_relu_infer (folded running statistics)
    gn / in / ln  gn_relu_fwd (no running statistics exist)
    none          bn_relu_infer with scale 1, shift 0 (ReLU only)
    conv pools    maxpool2_fwd
    head          head_fwd (avgpool + linear)

The Scaler is the identity at inference (models/modules.py).  On CPU, or
under HETEROFL_FORCE_EAGER=1, the module itself is called: the CPU path is
the numerics oracle, as everywhere in this project.

NativeLMInference does the same for the masked-LM transformer: per-token NLL
of pre-masked windows with

    embedding     embed_pos_fwd (token + positional gather)
    LayerNorm     ln_fwd (R = 1)
    attention     attn_fwd (S <= 64) / attn_fwd_block (longer windows)
    residual add  res_drop_fwd (p = 0)
    GELU          gelu_drop_fwd (p = 0, rate 1)
    linears       bf16 F.linear on the encoder and decoder.linear1 (the
                  library-GEMM decision of VERDICT.md K7); linear_q/k/v are
                  concatenated into one E -> 3E projection
    head          lm_head_ce (ops/csrc/lm_head.hip): vocabulary projection
                  fused with the cross-entropy, no (M, V) logits; or the
                  two-step bf16 F.linear + lm_ce_fwd where the router
                  (ops.fused.lm_head_route) measured that faster
    fill-mask     lm_head_topk (the same kernel with per-lane candidate
                  lists): window_topk and fill_mask take every position's
                  k <= 8 most likely tokens,
                  their log-probabilities and the label's NLL from one
                  vocabulary pass, again without (M, V) logits; it is the
                  only route (no two-step top-k measured faster, see
                  profiles/NOTES.md)

Both engines snapshot the model's weights when they are built; rebuild them
after the model changes.
"""
import torch
import torch.nn as nn

from .. import ops as native_ops
from ..models.conv import Conv
from ..models.resnet import ResNet, Block, Bottleneck
from ..models.transformer import Transformer


class NativeInference:
    """`large`: True follows ops.fused.large_conv_route, 'all' sends every
    supported conv shape to conv_fwd_large, False keeps every conv on
    conv_fwd.  `dtype`: activation dtype on the GPU (bf16 default; fp32 runs
    the exact-f32 MFMA path of conv_fwd and never the large kernel)."""

    def __init__(self, test_model, dtype=torch.bfloat16, large=True):
        if not isinstance(test_model, (ResNet, Conv)):
            raise TypeError('NativeInference supports the conv and resnet '
                            'models only')
        self.model = test_model
        p = next(test_model.parameters())
        self.device = p.device
        self.native = native_ops.use_native(p)
        self.dtype = dtype
        self.large = large if dtype == torch.bfloat16 else False
        if self.native:
            self.ext = native_ops.require_native()
            with torch.no_grad():
                if isinstance(test_model, ResNet):
                    self._build_resnet(test_model)
                else:
                    self._build_conv(test_model)

    # ------------------------------------------------------------- building
    def _conv_site(self, m):
        from ..ops.fused import conv_pack_weight, large_conv_supported
        if m.groups != 1 or m.kernel_size[0] != m.kernel_size[1] \
                or m.stride[0] != m.stride[1] \
                or m.padding[0] != m.padding[1] or m.dilation != (1, 1):
            raise ValueError('unsupported conv geometry: {}'.format(m))
        k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
        w = m.weight.detach().float().contiguous()
        site = {'w': w, 'k': k, 's': s, 'p': p,
                'cin': w.size(1), 'cout': w.size(0),
                'bias': None if m.bias is None
                else m.bias.detach().float().contiguous(),
                'packed': None}
        if self.large and large_conv_supported(k, s, p):
            site['packed'] = conv_pack_weight(w)
        return site

    def _norm_site(self, m, channels):
        from ..ops.fused import fold_bn
        if isinstance(m, nn.BatchNorm2d):
            if m.running_mean is None:
                raise ValueError(
                    'NativeInference needs a tracked model (BatchNorm '
                    'running statistics); pass the model runner.stats() '
                    'returns')
            scale, shift = fold_bn(m.weight.detach(), m.bias.detach(),
                                   m.running_mean, m.running_var, m.eps)
            return ('bn', scale.contiguous(), shift.contiguous())
        if isinstance(m, nn.GroupNorm):
            return ('gn', m.weight.detach().float().contiguous(),
                    m.bias.detach().float().contiguous(), m.num_groups, m.eps)
        if isinstance(m, nn.Identity):
            return ('bn', torch.ones(channels, device=self.device),
                    torch.zeros(channels, device=self.device))
        raise ValueError('unsupported norm: {}'.format(m))

    def _build_resnet(self, model):
        self.stem = self._conv_site(model.conv1)
        self.blocks = []
        for layer in (model.layer1, model.layer2, model.layer3, model.layer4):
            for blk in layer:
                if not isinstance(blk, (Block, Bottleneck)):
                    raise TypeError('unknown block {}'.format(type(blk)))
                b = {'n1': self._norm_site(blk.n1, blk.conv1.in_channels),
                     'conv1': self._conv_site(blk.conv1),
                     'n2': self._norm_site(blk.n2, blk.conv2.in_channels),
                     'conv2': self._conv_site(blk.conv2),
                     'shortcut': self._conv_site(blk.shortcut)
                     if hasattr(blk, 'shortcut') else None}
                if isinstance(blk, Bottleneck):
                    b['n3'] = self._norm_site(blk.n3, blk.conv3.in_channels)
                    b['conv3'] = self._conv_site(blk.conv3)
                self.blocks.append(b)
        self.final_norm = self._norm_site(model.n4, model.linear.in_features)
        self._head(model.linear)

    def _build_conv(self, model):
        self.steps = []
        norm, channels = None, None
        for m in model.blocks:
            if isinstance(m, nn.Conv2d):
                self.steps.append(('conv', self._conv_site(m)))
                channels, norm = m.out_channels, None
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                norm = m
            elif isinstance(m, nn.ReLU):
                self.steps.append(('norm', self._norm_site(
                    norm if norm is not None else nn.Identity(), channels)))
                norm = None
            elif isinstance(m, nn.MaxPool2d):
                self.steps.append(('pool', None))
            elif isinstance(m, nn.Linear):
                self._head(m)
            # Scaler / Identity / AdaptiveAvgPool2d / Flatten: the Scaler is
            # the identity at inference, pool+flatten live in the fused head
        self.blocks = None

    def _head(self, linear):
        self.head_w = linear.weight.detach().float().unsqueeze(0).contiguous()
        self.head_b = None if linear.bias is None else \
            linear.bias.detach().float().unsqueeze(0).contiguous()

    # -------------------------------------------------------------- running
    def _conv(self, site, x, residual=None):
        from ..ops.fused import conv_fwd_large, large_conv_route
        if site['packed'] is not None and (
                self.large == 'all' or large_conv_route(
                    x.size(0), site['cin'], x.size(2), x.size(3),
                    site['cout'], site['k'], site['s'], site['p'])):
            return conv_fwd_large(x, site['packed'], site['bias'], residual,
                                  site['s'], site['p'], site['cin'],
                                  site['cout'], site['k'])
        none = torch.Tensor()
        return self.ext.conv_fwd(
            x, site['w'], site['bias'] if site['bias'] is not None else none,
            residual if residual is not None else none, 1, site['s'],
            site['p'], 0)

    def _norm(self, site, x):
        if site[0] == 'bn':
            return self.ext.bn_relu_infer(x, site[1], site[2])
        return self.ext.gn_relu_fwd(x, site[1], site[2], site[3], site[4])[0]

    def __call__(self, x):
        """x: (N, C, H, W) normalized float images -> fp32 logits (N, J)."""
        with torch.no_grad():
            if not self.native:
                self.model.train(False)
                label = torch.zeros(x.size(0), dtype=torch.long,
                                    device=x.device)
                return self.model({'img': x, 'label': label})['score'].float()
            out = x.to(self.device, self.dtype).contiguous()
            if self.blocks is not None:
                out = self._conv(self.stem, out)
                for b in self.blocks:
                    o = self._norm(b['n1'], out)
                    sc = self._conv(b['shortcut'], o) \
                        if b['shortcut'] is not None else out
                    o = self._conv(b['conv1'], o)
                    if 'conv3' in b:
                        o = self._conv(b['conv2'], self._norm(b['n2'], o))
                        out = self._conv(b['conv3'], self._norm(b['n3'], o),
                                         residual=sc)
                    else:
                        out = self._conv(b['conv2'], self._norm(b['n2'], o),
                                         residual=sc)
                out = self._norm(self.final_norm, out)
            else:
                for kind, site in self.steps:
                    if kind == 'conv':
                        out = self._conv(site, out)
                    elif kind == 'norm':
                        out = self._norm(site, out)
                    else:
                        out = self.ext.maxpool2_fwd(out)[0]
            scores = self.ext.head_fwd(
                out, self.head_w,
                self.head_b if self.head_b is not None else torch.Tensor(),
                1)[0]
            return scores.squeeze(1)


class NativeLMInference:
    """Per-token NLL (window_nll) and top-k predictions (window_topk,
    fill_mask) of an eager models.transformer.Transformer at inference
    (Scaler and dropout are the identity).  `head` (window_nll only): 'fused' runs lm_head_ce,
    'gemm' the two-step bf16 F.linear + lm_ce_fwd, 'auto' follows
    ops.fused.lm_head_route.  `chunk`: sequences per forward; the default
    keeps attn_fwd's saved (N*H, S, S) bf16 buffer under ~256 MB."""

    ATTN_BYTES = 256 << 20
    LOGIT_BYTES = 256 << 20   # logits of one step where they are written

    def __init__(self, model, head='auto', chunk=None):
        from ..ops.fused import lm_head_pack
        if not isinstance(model, Transformer):
            raise TypeError('NativeLMInference supports the transformer only')
        if head not in ('fused', 'gemm', 'auto'):
            raise ValueError("head must be 'fused', 'gemm' or 'auto'")
        self.model = model
        self.head = head
        self.chunk = chunk
        p = next(model.parameters())
        self.device = p.device
        self.native = native_ops.use_native(p)
        emb = model.transformer_embedding
        self.V = model.num_tokens
        self.E = emb.embedding.weight.size(1)
        self.layers = model.transformer_encoder['layers']
        self.H = self.layers[0].mha.num_heads
        with torch.no_grad():
            lin2 = model.decoder.linear2
            self.packed = lm_head_pack(lin2.weight, lin2.bias)
            self.head_b = lin2.bias.detach().float().contiguous()
            if self.native:
                self.ext = native_ops.require_native()
                self._snapshot(model)

    # ------------------------------------------------------------- building
    def _snapshot(self, model):
        def w16(t):
            return t.detach().to(torch.bfloat16).contiguous()

        def norm(m):
            return (m.weight.detach().float().view(1, -1).contiguous(),
                    m.bias.detach().float().view(1, -1).contiguous(), m.eps)

        def lin(m):
            return (w16(m.weight), w16(m.bias))

        emb = model.transformer_embedding
        self.table = w16(emb.embedding.weight).unsqueeze(0)
        self.pos = w16(emb.positional_embedding.positional_embedding
                       .weight).unsqueeze(0)
        self.emb_norm = norm(emb.norm)
        self.sites = []
        for layer in self.layers:
            mha = layer.mha
            qkv = (mha.linear_q, mha.linear_k, mha.linear_v)
            self.sites.append({
                'qkv': (w16(torch.cat([m.weight for m in qkv])),
                        w16(torch.cat([m.bias for m in qkv]))),
                'o': lin(mha.linear_o), 'temperature': mha.attention.temperature,
                'n1': norm(layer.norm1), 'l1': lin(layer.linear1),
                'l2': lin(layer.linear2), 'n2': norm(layer.norm2)})
        dec = model.decoder
        self.dec_l1 = lin(dec.linear1)
        self.dec_norm = norm(dec.norm1)
        self.head_w16 = lin(dec.linear2)   # the 'gemm' head

    # -------------------------------------------------------------- running
    def _chunk(self, S):
        if self.chunk is not None:
            return max(int(self.chunk), 1)
        if not self.native:   # the eager path materialises fp32 logits
            return max(self.LOGIT_BYTES // (4 * S * self.V), 1)
        return max(self.ATTN_BYTES // (2 * self.H * S * S), 1)

    def _ln(self, x, site):
        return self.ext.ln_fwd(x, site[0], site[1], 1, site[2])[0]

    def _hidden(self, src):
        """(n, S) pre-masked ids -> (n*S, E) bf16 input of the vocabulary
        head."""
        import torch.nn.functional as F
        from ..ops.fused import _rng_cell
        ext = self.ext
        n, S = src.shape
        E, H = self.E, self.H
        d = E // H
        seed = _rng_cell(self.device)   # read by the p = 0 kernels, not used
        x = ext.embed_pos_fwd(src.view(1, n, S).contiguous(), self.table,
                              self.pos, 1.0)
        x = self._ln(x.view(n * S, E), self.emb_norm)
        for st in self.sites:
            qkv = F.linear(x, *st['qkv']).view(n, S, 3, H, d)
            qkv = qkv.permute(2, 0, 3, 1, 4).reshape(3, n * H, S, d)
            attn = ext.attn_fwd if S <= 64 else ext.attn_fwd_block
            o = attn(qkv[0], qkv[1], qkv[2], st['temperature'])[0]
            o = o.view(n, H, S, d).permute(0, 2, 1, 3).reshape(n * S, E)
            o = F.linear(o, *st['o'])
            x = self._ln(ext.res_drop_fwd(x, o, seed, 0, 1.0, 0.0)[0],
                         st['n1'])
            h = ext.gelu_drop_fwd(F.linear(x, *st['l1']), seed, 0, 1.0,
                                  0.0)[0]
            h = F.linear(h, *st['l2'])
            x = self._ln(ext.res_drop_fwd(x, h, seed, 0, 1.0, 0.0)[0],
                         st['n2'])
        h = ext.gelu_drop_fwd(F.linear(x, *self.dec_l1), seed, 0, 1.0, 0.0)[0]
        return self._ln(h, self.dec_norm)

    def _head_nll(self, h, label, vocab_mask):
        import torch.nn.functional as F
        from ..ops.fused import lm_head_ce, lm_head_route
        fused = self.head == 'fused' or (
            self.head == 'auto' and lm_head_route(h.size(0), self.E, self.V))
        if fused:
            return lm_head_ce(h, self.packed, self.head_b, label, vocab_mask,
                              self.V, self.E)[0]
        out = []
        step = max(self.LOGIT_BYTES // (2 * self.V), 1)
        for r0 in range(0, h.size(0), step):
            y = label[r0:r0 + step]
            logits = F.linear(h[r0:r0 + step], *self.head_w16)
            lse = self.ext.lm_ce_fwd(
                logits, y, vocab_mask if vocab_mask is not None
                else torch.Tensor(), 1)[1]
            picked = logits.gather(1, y.view(-1, 1)).squeeze(1).float()
            if vocab_mask is not None:
                picked = picked * (vocab_mask[y] != 0)
            out.append(lse - picked)
        return torch.cat(out)

    def _eager_hidden(self, src):
        m = self.model
        x = m.transformer_embedding(src)
        for layer in self.layers:
            x = layer(x)
        dec = m.decoder
        x = dec.norm1(dec.activation(dec.scaler(dec.linear1(x))))
        return x.reshape(-1, x.size(-1))

    def window_nll(self, src, label, vocab_mask=None):
        """src (N, S) int64 ids with the <mask> id already filled in, label
        (N, S) int64 -> (N, S) fp32 per-token NLL.  vocab_mask (V,) in
        {0, 1}: masked logits are 0 and stay in the softmax."""
        from ..ops.fused import lm_head_ce
        with torch.no_grad():
            N, S = src.shape
            src = src.to(self.device)
            label = label.to(self.device)
            if vocab_mask is not None:
                vocab_mask = vocab_mask.to(self.device).float()
            out = []
            step = self._chunk(S)
            for n0 in range(0, N, step):
                s = src[n0:n0 + step]
                y = label[n0:n0 + step].reshape(-1).contiguous()
                if self.native:
                    nll = self._head_nll(self._hidden(s), y, vocab_mask)
                else:
                    self.model.train(False)
                    nll = lm_head_ce(self._eager_hidden(s), self.packed,
                                     self.head_b, y, vocab_mask, self.V,
                                     self.E)[0]
                out.append(nll.view(-1, S))
            return torch.cat(out)

    def window_topk(self, src, k=5, label=None, vocab_mask=None,
                    only_masked=False):
        """src (N, S) int64 ids with the <mask> id already filled in ->
        (ids (N, S, k) int64, logp (N, S, k) fp32, nll (N, S) fp32 or None
        without `label`): every position's k most likely tokens in
        descending order (equal logits: the lower id first), their
        log-probabilities logit - lse, and the label's NLL from the same
        vocabulary pass (lm_head_topk).  only_masked: the head runs on the
        positions where src is the <mask> id only; every other position
        reads ids -1, logp -inf, nll 0."""
        from ..ops.fused import lm_head_topk
        with torch.no_grad():
            N, S = src.shape
            src = src.to(self.device)
            if label is not None:
                label = label.to(self.device)
            if vocab_mask is not None:
                vocab_mask = vocab_mask.to(self.device).float()
            ids, logp, nll = [], [], []
            step = self._chunk(S)
            for n0 in range(0, N, step):
                s = src[n0:n0 + step]
                rows = s.numel()
                if self.native:
                    h = self._hidden(s)
                else:
                    self.model.train(False)
                    h = self._eager_hidden(s)
                y = None if label is None else \
                    label[n0:n0 + step].reshape(-1).contiguous()
                # the split count of the chunk's full row count, also where
                # only the masked rows run: the two modes then agree bit
                # for bit on those rows
                splits = self.ext.lm_head_topk_splits(rows, self.V) \
                    if self.native else 0
                if only_masked:
                    at = (s.reshape(-1) == self.V).nonzero().squeeze(1)
                    h = h[at].contiguous()
                    y = None if y is None else y[at].contiguous()
                i_c = torch.full((rows, k), -1, dtype=torch.long,
                                 device=self.device)
                p_c = torch.full((rows, k), float('-inf'),
                                 dtype=torch.float32, device=self.device)
                n_c = torch.zeros(rows, dtype=torch.float32,
                                  device=self.device)
                if h.size(0):
                    val, idx, lse, nl = lm_head_topk(
                        h, self.packed, self.head_b, y, vocab_mask, self.V,
                        self.E, k, splits)
                    lp = val - lse.view(-1, 1)
                    if only_masked:
                        i_c[at], p_c[at] = idx, lp
                        if y is not None:
                            n_c[at] = nl
                    else:
                        i_c, p_c = idx, lp
                        n_c = nl if y is not None else n_c
                ids.append(i_c.view(-1, S, k))
                logp.append(p_c.view(-1, S, k))
                nll.append(n_c.view(-1, S))
            return (torch.cat(ids), torch.cat(logp),
                    None if label is None else torch.cat(nll))

    def fill_mask(self, src, k=5, vocab_mask=None):
        """Predictions for the <mask> positions of src (N, S): (positions
        (P, 2) int64 [sequence, offset] in row-major order, ids (P, k)
        int64, probs (P, k) fp32 = exp(logp))."""
        ids, logp, _ = self.window_topk(src, k=k, vocab_mask=vocab_mask,
                                        only_masked=True)
        pos = (src.to(self.device) == self.V).nonzero()
        return (pos, ids[pos[:, 0], pos[:, 1]],
                logp[pos[:, 0], pos[:, 1]].exp())


# ------------------------------------------------------ evaluation helpers
def user_csr(data_split, label_split, num_users, classes_size, mask, device):
    """CSR form of the users' test shards plus their (U, C) label masks, as
    eval_metrics takes them.  With mask off every class stays live."""
    ptr = [0]
    samples = []
    label_mask = torch.zeros(num_users, classes_size)
    for m in range(num_users):
        idx = list(data_split[m])
        samples.extend(idx)
        ptr.append(len(samples))
        if mask:
            label_mask[m, torch.as_tensor(label_split[m], dtype=torch.long)] = 1
        else:
            label_mask[m] = 1
    return (torch.tensor(ptr, dtype=torch.long, device=device),
            torch.tensor(samples, dtype=torch.long, device=device),
            label_mask.to(device))


def batched_logits(infer, img_u8, augment, batch=2048):
    """Logits of a staged uint8 image set, `batch` samples per forward."""
    scores = [infer(augment(img_u8[b0:b0 + batch], train=False))
              for b0 in range(0, img_u8.size(0), batch)]
    return torch.cat(scores) if scores else torch.zeros(0, 0)
