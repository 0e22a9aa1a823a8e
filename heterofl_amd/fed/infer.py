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

The engine snapshots the model's weights when it is built; rebuild it after
the model changes.
"""
import torch
import torch.nn as nn

from .. import ops as native_ops
from ..models.conv import Conv
from ..models.resnet import ResNet, Block, Bottleneck


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
