"""Federation core: width-sliced subnetwork distribute / combine.

Re-implements the semantics of the reference Federation (reference:
src/fed.py:8-298) with a typed index-map representation instead of
per-parameter torch.meshgrid gathers:

- every slice the HeteroFL rules produce is either FULL (whole axis),
  PREFIX(n) (the first n indices — conv/resnet channel slicing and
  transformer non-qkv slicing), or GATHER(tensor) (transformer per-head
  slicing and label-split-filtered output rows).
- distribute() turns PREFIX maps into contiguous narrow+clone (no gather);
- combine() accumulates into an fp32 accumulator + count per parameter and
  writes the masked average in place into the global tensors, exactly like
  reference src/fed.py:180-298 (including label_split filtering of the
  output layers).

The slicing rule sets per architecture mirror reference src/fed.py:26-159,
including the transformer quirks: per-head q/k/v slicing (fed.py:124-131)
and the idx_i reset after linear_q/linear_k biases (fed.py:147-151).
"""
import math
from collections import OrderedDict

import torch

FULL = 'full'      # whole axis
PREFIX = 'prefix'  # first n indices
GATHER = 'gather'  # explicit index tensor


class Axis:
    """One axis of a parameter slice."""
    __slots__ = ('kind', 'n', 'idx')

    def __init__(self, kind, n=None, idx=None):
        self.kind = kind
        self.n = n
        self.idx = idx

    @staticmethod
    def full(n):
        return Axis(FULL, n=n)

    @staticmethod
    def prefix(n):
        return Axis(PREFIX, n=n)

    @staticmethod
    def gather(idx):
        return Axis(GATHER, n=int(idx.numel()), idx=idx)

    def indices(self, device=None):
        """Materialize as an index tensor (for tests / RCCL padding masks)."""
        if self.kind == GATHER:
            return self.idx if device is None else self.idx.to(device)
        return torch.arange(self.n, device=device)

    def is_dense_prefix(self):
        return self.kind in (FULL, PREFIX)

    def __repr__(self):
        return f'Axis({self.kind}, n={self.n})'


class ParamSlice:
    """Slice spec for one parameter: out axis and (for dim>1) in axis."""
    __slots__ = ('out', 'inp')

    def __init__(self, out, inp=None):
        self.out = out
        self.inp = inp

    def __repr__(self):
        return f'ParamSlice(out={self.out}, inp={self.inp})'


def _ceil(x):
    return int(math.ceil(x))


class Federation:
    def __init__(self, global_parameters, rate, label_split, cfg):
        self.global_parameters = global_parameters
        self.rate = rate
        self.label_split = label_split
        self.cfg = cfg
        self.model_rate = None
        self.make_model_rate()

    # ------------------------------------------------------------------ rates
    def make_model_rate(self, generator=None):
        """Dynamic mode resamples each user's level per round
        (reference: src/fed.py:15-24).  Pass a seeded generator to keep the
        sampling identical across ranks without communication."""
        cfg = self.cfg
        if cfg['model_split_mode'] == 'dynamic':
            proportion = torch.tensor(cfg['proportion'])
            rate_idx = torch.multinomial(proportion, num_samples=cfg['num_users'],
                                         replacement=True, generator=generator).tolist()
            self.model_rate = [cfg['model_rate'][i] for i in rate_idx]
        elif cfg['model_split_mode'] == 'fix':
            self.model_rate = list(self.rate)
        else:
            raise ValueError('Not valid model split mode')

    # ------------------------------------------------------------- split maps
    def split_model(self, user_idx):
        name = self.cfg['model_name']
        if name == 'conv':
            return [self._split_conv(u) for u in user_idx]
        if 'resnet' in name:
            return [self._split_resnet(u) for u in user_idx]
        if name == 'transformer':
            return [self._split_transformer(u) for u in user_idx]
        raise ValueError('Not valid model name')

    def _scaler_rate(self, user, rate=None):
        """Width fraction of the slice: the user's current rate, or an
        explicit model rate (slice_for_rate)."""
        if rate is None:
            rate = self.model_rate[user]
        return rate / self.cfg['global_model_rate']

    def split_for_rate(self, rate):
        """Index map of the slice a client at `rate` receives."""
        name = self.cfg['model_name']
        if name == 'conv':
            return self._split_conv(None, rate)
        if 'resnet' in name:
            return self._split_resnet(None, rate)
        if name == 'transformer':
            return self._split_transformer(None, rate)
        raise ValueError('Not valid model name')

    def slice_for_rate(self, rate):
        """Global parameters sliced for `rate` — what distribute hands a
        client fixed at that rate — as a fresh OrderedDict of clones.  Goes
        through the per-tensor path, never the cached pack buffers of
        _pack_distribute, so the result aliases neither the global
        parameters nor a later distribute's output."""
        pidx = self.split_for_rate(rate)
        out = OrderedDict()
        for k, v in self.global_parameters.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype or 'bias' in ptype:
                out[k] = self._slice_value(v, pidx[k])
            else:
                out[k] = v.clone()
        return out

    def _split_conv(self, user, rate=None):
        """reference: src/fed.py:27-62 — slice output channels of every
        weight with dim>1; the final classifier keeps full rows."""
        gp = self.global_parameters
        weight_keys = [k for k in gp if 'weight' in k]
        bias_keys = [k for k in gp if 'bias' in k]
        output_weight_name = weight_keys[-1]
        output_bias_name = bias_keys[-1]
        rate = self._scaler_rate(user, rate)
        idx = OrderedDict()
        idx_i = None  # running output axis
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype:
                if v.dim() > 1:
                    if idx_i is None:
                        idx_i = Axis.full(v.size(1))
                    inp = idx_i
                    if k == output_weight_name:
                        out = Axis.full(v.size(0))
                    else:
                        out = Axis.prefix(_ceil(v.size(0) * rate))
                    idx[k] = ParamSlice(out, inp)
                    idx_i = out
                else:
                    idx[k] = ParamSlice(idx_i)
            elif 'bias' in ptype:
                idx[k] = ParamSlice(idx_i)
            # non weight/bias keys are skipped (distributed fully)
        return idx

    def _split_resnet(self, user, rate=None):
        """reference: src/fed.py:63-103 — conv1/conv2 sliced; shortcut reuses
        conv1's input index; linear keeps full output rows."""
        gp = self.global_parameters
        rate = self._scaler_rate(user, rate)
        idx = OrderedDict()
        idx_i = None
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype:
                if v.dim() > 1:
                    if 'conv1' in k or 'conv2' in k or 'conv3' in k:
                        # conv3 extends the reference rule (src/fed.py:82)
                        # to Bottleneck blocks, which the reference's fed
                        # path never exercised
                        if idx_i is None:
                            idx_i = Axis.full(v.size(1))
                        inp = idx_i
                        out = Axis.prefix(_ceil(v.size(0) * rate))
                        idx_i = out
                    elif 'shortcut' in k:
                        inp = idx[k.replace('shortcut', 'conv1')].inp
                        out = idx_i
                    elif 'linear' in k:
                        inp = idx_i
                        out = Axis.full(v.size(0))
                    else:
                        raise ValueError('Not valid k')
                    idx[k] = ParamSlice(out, inp)
                else:
                    idx[k] = ParamSlice(idx_i)
            elif 'bias' in ptype:
                if 'linear' in k:
                    idx[k] = ParamSlice(Axis.full(v.size(0)))
                else:
                    idx[k] = ParamSlice(idx_i)
        return idx

    def _split_transformer(self, user, rate=None):
        """reference: src/fed.py:104-156 — embedding slices the embedding dim
        keeping full vocab rows; q/k/v slice per head; decoder.linear2 keeps
        full vocab output; idx_i resets to the layer input after linear_q /
        linear_k biases so the residual stream stays at the sliced width."""
        gp = self.global_parameters
        num_heads = self.cfg['transformer']['num_heads']
        rate = self._scaler_rate(user, rate)
        idx = OrderedDict()
        idx_i = None
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype:
                if v.dim() > 1:
                    if 'embedding' in k.split('.')[-2]:
                        out = Axis.full(v.size(0))
                        inp = Axis.prefix(_ceil(v.size(1) * rate))
                        idx[k] = ParamSlice(out, inp)
                        idx_i = inp
                    elif 'decoder' in k and 'linear2' in k:
                        idx[k] = ParamSlice(Axis.full(v.size(0)), idx_i)
                    elif ('linear_q' in k) or ('linear_k' in k) or ('linear_v' in k):
                        inp = idx_i
                        head_dim = v.size(0) // num_heads
                        local_hd = _ceil(head_dim * rate)
                        out_idx = torch.arange(v.size(0)).reshape(
                            num_heads, -1)[:, :local_hd].reshape(-1)
                        out = Axis.gather(out_idx)
                        idx[k] = ParamSlice(out, inp)
                        idx_i = out
                    else:
                        inp = idx_i
                        out = Axis.prefix(_ceil(v.size(0) * rate))
                        idx[k] = ParamSlice(out, inp)
                        idx_i = out
                else:
                    idx[k] = ParamSlice(idx_i)
            elif 'bias' in ptype:
                if 'decoder' in k and 'linear2' in k:
                    idx[k] = ParamSlice(Axis.full(v.size(0)))
                elif ('linear_q' in k) or ('linear_k' in k) or ('linear_v' in k):
                    idx[k] = ParamSlice(idx_i)
                    if 'linear_v' not in k:
                        # reset the running index to this layer's INPUT axis
                        # (reference: src/fed.py:147-151)
                        idx_i = idx[k.replace('bias', 'weight')].inp
                else:
                    idx[k] = ParamSlice(idx_i)
        return idx

    # -------------------------------------------------------------- transport
    @staticmethod
    def _slice_value(v, ps):
        """Extract the slice a client receives."""
        if ps is None:
            return v.clone()
        if v.dim() > 1 and ps.inp is not None:
            out, inp = ps.out, ps.inp
            x = v
            if out.kind == PREFIX:
                x = x.narrow(0, 0, out.n)
            elif out.kind == GATHER:
                x = x.index_select(0, out.idx.to(v.device))
            if inp.kind == PREFIX:
                x = x.narrow(1, 0, inp.n)
            elif inp.kind == GATHER:
                x = x.index_select(1, inp.idx.to(v.device))
            return x.clone()
        out = ps.out
        if out.kind == FULL:
            return v.clone()
        if out.kind == PREFIX:
            return v.narrow(0, 0, out.n).clone()
        return v.index_select(0, out.idx.to(v.device)).clone()

    def distribute(self, user_idx, resample=True, generator=None,
                   slots=None):
        """reference: src/fed.py:161-178 — resample rates, build index maps,
        and hand each client its parameter slices.  Set resample=False when
        the engine already resampled rates (e.g. with a shared seeded
        generator for multi-rank determinism).  ``slots`` restricts the
        tensor slicing to this rank's clients (index maps are still built
        for every slot — combine needs only the local ones, but they are
        cheap); other slots get None.

        On GPU with the native extension, every dense-prefix slice is
        packed by ONE HIP kernel launch over a cached descriptor table
        (K13 of SURVEY §2b) instead of per-parameter narrow+clone calls;
        transformer per-head GATHER slices and non-fp32 buffers keep the
        per-tensor path."""
        if resample:
            self.make_model_rate(generator)
        param_idx = self.split_model(user_idx)
        want = list(range(len(user_idx))) if slots is None else list(slots)
        local_parameters = [None] * len(user_idx)
        packed = self._pack_distribute(user_idx, param_idx, want)
        if packed is not None:
            for m, lp in packed.items():
                local_parameters[m] = lp
            return local_parameters, param_idx
        for m in want:
            lp = OrderedDict()
            for k, v in self.global_parameters.items():
                ptype = k.split('.')[-1]
                if 'weight' in ptype or 'bias' in ptype:
                    lp[k] = self._slice_value(v, param_idx[m][k])
                else:
                    lp[k] = v.clone()
            local_parameters[m] = lp
        return local_parameters, param_idx

    def _pack_distribute(self, user_idx, param_idx, want):
        """One-kernel slice pack (see distribute).  Returns
        {slot: OrderedDict} or None when inapplicable.  Descriptors and
        destination buffers are cached per (slot -> rate) assignment —
        global master data_ptrs are stable (finalize writes in place)."""
        from .. import ops as native_ops
        gp = self.global_parameters
        first = next(iter(gp.values()))
        if not (first.is_cuda and native_ops.use_native(first)
                and native_ops.native_available()):
            return None
        key = tuple((m, self.model_rate[user_idx[m]]) for m in want)
        cache = getattr(self, '_pack_cache', None)
        if cache is None:
            from collections import OrderedDict as _OD
            cache = self._pack_cache = _OD()
        hit = cache.get(key)
        if hit is not None:
            cache.move_to_end(key)
        if hit is None:
            # dynamic mode draws a fresh rate assignment every round: cap
            # the descriptor/buffer cache (each entry owns the slots' dst
            # tensors) so it cannot grow with the round count
            while len(cache) >= 48:
                cache.popitem(last=False)
            import numpy as np
            desc_dt = np.dtype([('src', 'u8'), ('dst', 'u8'), ('rows', 'i4'),
                                ('cols', 'i4'), ('stride', 'i4'),
                                ('pad', 'i4')])
            descs = []
            outs = {}
            extras = []   # (slot, key, ps) handled per-tensor (gather/non-f32)
            max_rows = 1
            for m in want:
                lp = OrderedDict()
                for k, v in gp.items():
                    ptype = k.split('.')[-1]
                    ps = param_idx[m][k] if ('weight' in ptype
                                             or 'bias' in ptype) else None
                    sliceable = (v.dtype == torch.float32
                                 and ps is not None and ps.out is not None
                                 and ps.out.is_dense_prefix()
                                 and (ps.inp is None
                                      or ps.inp.is_dense_prefix()))
                    if ('weight' in ptype or 'bias' in ptype) and sliceable:
                        if v.dim() > 1 and ps.inp is not None:
                            rows = ps.out.n
                            cols = ps.inp.n * (v.numel() // (v.size(0)
                                                             * v.size(1)))
                            stride = v.numel() // v.size(0)
                            # inner-dims contiguity: prefix on dim 1 of a
                            # 4-D conv weight is contiguous only if we copy
                            # (inp.n * kh * kw) elems from each row start —
                            # true because dims 2+ are always FULL
                            dst = torch.empty(
                                (rows,) + (ps.inp.n,) + tuple(v.shape[2:]),
                                dtype=v.dtype, device=v.device)
                        else:
                            rows = 1
                            cols = ps.out.n
                            stride = cols
                            dst = torch.empty(ps.out.n, dtype=v.dtype,
                                              device=v.device)
                        descs.append((v.data_ptr(), dst.data_ptr(), rows,
                                      cols, stride, 0))
                        max_rows = max(max_rows, rows)
                        lp[k] = dst
                    else:
                        extras.append((m, k, ps))
                        lp[k] = None
                outs[m] = lp
            if descs:
                blob = torch.from_numpy(
                    np.array(descs, dtype=desc_dt).view(np.uint8)).to(
                        first.device)
            else:
                blob = torch.empty(0, dtype=torch.uint8, device=first.device)
            hit = cache[key] = (blob, len(descs), max_rows, outs, extras)
        blob, n, max_rows, outs, extras = hit
        if n:
            ext = native_ops.require_native()
            ext.pack_slices(blob, n, max_rows)
        for m, k, ps in extras:
            v = gp[k]
            ptype = k.split('.')[-1]
            if 'weight' in ptype or 'bias' in ptype:
                outs[m][k] = self._slice_value(v, ps)
            else:
                outs[m][k] = v.clone()
        return outs

    # --------------------------------------------------------------- combine
    def _output_layer_kind(self, k, weight_keys, bias_keys):
        """Which parameters get label-split row filtering in combine
        (reference: src/fed.py:193-198, 228-233, 263-274)."""
        name = self.cfg['model_name']
        if name == 'conv':
            if k == weight_keys[-1] or k == bias_keys[-1]:
                return True
        elif 'resnet' in name:
            if 'linear' in k:
                return True
        elif name == 'transformer':
            if k.split('.')[-2] == 'embedding' and k.split('.')[-1] == 'weight':
                return True
            if 'decoder' in k and 'linear2' in k:
                return True
        return False

    @staticmethod
    def _accumulate(tmp, cnt, ps, val):
        """tmp[slice] += val; cnt[slice] += 1 for one client's parameter."""
        if ps is None or ps.out is None:
            tmp += val
            cnt += 1
            return
        out, inp = ps.out, ps.inp
        if inp is not None and tmp.dim() > 1:
            if out.is_dense_prefix() and inp.is_dense_prefix():
                tmp[:out.n, :inp.n] += val
                cnt[:out.n, :inp.n] += 1
            elif inp.is_dense_prefix():
                oidx = out.indices(tmp.device)
                view_t = tmp.narrow(1, 0, inp.n)
                view_c = cnt.narrow(1, 0, inp.n)
                view_t.index_add_(0, oidx, val.to(view_t.dtype))
                view_c.index_add_(0, oidx, torch.ones_like(val, dtype=view_c.dtype))
            else:
                oidx = out.indices(tmp.device).unsqueeze(1)
                iidx = inp.indices(tmp.device).unsqueeze(0)
                tmp.index_put_((oidx, iidx), val.to(tmp.dtype), accumulate=True)
                cnt.index_put_((oidx, iidx),
                               torch.ones_like(val, dtype=cnt.dtype), accumulate=True)
        else:
            if out.is_dense_prefix():
                tmp[:out.n] += val
                cnt[:out.n] += 1
            else:
                oidx = out.indices(tmp.device)
                tmp.index_add_(0, oidx, val.to(tmp.dtype))
                cnt.index_add_(0, oidx, torch.ones_like(val, dtype=cnt.dtype))

    def accumulate(self, local_parameters, param_idx, user_idx, slots=None):
        """Build the fp32 zero-padded accumulator + count for a subset of the
        round's clients.  ``slots`` indexes into user_idx/param_idx;
        local_parameters maps slot -> state_dict (a list works too).

        This is the per-rank half of the padded-RCCL combine (SURVEY §2b
        K14): accumulators are global-shaped, so summing them across ranks
        and dividing reproduces the sequential combine exactly.
        """
        gp = self.global_parameters
        weight_keys = [k for k in gp if 'weight' in k]
        bias_keys = [k for k in gp if 'bias' in k]
        if slots is None:
            slots = range(len(param_idx))
        tmp_d, cnt_d = OrderedDict(), OrderedDict()
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            tmp = torch.zeros(v.size(), dtype=torch.float32, device=v.device)
            cnt = torch.zeros(v.size(), dtype=torch.float32, device=v.device)
            is_output = self._output_layer_kind(k, weight_keys, bias_keys)
            for m in slots:
                val = local_parameters[m][k]
                if 'weight' in ptype or 'bias' in ptype:
                    ps = param_idx[m][k]
                    if is_output and ps is not None and ps.out is not None:
                        label_split = torch.tensor(self.label_split[user_idx[m]])
                        out_idx = ps.out.indices()[label_split]
                        ps = ParamSlice(Axis.gather(out_idx), ps.inp)
                        val = val[label_split]
                    self._accumulate(tmp, cnt, ps, val.float())
                else:
                    tmp += val.float()
                    cnt += 1
            tmp_d[k] = tmp
            cnt_d[k] = cnt
        return tmp_d, cnt_d

    @staticmethod
    def _count_only(cnt, ps):
        """cnt[slice] += 1 for one client's parameter (no values)."""
        if ps is None or ps.out is None:
            cnt += 1
            return
        out, inp = ps.out, ps.inp
        if inp is not None and cnt.dim() > 1:
            if out.is_dense_prefix() and inp.is_dense_prefix():
                cnt[:out.n, :inp.n] += 1
            elif inp.is_dense_prefix():
                oidx = out.indices(cnt.device)
                cnt.narrow(1, 0, inp.n).index_add_(
                    0, oidx, torch.ones(oidx.numel(), inp.n, dtype=cnt.dtype,
                                        device=cnt.device))
            else:
                oidx = out.indices(cnt.device).unsqueeze(1)
                iidx = inp.indices(cnt.device).unsqueeze(0)
                ones = torch.ones(oidx.numel(), iidx.numel(), dtype=cnt.dtype,
                                  device=cnt.device)
                cnt.index_put_((oidx, iidx), ones, accumulate=True)
        else:
            if out.is_dense_prefix():
                cnt[:out.n] += 1
            else:
                oidx = out.indices(cnt.device)
                cnt.index_add_(0, oidx, torch.ones(oidx.numel(),
                                                   dtype=cnt.dtype,
                                                   device=cnt.device))

    def count_map(self, param_idx, user_idx, slots=None):
        """The count half of the combine, computed from index maps alone.

        Counts depend only on (param_idx, label_split, user_idx) — never on
        client parameter VALUES — and every rank builds param_idx for ALL of
        the round's clients (distribute slices tensors per-slot but index
        maps are global).  So in the multi-rank combine each rank can derive
        the full count tensor locally and the collective only has to move
        the value accumulators: half the payload of reducing counts too,
        bit-exactly (parallel/dist.py:distributed_combine).
        """
        gp = self.global_parameters
        weight_keys = [k for k in gp if 'weight' in k]
        bias_keys = [k for k in gp if 'bias' in k]
        if slots is None:
            slots = range(len(param_idx))
        cnt_d = OrderedDict()
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            cnt = torch.zeros(v.size(), dtype=torch.float32, device=v.device)
            is_output = self._output_layer_kind(k, weight_keys, bias_keys)
            for m in slots:
                if 'weight' in ptype or 'bias' in ptype:
                    ps = param_idx[m][k]
                    if is_output and ps is not None and ps.out is not None:
                        label_split = torch.tensor(self.label_split[user_idx[m]])
                        out_idx = ps.out.indices()[label_split]
                        ps = ParamSlice(Axis.gather(out_idx), ps.inp)
                    self._count_only(cnt, ps)
                else:
                    cnt += 1
            cnt_d[k] = cnt
        return cnt_d

    def finalize(self, tmp_d, cnt_d):
        """Masked count-weighted average written in place into the global
        tensors (reference: src/fed.py:217-218)."""
        for k, v in self.global_parameters.items():
            cnt = cnt_d[k]
            mask = cnt > 0
            avg = tmp_d[k] / cnt.clamp(min=1)
            v.copy_(torch.where(mask, avg, v.float()).to(v.dtype))

    def combine(self, local_parameters, param_idx, user_idx):
        """Sequential (single-process) combine (reference: src/fed.py:180-298)."""
        tmp_d, cnt_d = self.accumulate(local_parameters, param_idx, user_idx)
        self.finalize(tmp_d, cnt_d)
