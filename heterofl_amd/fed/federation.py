"""Federation core: width-sliced subnetwork distribute / combine.

Re-implements the semantics of the reference Federation (reference:
src/fed.py:8-298) with a typed index-map representation instead of
per-parameter torch.meshgrid gathers:

- every slice the HeteroFL rules produce is either FULL (whole axis),
  PREFIX(n) (the first n indices — conv/resnet channel slicing and
  transformer non-qkv slicing), GATHER(tensor) (transformer per-head
  slicing and label-split-filtered output rows), or ROLL(n, size, shift)
  (the window (shift + j) % size, j < n — rolling sub-model extraction,
  cfg['submodel'] = 'roll': every PREFIX axis becomes a window that moves
  by cfg['roll_step'] positions per round, so all global channels are
  trained evenly instead of only the lowest ones).
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
ROLL = 'roll'      # n indices (shift + j) % size: a window that may wrap


class Axis:
    """One axis of a parameter slice."""
    __slots__ = ('kind', 'n', 'idx', 'size', 'shift', 'period', 'take')

    def __init__(self, kind, n=None, idx=None, size=None, shift=0,
                 period=None, take=None):
        self.kind = kind
        self.n = n
        self.idx = idx
        self.size = size      # ROLL: the global axis size
        self.shift = shift    # ROLL / per-head GATHER: window start
        self.period = period  # per-head GATHER: head_dim
        self.take = take      # per-head GATHER: indices taken per head

    @staticmethod
    def full(n):
        return Axis(FULL, n=n)

    @staticmethod
    def prefix(n):
        return Axis(PREFIX, n=n)

    @staticmethod
    def gather(idx):
        return Axis(GATHER, n=int(idx.numel()), idx=idx)

    @staticmethod
    def roll(n, size, shift):
        """The n indices (shift + j) % size, j = 0..n-1."""
        return Axis(ROLL, n=n, size=size, shift=shift % size)

    @staticmethod
    def heads(num_heads, head_dim, take, shift=0):
        """Per-head GATHER: head h contributes h * head_dim +
        (shift + j) % head_dim for j < take.  Keeps the window parameters
        next to the index tensor so the native kernels can describe the
        axis without reading it."""
        shift = shift % head_dim
        j = (shift + torch.arange(take)) % head_dim
        idx = (torch.arange(num_heads).unsqueeze(1) * head_dim
               + j.unsqueeze(0)).reshape(-1)
        return Axis(GATHER, n=int(idx.numel()), idx=idx, shift=shift,
                    period=head_dim, take=take)

    def indices(self, device=None):
        """Materialize as an index tensor (for tests / RCCL padding masks)."""
        if self.kind == GATHER:
            return self.idx if device is None else self.idx.to(device)
        if self.kind == ROLL:
            return (self.shift + torch.arange(self.n, device=device)) \
                % self.size
        return torch.arange(self.n, device=device)

    def is_dense_prefix(self):
        return self.kind in (FULL, PREFIX)

    def window(self, size):
        """(period, shift, take) of the periodic window that maps local
        index j of this axis of a `size`-long global axis to
        (j // take) * period + (shift + j % take) % period, or None for a
        GATHER that is no such window."""
        if self.kind == FULL:
            return size, 0, size
        if self.kind == PREFIX:
            return size, 0, self.n
        if self.kind == ROLL:
            return size, self.shift, self.n
        if self.period is None:
            return None
        return self.period, self.shift, self.take

    def __repr__(self):
        if self.kind == ROLL:
            return f'Axis({self.kind}, n={self.n}, size={self.size}, ' \
                   f'shift={self.shift})'
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
        if cfg.get('submodel', 'static') not in ('static', 'roll'):
            raise ValueError('Not valid submodel mode')
        self.model_rate = None
        self.make_model_rate()
        # Diagnostics of the last call, reset on every call (tests and A/B
        # scripts read them; nothing in the engine depends on them):
        # distribute -> last_pack_route 'static' / 'roll' (the one-launch
        # pack kernels) or 'torch' (per-tensor), and, on the roll route
        # only, last_pack_per_tensor: the (slot, key) pairs the kernel did
        # not pack (None on the other routes);
        # accumulate -> last_combine_route 'kernel' / 'torch' and
        # last_combine_keys: the keys that came from combine_accumulate.
        self.last_pack_route = None
        self.last_pack_per_tensor = None
        self.last_combine_route = None
        self.last_combine_keys = []

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
    def split_model(self, user_idx, round=None):
        """Index maps of the round's clients.  ``round`` is the global
        epoch number; it moves the windows under cfg['submodel'] = 'roll'
        and is ignored under 'static'."""
        name = self.cfg['model_name']
        if name == 'conv':
            return [self._split_conv(u, round=round) for u in user_idx]
        if 'resnet' in name:
            return [self._split_resnet(u, round=round) for u in user_idx]
        if name == 'transformer':
            return [self._split_transformer(u, round=round)
                    for u in user_idx]
        raise ValueError('Not valid model name')

    def _roll_base(self, round):
        """Unreduced shift of a round: (round - 1) * roll_step, or None when
        the windows do not move (static mode, or no round given).  Each axis
        reduces it modulo its own period.  All clients of a round share it,
        so windows of different rates stay nested and axes of equal global
        size select the same channels."""
        if round is None or self.cfg.get('submodel', 'static') != 'roll':
            return None
        return (int(round) - 1) * int(self.cfg.get('roll_step', 1))

    @staticmethod
    def _window(n, size, base):
        """The axis that is PREFIX(n) today, at a round's shift: FULL when
        it covers the whole axis (a full-width client never receives a
        permuted model), PREFIX(n) at shift 0, ROLL otherwise."""
        if base is None:
            return Axis.prefix(n)
        if n == size:
            return Axis.full(size)
        shift = base % size
        if shift == 0:
            return Axis.prefix(n)
        return Axis.roll(n, size, shift)

    def _scaler_rate(self, user, rate=None):
        """Width fraction of the slice: the user's current rate, or an
        explicit model rate (slice_for_rate)."""
        if rate is None:
            rate = self.model_rate[user]
        return rate / self.cfg['global_model_rate']

    def split_for_rate(self, rate, round=None):
        """Index map of the slice a client at `rate` receives (in `round`,
        under roll mode)."""
        name = self.cfg['model_name']
        if name == 'conv':
            return self._split_conv(None, rate, round=round)
        if 'resnet' in name:
            return self._split_resnet(None, rate, round=round)
        if name == 'transformer':
            return self._split_transformer(None, rate, round=round)
        raise ValueError('Not valid model name')

    def slice_for_rate(self, rate, round=None):
        """Global parameters sliced for `rate` — what distribute hands a
        client fixed at that rate (in `round`, under roll mode) — as a fresh
        OrderedDict of clones.  Goes through the per-tensor path, never the
        cached pack buffers of _pack_distribute, so the result aliases
        neither the global parameters nor a later distribute's output."""
        pidx = self.split_for_rate(rate, round=round)
        out = OrderedDict()
        for k, v in self.global_parameters.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype or 'bias' in ptype:
                out[k] = self._slice_value(v, pidx[k])
            else:
                out[k] = v.clone()
        return out

    def _split_conv(self, user, rate=None, round=None):
        """reference: src/fed.py:27-62 — slice output channels of every
        weight with dim>1; the final classifier keeps full rows."""
        gp = self.global_parameters
        weight_keys = [k for k in gp if 'weight' in k]
        bias_keys = [k for k in gp if 'bias' in k]
        output_weight_name = weight_keys[-1]
        output_bias_name = bias_keys[-1]
        rate = self._scaler_rate(user, rate)
        base = self._roll_base(round)
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
                        out = self._window(_ceil(v.size(0) * rate),
                                           v.size(0), base)
                    idx[k] = ParamSlice(out, inp)
                    idx_i = out
                else:
                    idx[k] = ParamSlice(idx_i)
            elif 'bias' in ptype:
                idx[k] = ParamSlice(idx_i)
            # non weight/bias keys are skipped (distributed fully)
        return idx

    def _split_resnet(self, user, rate=None, round=None):
        """reference: src/fed.py:63-103 — conv1/conv2 sliced; shortcut reuses
        conv1's input index; linear keeps full output rows."""
        gp = self.global_parameters
        rate = self._scaler_rate(user, rate)
        base = self._roll_base(round)
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
                        out = self._window(_ceil(v.size(0) * rate),
                                           v.size(0), base)
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

    def _split_transformer(self, user, rate=None, round=None):
        """reference: src/fed.py:104-156 — embedding slices the embedding dim
        keeping full vocab rows; q/k/v slice per head; decoder.linear2 keeps
        full vocab output; idx_i resets to the layer input after linear_q /
        linear_k biases so the residual stream stays at the sliced width."""
        gp = self.global_parameters
        num_heads = self.cfg['transformer']['num_heads']
        rate = self._scaler_rate(user, rate)
        base = self._roll_base(round)
        idx = OrderedDict()
        idx_i = None
        for k, v in gp.items():
            ptype = k.split('.')[-1]
            if 'weight' in ptype:
                if v.dim() > 1:
                    if 'embedding' in k.split('.')[-2]:
                        out = Axis.full(v.size(0))
                        inp = self._window(_ceil(v.size(1) * rate),
                                           v.size(1), base)
                        idx[k] = ParamSlice(out, inp)
                        idx_i = inp
                    elif 'decoder' in k and 'linear2' in k:
                        idx[k] = ParamSlice(Axis.full(v.size(0)), idx_i)
                    elif ('linear_q' in k) or ('linear_k' in k) or ('linear_v' in k):
                        inp = idx_i
                        head_dim = v.size(0) // num_heads
                        local_hd = _ceil(head_dim * rate)
                        # the window rolls inside each head (period
                        # head_dim); a head taken whole is not permuted
                        shift = 0 if base is None or local_hd == head_dim \
                            else base % head_dim
                        out = Axis.heads(num_heads, head_dim, local_hd,
                                         shift)
                        idx[k] = ParamSlice(out, inp)
                        idx_i = out
                    else:
                        inp = idx_i
                        out = self._window(_ceil(v.size(0) * rate),
                                           v.size(0), base)
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
            elif out.kind in (GATHER, ROLL):
                x = x.index_select(0, out.indices(v.device))
            if inp.kind == PREFIX:
                x = x.narrow(1, 0, inp.n)
            elif inp.kind in (GATHER, ROLL):
                x = x.index_select(1, inp.indices(v.device))
            return x.clone()
        out = ps.out
        if out.kind == FULL:
            return v.clone()
        if out.kind == PREFIX:
            return v.narrow(0, 0, out.n).clone()
        return v.index_select(0, out.indices(v.device)).clone()

    def distribute(self, user_idx, resample=True, generator=None,
                   slots=None, round=None):
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
        per-tensor path.

        ``round`` is the global epoch number.  Under cfg['submodel'] =
        'roll' it places the extraction windows (shift (round - 1) *
        roll_step modulo each axis' period; round 1 and round=None are the
        static prefixes), and the native route is pack_slices_roll: one
        launch packs every fp32 weight and bias, rolled and per-head q/k/v
        slices included, from a descriptor table rebuilt from this call's
        index maps.

        Lifetime of the result on the native routes: the tensors handed out
        are cached destination buffers — one set per (slot -> rate)
        assignment in static mode, one per (slot, rate) in roll mode — and
        a later distribute that hands a slot the same rate packs into the
        SAME tensors.  They may be trained in place (the next pack
        overwrites them), but a caller that needs a round's slices or the
        states trained in them after the next distribute must clone them
        first.  slice_for_rate and the torch route return fresh clones."""
        if resample:
            self.make_model_rate(generator)
        param_idx = self.split_model(user_idx, round=round)
        want = list(range(len(user_idx))) if slots is None else list(slots)
        local_parameters = [None] * len(user_idx)
        self.last_pack_per_tensor = None
        if self.cfg.get('submodel', 'static') == 'roll':
            packed = self._pack_distribute_roll(user_idx, param_idx, want)
        else:
            packed = self._pack_distribute(user_idx, param_idx, want)
        self.last_pack_route = 'torch' if packed is None else \
            'roll' if self.cfg.get('submodel', 'static') == 'roll' else \
            'static'
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

    def _native_ready(self):
        """GPU-resident global parameters, the extension built, and no
        HETEROFL_FORCE_EAGER: the condition of the native routes."""
        from .. import ops as native_ops
        first = next(iter(self.global_parameters.values()))
        return (first.is_cuda and native_ops.use_native(first)
                and native_ops.native_available())

    def _pack_roll_slot(self, pidx, span_dt):
        """Destination buffers of one slot at one rate, with the parts of
        their spans that depend on the slice shapes only: (OrderedDict key
        -> buffer or None, [(key, is 2-D)], span array)."""
        import numpy as np
        lp, packed, rows_l = OrderedDict(), [], []
        for k, v in self.global_parameters.items():
            ptype = k.split('.')[-1]
            ps = pidx[k] if ('weight' in ptype or 'bias' in ptype) else None
            lp[k] = None
            if not (v.dtype == torch.float32 and ps is not None
                    and ps.out is not None and v.dim() >= 1
                    and v.is_contiguous()):
                continue
            two_d = v.dim() > 1 and ps.inp is not None
            # a 1-D tensor is one row whose columns are its out axis
            if two_d:
                O, I = v.size(0), v.size(1)
                n_out, n_in = ps.out.n, ps.inp.n
                shape = (n_out, n_in) + tuple(v.shape[2:])
            else:
                O, I = 1, v.size(0)
                n_out, n_in = 1, ps.out.n
                shape = (n_in,) + tuple(v.shape[1:])
            inner = v.numel() // (O * I)
            dst = torch.empty(shape, dtype=v.dtype, device=v.device)
            lp[k] = dst
            rpb = max(1, 4096 // max(n_in * inner, 1))
            packed.append((k, two_d))
            rows_l.append((v.data_ptr(), dst.data_ptr(), (O, 0, 0, 0),
                           (I, 0, 0, 0), n_out, n_in, inner, rpb))
        return lp, packed, np.array(rows_l, dtype=span_dt)

    def _pack_distribute_roll(self, user_idx, param_idx, want):
        """One-kernel pack of periodic-window slices (roll mode; see
        distribute).  Returns {slot: OrderedDict} or None when inapplicable.
        Destination buffers depend only on the slice shapes, so they are
        cached per (slot, rate) — a slot keeps one buffer set per rate it has
        held, whatever the other slots hold — and the block table per
        (slot -> rate) assignment; the span table carries the windows and
        is rebuilt from this round's param_idx on every call."""
        from .. import ops as native_ops
        gp = self.global_parameters
        first = next(iter(gp.values()))
        if not self._native_ready():
            return None
        import numpy as np
        span_dt = np.dtype([('src', 'u8'), ('dst', 'u8'), ('out', 'i4', 4),
                            ('inp', 'i4', 4), ('rows', 'i4'), ('cols', 'i4'),
                            ('inner', 'i4'), ('rpb', 'i4')])
        key = tuple((m, self.model_rate[user_idx[m]]) for m in want)
        slot_cache = getattr(self, '_pack_roll_slots', None)
        # cached spans hold the global tensors' addresses (finalize writes
        # in place, so they are stable); start over if they ever move
        srcs = tuple(v.data_ptr() for v in gp.values())
        if slot_cache is None or self._pack_roll_srcs != srcs:
            slot_cache = self._pack_roll_slots = OrderedDict()
            self._pack_roll_cache = OrderedDict()
            self._pack_roll_srcs = srcs
        outs, packed, bases = {}, [], []
        for sk in key:
            ent = slot_cache.get(sk)
            if ent is not None:
                slot_cache.move_to_end(sk)
            else:
                ent = slot_cache[sk] = self._pack_roll_slot(
                    param_idx[sk[0]], span_dt)
            outs[sk[0]] = ent[0]
            packed.extend((sk[0], k, two_d) for k, two_d in ent[1])
            bases.append(ent[2])
        # one buffer set per slot and width level is the whole working set
        # of dynamic mode, where a slot may hold any level in any round; the
        # slots of this call were just touched, so they survive an eviction
        levels = len(set(self.cfg['model_rate']))
        while len(slot_cache) > max(48, len(key) * levels):
            slot_cache.popitem(last=False)
        base = np.concatenate(bases) if bases else np.zeros(0, span_dt)
        cache = self._pack_roll_cache
        blk = cache.get(key)
        if blk is not None:
            cache.move_to_end(key)
        else:
            # same cap as _pack_distribute: dynamic mode draws a fresh rate
            # assignment every round.  blocks[b] = (span, first row), each
            # block copying rows_per_block rows
            while len(cache) >= 48:
                cache.popitem(last=False)
            n_blk = (base['rows'] + base['rpb'] - 1) // base['rpb']
            span_of = np.repeat(np.arange(len(base), dtype=np.int64), n_blk)
            first_blk = np.cumsum(n_blk) - n_blk
            row0 = (np.arange(span_of.size) - first_blk[span_of]) \
                * base['rpb'][span_of]
            blk = cache[key] = torch.from_numpy(np.stack(
                [span_of, row0], 1).astype(np.int32)).to(first.device)
        # this round's windows, from this round's maps
        unit = (1, 0, 1)
        ow_l, iw_l, extras = [], [], set()
        for d, (m, k, two_d) in enumerate(packed):
            ps = param_idx[m][k]
            if two_d:
                ow = ps.out.window(int(base['out'][d, 0]))
                iw = ps.inp.window(int(base['inp'][d, 0]))
            else:
                ow, iw = unit, ps.out.window(int(base['inp'][d, 0]))
            if ow is None or iw is None:
                extras.add((m, k))   # arbitrary gather: per-tensor
                ow = iw = unit
            ow_l.append(ow)
            iw_l.append(iw)
        spans = base.copy()
        if len(packed):
            spans['out'][:, 1:] = np.array(ow_l, dtype=np.int32)
            spans['inp'][:, 1:] = np.array(iw_l, dtype=np.int32)
            live = np.array([(m, k) not in extras for m, k, _ in packed]) \
                if extras else np.ones(len(packed), dtype=bool)
            spans['rows'][~live] = 0   # copies nothing
            # the cached buffers must have this round's slice shapes and
            # the windows must stay inside the global tensors
            for ax, n in (('out', 'rows'), ('inp', 'cols')):
                size, period, shift, take = (spans[ax][live, i]
                                             for i in range(4))
                if not ((period >= 1).all() and (size % period == 0).all()
                        and (shift >= 0).all() and (shift < period).all()
                        and (take >= 1).all() and (take <= period).all()
                        and ((size // period) * take
                             == base[n][live]).all()):
                    raise RuntimeError(
                        'pack_slices_roll: a window does not match its '
                        'cached slice buffer')
            ext = native_ops.require_native()
            ext.pack_slices_roll(
                torch.from_numpy(spans.view(np.uint8)).to(first.device),
                len(packed), blk)
        packed_keys = {(m, k) for m, k, _ in packed} - extras
        result = {}
        per_tensor = []
        for m in want:
            lp = OrderedDict(outs[m])
            for k, v in gp.items():
                if (m, k) in packed_keys:
                    continue
                per_tensor.append((m, k))
                ptype = k.split('.')[-1]
                if 'weight' in ptype or 'bias' in ptype:
                    lp[k] = self._slice_value(v, param_idx[m][k])
                else:
                    lp[k] = v.clone()
            result[m] = lp
        # (slot, key) pairs that did not come from the kernel
        self.last_pack_per_tensor = per_tensor
        return result

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

    def _native_combine_wanted(self):
        """Route of accumulate: the combine_accumulate kernel is considered
        only on GPU with the native extension — by default under
        cfg['submodel'] = 'roll', whose maps would otherwise take the
        index_add_/index_put_ paths; HETEROFL_NATIVE_COMBINE=1 opts static
        mode in (A/B), =0 forces the torch loop.  Read on every call."""
        import os
        if not self._native_ready():
            return False
        knob = os.environ.get('HETEROFL_NATIVE_COMBINE')
        if knob == '0':
            return False
        return knob == '1' or self.cfg.get('submodel', 'static') == 'roll'

    def _accumulate_native(self, local_parameters, param_idx, user_idx, slots,
                           weight_keys, bias_keys):
        """{key: (tmp, cnt)} from one combine_accumulate launch for every
        fp32 key whose client maps are periodic windows (all that the three
        rule sets produce); the other keys are left to the torch loop.  The
        label-split filter of the output layers travels as a row mask."""
        import numpy as np
        from ..ops.fused import combine_accumulate
        gp = self.global_parameters
        keys, shapes, clients = [], [], []
        row_masks = {}
        for k, v in gp.items():
            if v.dtype != torch.float32 or v.dim() < 1:
                continue
            ptype = k.split('.')[-1]
            sliced = 'weight' in ptype or 'bias' in ptype
            is_output = self._output_layer_kind(k, weight_keys, bias_keys)
            O = v.size(0)
            I = v.size(1) if v.dim() > 1 else 1
            ents = []
            for m in slots:
                val = local_parameters[m][k]
                ps = param_idx[m][k] if sliced else None
                if val.dtype != torch.float32 or val.device != v.device:
                    ents = None
                    break
                if ps is None or ps.out is None:
                    ow, iw, mask = (O, 0, O), None, None
                else:
                    ow = ps.out.window(O)
                    # a 2-D tensor sliced on its out axis only (ps.inp None)
                    # keeps its whole in axis, like the torch path
                    iw = ps.inp.window(I) if (ps.inp is not None
                                              and v.dim() > 1) else None
                    if ow is None or (ps.inp is not None and v.dim() > 1
                                      and iw is None):
                        ents = None
                        break
                    mask = None
                    if is_output:
                        ls = self.label_split[user_idx[m]]
                        if len(set(ls)) != len(ls):
                            ents = None   # repeated labels add twice in
                            break         # the torch loop; keep it there
                        mkey = (m, ps.out.n)
                        mask = row_masks.get(mkey)
                        if mask is None:
                            mask = np.zeros(ps.out.n, dtype=np.uint8)
                            mask[np.asarray(ls, dtype=np.int64)] = 1
                            row_masks[mkey] = mask
                ents.append((val, ow, iw, mask))
            if ents is None:
                continue
            keys.append(k)
            shapes.append(v.shape)
            clients.append(ents)
        if not keys:
            return {}
        first = gp[keys[0]]
        tmps, cnts = combine_accumulate(shapes, clients, first.device)
        return {k: (t, c) for k, t, c in zip(keys, tmps, cnts)}

    def accumulate(self, local_parameters, param_idx, user_idx, slots=None):
        """Build the fp32 zero-padded accumulator + count for a subset of the
        round's clients.  ``slots`` indexes into user_idx/param_idx;
        local_parameters maps slot -> state_dict (a list works too).

        On GPU with the native extension the fp32 keys come from ONE
        combine_accumulate launch (see _native_combine_wanted for the
        routing), bit-identical to the torch loop below, which stays the CPU
        path and the oracle.

        This is the per-rank half of the padded-RCCL combine (SURVEY §2b
        K14): accumulators are global-shaped, so summing them across ranks
        and dividing reproduces the sequential combine exactly.
        """
        gp = self.global_parameters
        weight_keys = [k for k in gp if 'weight' in k]
        bias_keys = [k for k in gp if 'bias' in k]
        if slots is None:
            slots = range(len(param_idx))
        slots = list(slots)
        native = self._accumulate_native(local_parameters, param_idx,
                                         user_idx, slots, weight_keys,
                                         bias_keys) \
            if self._native_combine_wanted() else {}
        self.last_combine_route = 'kernel' if native else 'torch'
        self.last_combine_keys = list(native)
        tmp_d, cnt_d = OrderedDict(), OrderedDict()
        for k, v in gp.items():
            if k in native:
                tmp_d[k], cnt_d[k] = native[k]
                continue
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
                # conv weights carry (kh, kw) behind the two sliced axes
                cnt.narrow(1, 0, inp.n).index_add_(
                    0, oidx, torch.ones((oidx.numel(), inp.n)
                                        + tuple(cnt.shape[2:]),
                                        dtype=cnt.dtype, device=cnt.device))
            else:
                oidx = out.indices(cnt.device).unsqueeze(1)
                iidx = inp.indices(cnt.device).unsqueeze(0)
                ones = torch.ones((oidx.numel(), iidx.numel())
                                  + tuple(cnt.shape[2:]), dtype=cnt.dtype,
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
