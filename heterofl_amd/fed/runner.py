"""Federated round orchestration.

Drives the reference round structure (src/train_classifier_fed.py:74-94):
sample active clients -> distribute slices -> local training -> combine ->
sBN statistics pass -> evaluation -> checkpoint.  The local-training engine
is pluggable: 'sequential' (reference-faithful oracle) or 'batched'
(MI355X fast path, clients of one rate trained in one grouped model).

Multi-rank operation (one process per GPU over RCCL): active clients are
sharded across ranks; every rank samples identical user_idx and dynamic
rates from a round-seeded generator, trains its shard, and combine runs as
a padded all-reduce (see parallel/dist.py).
"""
import math
import os
import time

import numpy as np
import torch

_TIMING = os.environ.get('HETEROFL_TIMING') == '1'


class _phase_timer:
    acc = {}

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _TIMING:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        return self

    def __exit__(self, *a):
        if _TIMING:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dt = time.perf_counter() - self.t0
            _phase_timer.acc[self.name] = _phase_timer.acc.get(self.name, 0.0) + dt

    @classmethod
    def report(cls):
        return {k: round(v, 4) for k, v in sorted(cls.acc.items())}

from ..data import SplitDataset, BatchDataset, make_data_loader
from ..metrics import Metric
from ..models import make_model
from ..utils import collate, to_device
from .federation import Federation
from .sequential import SequentialClientTrainer


def sample_active_users(cfg, epoch=None, generator=None):
    """ceil(frac*num_users) clients by randperm
    (reference: src/train_classifier_fed.py:172-181).  With a generator the
    sampling is reproducible across ranks and GPU counts."""
    num_active = int(np.ceil(cfg['frac'] * cfg['num_users']))
    perm = torch.randperm(cfg['num_users'], generator=generator)
    return perm[:num_active].tolist()


class FedRunner:
    def __init__(self, cfg, dataset, data_split, label_split, model, optimizer,
                 logger=None, dist_ctx=None):
        self.cfg = cfg
        self.dataset = dataset
        self.data_split = data_split
        self.label_split = label_split
        self.global_model = model
        self.optimizer = optimizer
        self.logger = logger
        self.dist_ctx = dist_ctx  # parallel.DistContext or None
        self.federation = Federation(model.state_dict(), cfg['model_rate'],
                                     label_split, cfg)
        self.is_lm = cfg['model_name'] == 'transformer'
        use_batched = cfg.get('engine', 'sequential') == 'batched'
        # The grouped BBottleneck engine passed its GPU numerics suite
        # (GPUTEST_r01) so Bottleneck resnets now use the batched engine by
        # default; HETEROFL_BATCHED_BOTTLENECK=0 forces the sequential oracle
        if use_batched and cfg['model_name'] in ('resnet50', 'resnet101',
                                                 'resnet152') and \
                os.environ.get('HETEROFL_BATCHED_BOTTLENECK', '1') == '0':
            use_batched = False
        if use_batched and self.is_lm:
            from .batched_lm_trainer import BatchedLMClientTrainer
            self.trainer = BatchedLMClientTrainer(cfg)
            self.trainer.set_data(dataset, data_split)
        elif use_batched:
            from .batched import BatchedClientTrainer
            self.trainer = BatchedClientTrainer(cfg)
            self.trainer.set_data(dataset, data_split)
        else:
            self.trainer = SequentialClientTrainer(cfg)
        self._round_gen = None

    # ------------------------------------------------------------------ round
    def _round_generator(self, epoch):
        """Seeded per round so all ranks agree on sampling without
        communication (SURVEY §7 reproducibility contract)."""
        seed = int(self.cfg.get('round_seed_base', self.cfg.get('init_seed', 0)))
        g = torch.Generator()
        g.manual_seed((seed * 1000003 + epoch) % (2 ** 63 - 1))
        return g

    def _make_loader(self, user):
        cfg = self.cfg
        if self.is_lm:
            # LM clients own rows of the batchified token matrix
            # (reference: src/train_transformer_fed.py:158-162)
            return BatchDataset(SplitDataset(self.dataset['train'],
                                             self.data_split['train'][user]),
                                cfg['bptt'])
        loader = make_data_loader(
            {'train': SplitDataset(self.dataset['train'],
                                   self.data_split['train'][user])}, cfg)['train']
        return loader

    def train_round(self, epoch):
        cfg = self.cfg
        self.global_model.load_state_dict(self.federation.global_parameters)
        self.global_model.train(True)
        lr = self.optimizer.param_groups[0]['lr']

        g = self._round_generator(epoch)
        if cfg['world_size'] > 1 or self.dist_ctx is not None:
            user_idx = sample_active_users(cfg, epoch, generator=g)
            self.federation.make_model_rate(generator=g)
            resample = False
        else:
            user_idx = sample_active_users(cfg, epoch)
            resample = True
        # shard clients across ranks (identity shard when single rank)
        rank, world = (0, 1) if self.dist_ctx is None else \
            (self.dist_ctx.rank, self.dist_ctx.world_size)
        my_clients = list(range(rank, len(user_idx), world))
        with _phase_timer('1.distribute'):
            local_parameters, param_idx = self.federation.distribute(
                user_idx, resample=resample,
                slots=my_clients if world > 1 else None, round=epoch)

        with _phase_timer('2.local_train'):
            trained = dict(self.trainer.train_clients(
                my_clients, user_idx, local_parameters,
                self.federation.model_rate, self._make_loader,
                self.label_split, lr, self.logger))

        with _phase_timer('3.combine'):
            if self.dist_ctx is None:
                # combine averages whoever reported — a client that failed
                # mid-round simply contributes nothing (reference tolerance
                # semantics, src/fed.py:180-298)
                tmp_d, cnt_d = self.federation.accumulate(
                    trained, param_idx, user_idx,
                    slots=sorted(trained.keys()))
                self.federation.finalize(tmp_d, cnt_d)
            else:
                from ..parallel.dist import distributed_combine
                distributed_combine(self.federation, trained, param_idx,
                                    user_idx, self.dist_ctx)
        self.global_model.load_state_dict(self.federation.global_parameters)
        if self.logger is not None:
            # per-round console line (the engine-level equivalent of the
            # reference's per-batch Train Epoch/ETA prints,
            # src/train_classifier_fed.py:108-119 — the graphed inner loop
            # has no per-batch host involvement to log from)
            if self.dist_ctx is not None:
                self.logger.sync()  # merge each rank's clients' train metrics
            total = cfg['num_epochs']['global'] if \
                isinstance(cfg['num_epochs'], dict) else cfg['num_epochs']
            info = {'info': ['Model: {}'.format(cfg.get('model_tag', '')),
                             'Train Epoch: {}({:.0f}%)'.format(
                                 epoch, 100.0 * epoch / max(total, 1)),
                             'Learning rate: {:.4g}'.format(lr)]}
            self.logger.append(info, 'train', mean=False)
            if self.dist_ctx is None or self.dist_ctx.is_main:
                flat = [m for group in cfg['metric_name']['train'].values()
                        for m in group]
                self.logger.write('train', flat)
        return user_idx

    # ------------------------------------------------------------------ stats
    def stats(self):
        """sBN statistics pass: rebuild the global model with tracked running
        stats and run the full train set in train mode under no_grad
        (reference: src/train_classifier_fed.py:127-138).

        Multi-rank (C2 of SURVEY §2b): the train set is sharded across ranks
        and the cumulative running stats are combined by a batch-count
        weighted all-reduce over RCCL — momentum=None BN keeps the running
        stats as the mean over batches, so the weighted mean over ranks
        reproduces the sequential pass (equal-size batches)."""
        return self._stats_model(self.cfg['global_model_rate'], None)

    def _stats_model(self, rate, params):
        """The statistics pass at one width level.  params=None is the
        global model at the global rate (stats()); otherwise `params` is the
        global model sliced for `rate` (Federation.slice_for_rate) and the
        slice is treated as a full model of its own: the tracked model is
        built with global_model_rate = rate, so its Scaler rate is 1 and the
        statistics come from the unscaled activations."""
        cfg = self.cfg
        if self.is_lm:
            return self.global_model  # LM path has no sBN pass (reference:
            # src/train_transformer_fed.py:77)
        with torch.no_grad():
            if params is None:
                test_model = make_model(
                    cfg, model_rate=cfg['global_model_rate'],
                    track=True).to(cfg['device'])
                test_model.load_state_dict(self.global_model.state_dict(),
                                           strict=False)
            else:
                test_model = make_model(
                    dict(cfg, global_model_rate=rate), model_rate=rate,
                    track=True).to(cfg['device'])
                test_model.load_state_dict(params, strict=False)
            if self._native_stats_ok():
                self._native_stats(test_model, rate, params)
                return test_model
            test_model.train(True)
            # BN momentum=None is a cumulative average over batches, which is
            # batch-size invariant for equal-size batches — so the stats pass
            # can use large batches on GPU instead of the train batch of 10
            # (5000 launches -> ~100 per round)
            scfg = dict(cfg)
            scfg['shuffle'] = dict(cfg['shuffle'])
            scfg['shuffle']['train'] = False  # stats don't need a shuffle;
            # unshuffled batches make the pass deterministic and identical
            # across GPU counts
            if torch.cuda.is_available():
                scfg['batch_size'] = dict(cfg['batch_size'])
                scfg['batch_size']['train'] = 500
            train = self.dataset['train']
            n_batches = 0
            if self.dist_ctx is not None and self.dist_ctx.world_size > 1:
                rank, world = self.dist_ctx.rank, self.dist_ctx.world_size
                bs = scfg['batch_size']['train']
                # shard whole batches (incl. the partial tail batch) across
                # ranks: cumulative-BN (momentum=None) weighs every batch
                # equally, so giving the tail to exactly one rank and
                # weighting ranks by batch count reproduces the single-rank
                # pass exactly — tail included
                total_b = (len(train) + bs - 1) // bs
                my_b = list(range(rank, total_b, world))
                idx = [i for b in my_b
                       for i in range(b * bs, min((b + 1) * bs, len(train)))]
                train = SplitDataset(train, idx)
            loader = make_data_loader({'train': train}, scfg)['train']
            for input in loader:
                input = collate(input)
                input = to_device(input, cfg['device'])
                test_model(input)
                n_batches += 1
            if self.dist_ctx is not None and self.dist_ctx.world_size > 1:
                import torch.distributed as dist
                bufs = []
                for mod in test_model.modules():
                    if hasattr(mod, 'running_mean') and                             mod.running_mean is not None:
                        bufs.append(mod.running_mean)
                        bufs.append(mod.running_var)
                if bufs:
                    w = float(n_batches)
                    flat = torch.cat([b.reshape(-1).float() * w
                                      for b in bufs])
                    cnt = torch.tensor([w], device=flat.device)
                    dist.all_reduce(flat)
                    dist.all_reduce(cnt)
                    flat /= cnt
                    off = 0
                    for b in bufs:
                        n = b.numel()
                        b.copy_(flat[off:off + n].view_as(b))
                        off += n
        return test_model

    # ------------------------------------------------------ native sBN pass
    def _native_stats_ok(self):
        """Route the sBN statistics pass through the batched native engine
        (MFMA convs + fused sBN kernels) instead of the eager per-client
        model.  bn only (other norms track no running stats) and vision only;
        HETEROFL_NATIVE_STATS=0 forces the eager pass."""
        from .batched import BatchedClientTrainer
        return (self.cfg['norm'] == 'bn' and not self.is_lm
                and isinstance(self.trainer, BatchedClientTrainer)
                and os.environ.get('HETEROFL_NATIVE_STATS', '1') == '1')

    def _native_stats(self, test_model, rate=None, params=None):
        """Run the full train set (normalized, augmented, unshuffled,
        batch 500 on GPU) through a 1-group batched model at `rate` (default:
        the global rate) holding `params` (default: the global parameters)
        and harvest each fused BN kernel's per-batch mean/var into the
        cumulative (momentum=None) running stats of test_model
        (reference semantics: src/train_classifier_fed.py:127-138 with
        BatchNorm2d(momentum=None), src/models/resnet.py:16-17).

        Multi-rank: whole batches (incl. the partial tail) shard across
        ranks; per-module stats merge with a batch-count-weighted
        all-reduce (C2)."""
        from .batched import pack_states, BNormReLU
        cfg = self.cfg
        device = torch.device(cfg['device'])
        trainer = self.trainer
        if params is None:
            bmodel = trainer._batched_model(cfg['global_model_rate'], 1)
            pack_states(bmodel, [dict(self.federation.global_parameters)])
        else:
            # a width level is its own full model: Scaler rate 1
            bmodel = trainer._batched_model(rate, 1, scaler_rate=1.0)
            pack_states(bmodel, [dict(params)])
        bmodel.train(True)

        state = {}  # module -> [mean, unbiased_var, n_batches]

        def sink(mod, mean, invstd, x):
            n, _, h, w = x.shape
            m = n * h * w
            mu = mean.float()
            biased = invstd.float().pow(-2) - 1e-5
            unb = biased * (m / max(m - 1, 1))
            s = state.get(mod)
            if s is None:
                state[mod] = [mu.clone(), unb.clone(), 1]
            else:
                s[2] += 1
                k = s[2]
                s[0] += (mu - s[0]) / k
                s[1] += (unb - s[1]) / k

        bn_mods = [(name, m) for name, m in bmodel.named_modules()
                   if isinstance(m, BNormReLU) and m.norm == 'bn']
        for _, m in bn_mods:
            m.stats_sink = sink
        try:
            train = self.dataset['train']
            img = getattr(self, '_stats_img', None)
            if img is None:
                img = train.img
                if img.dim() == 3:
                    img = img.unsqueeze(-1)
                img = img.to(device)
                self._stats_img = img
            n_total = img.size(0)
            # cumulative BN is batch-size invariant for equal-size batches,
            # so the GPU pass uses large batches (fewer launches, fuller
            # kernels); HETEROFL_STATS_BS tunes it
            bs = int(os.environ.get('HETEROFL_STATS_BS', '2500')) \
                if device.type == 'cuda' else cfg['batch_size']['train']
            total_b = (n_total + bs - 1) // bs
            rank, world = (0, 1) if self.dist_ctx is None else \
                (self.dist_ctx.rank, self.dist_ctx.world_size)
            # the reference's stats pass iterates the TRAIN loader, i.e.
            # with train-time augmentation active (train_classifier_fed.py:
            # 127-138 over the train dataset's transforms).  Activations run
            # in the engine's compute dtype: fp32 MFMA is 1/16 the bf16 rate,
            # and the model trains in bf16 anyway (BN statistics accumulate
            # in fp32 inside the kernel either way).
            amp = getattr(trainer, '_amp', False)
            for b in range(rank, total_b, world):
                batch = img[b * bs:min((b + 1) * bs, n_total)]
                x = trainer.augment(batch, train=True)
                if amp:
                    x = x.to(torch.bfloat16)
                bmodel(x)
        finally:
            for _, m in bn_mods:
                m.stats_sink = None
        if self.dist_ctx is not None and self.dist_ctx.world_size > 1:
            import torch.distributed as dist
            parts, weights = [], []
            for _, m in bn_mods:
                if m not in state:  # rank had zero batches (tiny dataset)
                    z = torch.zeros(m.weight.numel(), device=device)
                    state[m] = [z, z.clone(), 0]
                mu, var, k = state[m]
                parts.append(mu * k)
                parts.append(var * k)
                weights.append(float(k))
            flat = torch.cat([p.reshape(-1) for p in parts])
            wt = torch.tensor(weights, dtype=torch.float32, device=flat.device)
            dist.all_reduce(flat)
            dist.all_reduce(wt)
            off = 0
            for i, (_, m) in enumerate(bn_mods):
                mu, var, k = state[m]
                n = mu.numel()
                state[m] = [flat[off:off + n] / wt[i].clamp(min=1),
                            flat[off + n:off + 2 * n] / wt[i].clamp(min=1),
                            int(wt[i].item())]
                off += 2 * n
        named = dict(test_model.named_modules())
        for name, m in bn_mods:
            mu, var, k = state[m]
            tgt = named[name]
            tgt.running_mean.copy_(mu.to(tgt.running_mean.dtype))
            tgt.running_var.copy_(var.to(tgt.running_var.dtype))
            if tgt.num_batches_tracked is not None:
                tgt.num_batches_tracked.fill_(k)
        test_model.train(False)

    # ------------------------------------------- per-width-level evaluation
    def _stage_eval(self):
        """Raw uint8 test set, labels and the device-side normalizer, staged
        on the run's device once."""
        from .batched import DeviceAugment
        staged = getattr(self, '_eval_staged', None)
        if staged is None:
            ds = self.dataset['test']
            device = torch.device(self.cfg['device'])
            img = ds.img
            if img.dim() == 3:
                img = img.unsqueeze(-1)
            aug = DeviceAugment(self.cfg['data_name'], device)
            labels = torch.tensor(ds.target, device=device)
            staged = (img.to(device), labels, aug)
            self._eval_staged = staged
        return staged

    def _native_eval_sums(self, test_model):
        """(local (U, 3), global (3,)) rows of (loss sum, correct, count) for
        a tracked model: NativeInference logits over the whole test set, then
        ops.fused.eval_metrics over the users' CSR shards."""
        from ..ops.fused import eval_metrics
        from .infer import NativeInference, batched_logits, user_csr
        cfg = self.cfg
        img, labels, aug = self._stage_eval()
        csr = getattr(self, '_eval_csr', None)
        if csr is None:
            csr = user_csr(self.data_split['test'], self.label_split,
                           cfg['num_users'], cfg['classes_size'],
                           cfg['mask'], img.device)
            self._eval_csr = csr
        scores = batched_logits(NativeInference(test_model), img, aug)
        return eval_metrics(scores, labels, *csr)

    @staticmethod
    def _sums_to_metrics(row, flavor, names, suffix=''):
        """(loss sum, correct, count) -> {'<flavor>-Loss', '<flavor>-Accuracy'}
        restricted to `names`; None for an empty row."""
        loss, correct, count = row
        if count == 0:
            return None
        full = {flavor + '-Loss': loss / count,
                flavor + '-Accuracy': 100.0 * correct / count}
        return {k + suffix: v for k, v in full.items() if k in names}

    def test_levels(self, epoch):
        """Evaluate every width level a client may deploy: for each distinct
        rate in cfg['model_rate'], slice the global parameters, run an sBN
        statistics pass at that width (the slice is its own full model:
        Scaler rate 1), and evaluate the tracked slice with the native
        inference engine.  Returns {rate: {'Global-Loss', 'Global-Accuracy',
        'Local-Loss', 'Local-Accuracy'}} and logs each metric under
        'test/<name>@<rate>'; the tracked per-level models stay available in
        self.level_models.  Vision models only.  Multi-rank: every rank
        computes the identical result redundantly; rank 0 writes.

        Under cfg['submodel'] = 'roll' the slices are the windows of round
        `epoch`: the levels are evaluated as the clients of the round just
        trained received them."""
        from .. import ops as native_ops
        if self.is_lm:
            raise NotImplementedError(
                'test_levels covers the vision models; the transformer has '
                'no sBN pass and a separate evaluation path')
        cfg = self.cfg
        all_names = ['Local-Loss', 'Local-Accuracy', 'Global-Loss',
                     'Global-Accuracy']
        out = {}
        self.level_models = {}
        with torch.no_grad():
            for rate in sorted(set(cfg['model_rate']), reverse=True):
                params = self.federation.slice_for_rate(rate, round=epoch)
                prev = native_ops.set_large_conv(True)
                try:
                    test_model = self._stats_model(rate, params)
                finally:
                    native_ops.set_large_conv(prev)
                test_model.train(False)
                self.level_models[rate] = test_model
                local, glob = self._native_eval_sums(test_model)
                lsum = local.sum(0).tolist()
                glob = glob.tolist()
                suffix = '@{}'.format(rate)
                res = {}
                for row, flavor in ((glob, 'Global'), (lsum, 'Local')):
                    ev = self._sums_to_metrics(row, flavor, all_names)
                    if ev is None:
                        continue
                    res.update(ev)
                    if self.logger:
                        self.logger.append(
                            {k + suffix: v for k, v in ev.items()}, 'test',
                            int(row[2]))
                out[rate] = res
        if self.logger and (self.dist_ctx is None or self.dist_ctx.is_main):
            info = {'info': ['Test Epoch: {}({:.0f}%)'.format(epoch, 100.)]}
            self.logger.append(info, 'test', mean=False)
            self.logger.write('test', [n + '@{}'.format(r) for r in out
                                       for n in all_names])
        return out

    # --------------------------------------------------- native LM evaluation
    def _stage_lm_eval(self):
        """The batchified test token matrix (rows, T) on the run's device,
        staged once, and the (start, length) of every BatchDataset(test,
        bptt) window: full windows plus one shorter tail."""
        staged = getattr(self, '_lm_eval_staged', None)
        if staged is None:
            tokens = self.dataset['test'][:]['label'].to(self.cfg['device'])
            T, bptt = tokens.size(1), self.cfg['bptt']
            windows = [(s, min(bptt, T - s)) for s in range(0, T, bptt)]
            staged = (tokens.contiguous(), windows)
            self._lm_eval_staged = staged
        return staged

    def _lm_masked_src(self, tokens):
        """One Bernoulli(mask_rate) draw over the whole (rows, T) matrix from
        the global torch RNG; masked positions read the <mask> id."""
        mask = torch.bernoulli(torch.full(
            tuple(tokens.shape), self.cfg['mask_rate'], device=tokens.device))
        return tokens.masked_fill(mask == 1, self.cfg['num_tokens'])

    @staticmethod
    def _lm_topk():
        """HETEROFL_LM_TOPK: 0 / unset is off, 1..8 asks the LM evaluation
        for top-1 / top-k token accuracy next to loss and perplexity."""
        raw = os.environ.get('HETEROFL_LM_TOPK', '0')
        try:
            k = int(raw)
        except ValueError:
            k = -1
        if not 0 <= k <= 8:
            raise ValueError('HETEROFL_LM_TOPK must be an integer in 0..8, '
                             'got {!r}'.format(raw))
        return k

    def _lm_window_metrics(self, model, src, which, topk=0):
        """[(loss_w, ppl_w)] for the windows `which`: loss_w is the mean NLL
        over the window's rows x S_w tokens and ppl_w = exp(loss_w), the
        reference's per-window Perplexity.  All full windows go through
        NativeLMInference as one batch of sequences, the tail as another.

        topk > 0: the NLL comes from window_topk (one vocabulary pass for
        loss and predictions) and every tuple gains a third entry, the
        window's integer counts {'n', 'hit1', 'hitk', 'mn', 'mhit1',
        'mhitk'}: positions, labels met by the first / by any of the topk
        predictions, and the same over the <mask> positions of src."""
        from .infer import NativeLMInference
        tokens, windows = self._stage_lm_eval()
        engine = NativeLMInference(model)
        rows, bptt = tokens.size(0), self.cfg['bptt']
        loss, counts = {}, {}

        def means(nll, groups):
            # one mean per window of the batch of full windows; the tail
            # (groups 0) is reduced as a whole
            if not groups:
                return [nll.double().mean().item()]
            return nll.view(groups, -1).double().mean(1).tolist()

        def run(s, y, groups):
            """Mean NLL and, with topk, the 6 counts of each of `groups`
            windows (0: the tail, one window)."""
            if not topk:
                return means(engine.window_nll(s, y), groups), None
            ids, _, nll = engine.window_topk(s, k=topk, label=y)
            hit = ids == y.unsqueeze(-1)
            hit1, hitk = hit[..., 0], hit.any(-1)
            masked = s == self.cfg['num_tokens']
            cnt = torch.stack([torch.ones_like(hit1), hit1, hitk, masked,
                               hit1 & masked, hitk & masked], -1)
            return means(nll, groups), \
                cnt.view(max(groups, 1), -1, 6).sum(1).tolist()

        full = [w for w in which if windows[w][1] == bptt]
        if full:
            idx = torch.tensor([windows[w][0] for w in full],
                               device=tokens.device).view(-1, 1) + \
                torch.arange(bptt, device=tokens.device).view(1, -1)
            # (windows, rows, bptt) -> one sequence per (window, row)
            mean, cnt = run(src[:, idx].permute(1, 0, 2).reshape(-1, bptt),
                            tokens[:, idx].permute(1, 0, 2)
                            .reshape(-1, bptt), len(full))
            loss.update(zip(full, mean))
            if topk:
                counts.update(zip(full, cnt))
        for w in which:
            if w not in loss:
                s, n = windows[w]
                mean, cnt = run(src[:, s:s + n].contiguous(),
                                tokens[:, s:s + n].contiguous(), 0)
                loss[w] = mean[0]
                if topk:
                    counts[w] = cnt[0]
        if not topk:
            return [(loss[w], math.exp(loss[w])) for w in which]
        keys = ('n', 'hit1', 'hitk', 'mn', 'mhit1', 'mhitk')
        return [(loss[w], math.exp(loss[w]), dict(zip(keys, counts[w])))
                for w in which]

    @staticmethod
    def _lm_accuracy_names(topk):
        """(all-position names, masked-position names) under the knob."""
        tail = ['-Top{}'.format(topk)] if topk > 1 else []
        return (['Global-Accuracy' + t for t in [''] + tail],
                ['Global-Masked-Accuracy' + t for t in [''] + tail])

    def _lm_log_accuracy(self, logger, cnt, topk, rows, suffix=''):
        """Log one window's accuracies (percent): over all positions with
        weight `rows`, like the loss; over the <mask> positions with weight
        their number, which pools them over the evaluation."""
        names, mnames = self._lm_accuracy_names(topk)
        hits = (cnt['hit1'], cnt['hitk'])
        logger.append({n + suffix: 100.0 * h / cnt['n']
                       for n, h in zip(names, hits)}, 'test', rows)
        if cnt['mn']:
            mhits = (cnt['mhit1'], cnt['mhitk'])
            logger.append({n + suffix: 100.0 * h / cnt['mn']
                           for n, h in zip(mnames, mhits)}, 'test', cnt['mn'])

    def _native_lm_test(self, test_model, logger, cfg, rank, world):
        """LM evaluation under HETEROFL_NATIVE_LM_EVAL=1: this rank's windows
        (r, r + world, ...) through NativeLMInference, logged per window with
        weight rows exactly as the eager loop logs them.  HETEROFL_LM_TOPK=k
        adds Global-Accuracy[-Top{k}] and Global-Masked-Accuracy[-Top{k}]
        (see test_lm_levels).

        The mask is drawn once per evaluation over the whole token matrix;
        the eager loop draws one per window, so under mask_rate > 0 the two
        paths see different (equally distributed) masks and agree only
        statistically.  With mask_rate == 0 they agree exactly."""
        tokens, windows = self._stage_lm_eval()
        src = self._lm_masked_src(tokens)
        topk = self._lm_topk()
        names = cfg['metric_name']['test']['Global']
        which = list(range(rank, len(windows), world))
        for res in self._lm_window_metrics(test_model, src, which, topk):
            ev = {'Global-Loss': res[0], 'Global-Perplexity': res[1]}
            if logger:
                logger.append({k: v for k, v in ev.items() if k in names},
                              'test', tokens.size(0))
                if topk:
                    self._lm_log_accuracy(logger, res[2], topk,
                                          tokens.size(0))

    def test_lm_levels(self, epoch):
        """Masked-LM counterpart of test_levels: for each distinct rate in
        cfg['model_rate'], descending, slice the global parameters, load the
        slice into a full model of its own (Scaler rate 1) and evaluate it
        with NativeLMInference.  One mask, drawn once from the global torch
        RNG, is shared by every level, so the levels are comparable.
        Returns {rate: {'Global-Loss', 'Global-Perplexity'}}: the means over
        the windows of the per-window loss and exp(loss), every window
        weighing `rows`.  Each metric is logged under 'test/<name>@<rate>';
        the per-level models stay in self.level_models.  Multi-rank: every
        rank computes the identical result redundantly; rank 0 writes.

        Under cfg['submodel'] = 'roll' the slices are the windows of round
        `epoch`: the levels are evaluated as the clients of the round just
        trained received them.

        HETEROFL_LM_TOPK=k (1..8) adds token accuracy in percent, from the
        same vocabulary pass as the loss: 'Global-Accuracy' and, for k > 1,
        'Global-Accuracy-Top{k}' (label among the first / the first k
        predictions, averaged over the windows like the loss), and
        'Global-Masked-Accuracy[-Top{k}]' (the same over the <mask>
        positions, pooled over the evaluation; left out when nothing is
        masked)."""
        if not self.is_lm:
            raise NotImplementedError(
                'test_lm_levels covers the transformer; use test_levels for '
                'the vision models')
        cfg = self.cfg
        topk = self._lm_topk()
        names, mnames = self._lm_accuracy_names(topk) if topk else ([], [])
        out = {}
        self.level_models = {}
        with torch.no_grad():
            tokens, windows = self._stage_lm_eval()
            src = self._lm_masked_src(tokens)
            which = list(range(len(windows)))
            for rate in sorted(set(cfg['model_rate']), reverse=True):
                params = self.federation.slice_for_rate(rate, round=epoch)
                model = make_model(dict(cfg, global_model_rate=rate),
                                   model_rate=rate).to(cfg['device'])
                model.load_state_dict(params)
                model.train(False)
                self.level_models[rate] = model
                res = self._lm_window_metrics(model, src, which, topk)
                suffix = '@{}'.format(rate)
                for r in res:
                    if self.logger:
                        self.logger.append(
                            {'Global-Loss' + suffix: r[0],
                             'Global-Perplexity' + suffix: r[1]}, 'test',
                            tokens.size(0))
                        if topk:
                            self._lm_log_accuracy(self.logger, r[2], topk,
                                                  tokens.size(0), suffix)
                out[rate] = {
                    'Global-Loss': sum(r[0] for r in res) / len(res),
                    'Global-Perplexity': sum(r[1] for r in res) / len(res)}
                if topk:
                    for n, h in zip(names, ('hit1', 'hitk')):
                        out[rate][n] = sum(100.0 * r[2][h] / r[2]['n']
                                           for r in res) / len(res)
                    mn = sum(r[2]['mn'] for r in res)
                    for n, h in zip(mnames, ('mhit1', 'mhitk')):
                        if mn:
                            out[rate][n] = \
                                100.0 * sum(r[2][h] for r in res) / mn
        if self.logger and (self.dist_ctx is None or self.dist_ctx.is_main):
            info = {'info': ['Test Epoch: {}({:.0f}%)'.format(epoch, 100.)]}
            self.logger.append(info, 'test', mean=False)
            self.logger.write('test', [n + '@{}'.format(r) for r in out
                                       for n in out[r]])
        return out

    # -------------------------------------------------------- fast GPU eval
    def _fast_vision_eval(self, test_model, metric, logger, cfg, rank, world):
        """Loader-free evaluation: stage the raw uint8 test set on device
        once, run ONE pass of large-batch forwards for the UNMASKED logits,
        then derive every user's Local (label-split-masked, reference:
        src/models/resnet.py:152-157) and the Global metrics from those
        logits.  Same math as the per-user loader loop (the mask only
        rewrites logits), ~100x fewer host round-trips.  Users and samples
        shard across ranks exactly like the loader path."""
        from ..models.functional import masked_cross_entropy
        from .batched import DeviceAugment
        import torch.nn.functional as F
        device = torch.device(cfg['device'])
        img, labels, aug = self._stage_eval()
        n = img.size(0)
        if os.environ.get('HETEROFL_NATIVE_EVAL', '0') == '1':
            # native evaluator: hand-written inference kernels for the
            # logits, one eval_metrics launch pair instead of the per-user
            # loop.  Every rank holds all sums; it logs its share of users
            # (and rank 0 the Global row) so logger.sync() merges as usual.
            local, glob = self._native_eval_sums(test_model)
            names = cfg['metric_name']['test']
            local, glob = local.tolist(), glob.tolist()
            for m in range(rank, cfg['num_users'], world):
                ev = self._sums_to_metrics(local[m], 'Local',
                                           names.get('Local', []))
                if ev is not None and logger:
                    logger.append(ev, 'test', int(local[m][2]))
            if rank == 0:
                ev = self._sums_to_metrics(glob, 'Global',
                                           names.get('Global', []))
                if ev is not None and logger:
                    logger.append(ev, 'test', int(glob[2]))
            return
        bs = 2048
        scores = []
        for b0 in range(0, n, bs):
            x = aug(img[b0:b0 + bs], train=False)
            out = test_model({'img': x, 'label': labels[b0:b0 + bs]})
            scores.append(out['score'].float())
        scores = torch.cat(scores)
        names = cfg['metric_name']['test']
        # Local metrics: this rank's share of users
        for m in range(rank, cfg['num_users'], world):
            idx = torch.as_tensor(self.data_split['test'][m],
                                  dtype=torch.long, device=device)
            if idx.numel() == 0:
                continue
            y = labels[idx]
            ls = torch.tensor(self.label_split[m], device=device)
            sc = scores[idx]
            if cfg['mask']:
                sc, loss = masked_cross_entropy(sc, y, ls,
                                                cfg['classes_size'])
            else:
                loss = F.cross_entropy(sc, y)
            ev = metric.evaluate(names['Local'],
                                 {'label': y, 'label_split': ls},
                                 {'score': sc, 'loss': loss})
            if logger:
                logger.append(ev, 'test', idx.numel())
        # Global metrics: this rank's share of samples, unmasked logits
        gidx = torch.arange(rank, n, world, device=device)
        gy = labels[gidx]
        gs = scores[gidx]
        ev = metric.evaluate(names['Global'], {'label': gy},
                             {'score': gs,
                              'loss': F.cross_entropy(gs, gy)})
        if logger:
            logger.append(ev, 'test', gidx.numel())

    # ------------------------------------------------------------------- test
    def test(self, test_model, epoch):
        """Per-client Local metrics + Global metrics
        (reference: src/train_classifier_fed.py:141-169).  On GPU the eval
        batch is enlarged (metric means are batch-size invariant under the
        logger's count weighting) so evaluation is not launch-bound.

        Multi-rank (C3 of SURVEY §2b): the per-user Local loop is sharded by
        user and the Global set by sample across ranks; logger.sync() then
        merges the shards' weighted sums so every rank sees the sequential
        run's exact means (weighted means are additive over disjoint
        shards).

        The transformer is evaluated by the eager per-window loop, or under
        HETEROFL_NATIVE_LM_EVAL=1 by NativeLMInference (_native_lm_test,
        which also documents how its token mask differs)."""
        cfg = self.cfg
        if torch.cuda.is_available() and not self.is_lm:
            cfg = dict(cfg)
            cfg['batch_size'] = dict(cfg['batch_size'])
            cfg['batch_size']['test'] = max(cfg['batch_size']['test'], 500)
        rank, world = (0, 1) if self.dist_ctx is None else \
            (self.dist_ctx.rank, self.dist_ctx.world_size)
        metric = Metric()
        logger = self.logger
        with torch.no_grad():
            test_model.train(False)
            if not self.is_lm and torch.cuda.is_available() and \
                    os.environ.get('HETEROFL_FAST_EVAL', '1') == '1' and \
                    hasattr(self.dataset['test'], 'img'):
                self._fast_vision_eval(test_model, metric, logger, cfg,
                                       rank, world)
            elif not self.is_lm:
                for m in range(rank, cfg['num_users'], world):
                    loader = make_data_loader(
                        {'test': SplitDataset(self.dataset['test'],
                                              self.data_split['test'][m])}, cfg)['test']
                    for input in loader:
                        input = collate(input)
                        input_size = input['label'].size(0)
                        input['label_split'] = torch.tensor(self.label_split[m])
                        input = to_device(input, cfg['device'])
                        output = test_model(input)
                        ev = metric.evaluate(cfg['metric_name']['test']['Local'],
                                             input, output)
                        if logger:
                            logger.append(ev, 'test', input_size)
                global_test = self.dataset['test']
                if world > 1:
                    global_test = SplitDataset(
                        global_test, list(range(rank, len(global_test), world)))
                loader = make_data_loader({'test': global_test}, cfg)['test']
                for input in loader:
                    input = collate(input)
                    input_size = input['label'].size(0)
                    input = to_device(input, cfg['device'])
                    output = test_model(input)
                    ev = metric.evaluate(cfg['metric_name']['test']['Global'],
                                         input, output)
                    if logger:
                        logger.append(ev, 'test', input_size)
            elif os.environ.get('HETEROFL_NATIVE_LM_EVAL', '0') == '1':
                self._native_lm_test(test_model, logger, cfg, rank, world)
            else:
                ds = BatchDataset(self.dataset['test'], cfg['bptt'])
                for i in range(rank, len(ds), world):
                    input = ds[i]
                    input_size = input['label'].size(0)
                    input = to_device(input, cfg['device'])
                    output = test_model(input)
                    ev = metric.evaluate(cfg['metric_name']['test']['Global'],
                                         input, output)
                    if logger:
                        logger.append(ev, 'test', input_size)
            if logger:
                if self.dist_ctx is not None:
                    logger.sync()
                info = {'info': ['Test Epoch: {}({:.0f}%)'.format(epoch, 100.)]}
                logger.append(info, 'test', mean=False)
                if self.dist_ctx is None or self.dist_ctx.is_main:
                    names = cfg['metric_name']['test']
                    flat = sum(names.values(), []) if isinstance(names, dict) \
                        else names
                    logger.write('test', flat)
