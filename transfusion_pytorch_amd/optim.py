"""Fused optimizer + data-parallel gradient exchange for the flat parameter buffer.

`train_toy.py:52-57` does loss.backward(); clip_grad_norm_(0.5); Adam.step(); zero_grad().  Here the whole
model is ONE flat fp32 buffer, so the step is: [one RCCL all-reduce over xGMI] -> one sum-of-squares
reduction -> one fused clip+Adam kernel.  No host sync: the clip coefficient is computed on the device.
"""
from __future__ import annotations

import contextlib
import os
import struct

import torch
import torch.distributed as dist

from . import capi


class GradReducer:
    """Overlap of the data-parallel gradient exchange with the backward (reference practice: DDP's bucketed all-reduce under `accelerate`,
    train_mnist.py:114-126).  The flat gradient buffer completes BACK TO FRONT during the hand-written backward - the heads first, then the
    layers from the last to the first (their AdaLN conditioning weights included: engine.Plan forms those per layer), the embeddings last -
    so the buffer is exchanged in `groups` layer groups: as soon as a group's gradients are final (`Plan.bwd_cuts`), its two contiguous
    ranges (AdaLN weights, the layers' own parameters) go out as ONE asynchronous collective launch on the collective's stream while the
    backward of the earlier layers runs; what is left (AdaLN biases, time conditioning, the AttentionResidual parameters, embeddings, input /
    output projections) follows the backward as one more launch: groups + 1 collectives per step (5 by default).
    Every element is reduced exactly once (tests/test_dp_gloo.py).  One process per GPU, RCCL over xGMI via torch.distributed."""

    def __init__(self, model, process_group=None, groups: int = 4, exchange_dtype=None):
        self.model, self.group = model, process_group
        self.exchange_dtype = exchange_dtype         # torch.bfloat16: the ranges travel as bf16 (half the xGMI bytes), summed in bf16, written back to the fp32 buffer
        ps, md = model.store, model.md
        self.groups = max(1, min(groups, md.depth))
        self.per = -(-md.depth // self.groups)
        self.handles, self.done, self.staged = [], [], []
        self._step = -1
        d, D = md.dim, md.depth
        off = lambda name: ps.offsets[name][0]
        end = lambda name: ps.offsets[name][0] + int(torch.Size(ps.offsets[name][1]).numel())
        self._w0, self._b0 = off('transformer.layers.0.1.to_film.weight'), off('transformer.layers.0.1.to_film.bias')
        self._wl, self._bl = 2 * 3 * d * 4 * d, 2 * 3 * d                     # AdaLN weight / bias elements per layer (contiguous, layer-major)
        first = lambda i: off(f'transformer.layers.{i}.0.weight') if md.has_skip(i) else off(f'transformer.layers.{i}.1.fn.to_qk.0.weight')
        self._core = [first(i) for i in range(D)] + [off('transformer.norm.gamma')]
        self._head = (off('transformer.norm.gamma'), ps.numel)               # final norm, in / out projections, embeddings, logits
        self._mid = (end(f'transformer.layers.{D - 1}.2.to_ada_ln_zero.bias'), self._core[0])     # time conditioning MLP

    def ranges(self, lo: int, hi: int):
        """flat [start, end) ranges of the gradients of layers lo..hi (inclusive) that go out with the group: the layers' AdaLN conditioning
        weights and their own parameters.  (Their AdaLN biases - 6 d floats per layer, adjacent to the time-conditioning MLP - travel with the tail.)"""
        return [(self._w0 + lo * self._wl, self._w0 + (hi + 1) * self._wl), (self._core[lo], self._core[hi + 1])]

    def _reduce(self, ranges, async_op):
        """ONE collective launch for all `ranges`: fp32 in place through torch.distributed's coalescing manager (RCCL: one grouped launch, no
        staging copy; gloo: allreduce_coalesced), or - `exchange_dtype` - one all-reduce of a staged reduced-precision copy of the ranges"""
        g = self.model.store.grad
        ranges = [(a, b) for a, b in ranges if b > a]
        if not ranges:
            return
        if self.exchange_dtype is not None:
            buf = torch.cat([g[a:b].to(self.exchange_dtype) for a, b in ranges])
            h = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
            if async_op:
                self.handles.append(h); self.staged.append((ranges, buf))
            else:
                self._unstage(ranges, buf)
        elif len(ranges) == 1:
            a, b = ranges[0]
            h = dist.all_reduce(g[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
            if async_op:
                self.handles.append(h)
        elif self._coalesce():
            with dist._coalescing_manager(group=self.group, async_ops=async_op) as cm:
                for a, b in ranges:
                    dist.all_reduce(g[a:b], op=dist.ReduceOp.SUM, group=self.group)
            if async_op:
                self.handles.append(cm)
        else:
            # public API only: one all-reduce per range (two collective launches per layer group instead of one).  THE DEFAULT until a real
            # multi-rank RCCL run has validated the private `_coalescing_manager` path (TFX_DP_COALESCE=1 selects it)
            for a, b in ranges:
                h = dist.all_reduce(g[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
                if async_op:
                    self.handles.append(h)
            self.launches += len(ranges) - 1
        self.done += ranges
        self.launches += 1

    @staticmethod
    def _coalesce() -> bool:
        return os.environ.get('TFX_DP_COALESCE', '0') == '1' and hasattr(dist, '_coalescing_manager')

    def _unstage(self, ranges, buf):
        g, off = self.model.store.grad, 0
        for a, b in ranges:
            g[a:b].copy_(buf[off:off + b - a]); off += b - a

    launches = 0             # collective launches of the current step (<= groups + 1)

    def begin(self):
        self.handles, self.done, self.staged = [], [], []
        self.exchanged = False
        self.last_launches, self.launches = self.launches, 0

    last_launches = 0        # collective launches of the previous (finished) step

    exchanged = False        # a backward has sent layer groups out and no optimizer step has consumed them yet
    defer = False            # inside `FusedAdam.no_sync()`: this backward only accumulates (no cut, no collective) - a later one exchanges

    def group_ready(self, lo: int, hi: int):
        """called between two segments of the backward list: layers lo..hi are final (and, at the first cut, nothing else is)"""
        self._reduce(self.ranges(lo, hi), async_op=True)
        self.exchanged = True

    def check_fresh(self):
        """one backward per optimizer step (like DDP without `no_sync`): a second backward would accumulate into ranges that are already summed
        over the ranks (counting the first micro-batch `world` times) and race with the collectives in flight"""
        if self.exchanged:
            raise RuntimeError('overlap_grad_sync: a second backward() before optimizer.step() after the layer groups went out - run the micro-batches '
                               'that only accumulate under `with opt.no_sync():` (the LAST backward of the step, outside it, exchanges the sums)')

    def finish(self):
        """after the backward: exchange whatever no cut covered, then make the current stream wait for every collective"""
        n = self.model.store.numel
        covered = sorted(self.done)
        rest, pos = [], 0
        for a, b in covered:
            if a > pos:
                rest.append((pos, a))
            pos = max(pos, b)
        if pos < n:
            rest.append((pos, n))
        self._reduce(rest, async_op=False)
        for h in self.handles:
            h.wait()
        self.handles = []
        for ranges, buf in self.staged:               # reduced-precision ranges come back into the fp32 buffer
            self._unstage(ranges, buf)
        self.staged = []
        assert sum(b - a for a, b in self.done) == n, 'every gradient element must be reduced exactly once'


_ADAM_KEYS = ('lr', 'betas', 'eps', 'weight_decay', 'decoupled_weight_decay')
_ATAN2_KEYS = ('lr', 'betas', 'weight_decay', 'decoupled_weight_decay')          # the Adam-atan2 rule has no eps; its a, b are optimizer-wide


def _group_alias(key, index=0, doc=None):
    """attribute that reads and writes `param_groups[index][key]` (the scalars live in the groups, where schedulers and checkpoints look)"""
    def get(self):
        return self.param_groups[index][key]

    def put(self, value):
        self.param_groups[index][key] = value
    return property(get, put, doc=doc)


def decay_groups(model, weight_decay, decoupled=True):
    """the usual two parameter groups of `model.parameters()`: matrices and tables (`ndim >= 2`) decay; gains, biases, `layerscale` and
    `pseudo_queries` do not.  For `FusedAdam(model, param_groups=decay_groups(model, 0.1))` / `FusedMuon(...)`; every parameter is named, the
    first group is the decaying one."""
    names = {id(p): n for n, p in model.named_parameters()}
    plain = lambda p: p.ndim < 2 or names.get(id(p), '').endswith(('layerscale', 'pseudo_queries', 'gamma', 'bias'))
    params = list(model.parameters())
    return [dict(params=[p for p in params if not plain(p)], weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled)),
            dict(params=[p for p in params if plain(p)], weight_decay=0., decoupled_weight_decay=bool(decoupled))]


class FusedAdam(torch.optim.Optimizer):
    """global-norm clip + Adam over the flat fp32 buffer as one launch (train_toy.py:55-57), the data-parallel gradient exchange in front of it, a stock
    Adam under the same clip coefficient for `model.external_parameters()`.

    A `torch.optim.Optimizer`: `torch.optim.lr_scheduler.*` and optimizer wrappers take it, `state_dict()` / `load_state_dict()` have torch's format
    (interchangeable with `torch.optim.Adam(model.parameters())` / `AdamW`).  It owns `model.parameters()` in that order - the views into the flat
    buffer, the external parameters, for a SelfMaskedRepTraining wrapper the head's; parameters of the model that are neither (frozen ones, the
    user's modality encoders / decoders) are listed, never stepped and carry no state.

    `param_groups`: dicts `{'params': [parameters or their names], 'lr'?, 'betas'?, 'eps'?, 'weight_decay'?, 'decoupled_weight_decay'?}` (at most
    TFX_ADAM_MAX_GROUPS); parameters no group names belong to `param_groups[0]`.  `opt.param_groups` is live: every scalar is re-read at each step;
    `lr`, `betas`, `eps`, `weight_decay` are `param_groups[0]`'s.  `decoupled_weight_decay`: torch.optim.AdamW's rule (p *= 1 - lr wd) instead of the
    L2 form (g += wd p).  One group with the L2 form is the launch FusedAdam always made (`tfx_adam_step`); anything else goes through
    `tfx_adam_step_groups` with `group_ranges()` as a device table: one launch either way, one step count, one clip coefficient over everything.

    Frozen parameters (`p.requires_grad_(False)` on views into the flat buffer; groups may hold them, a group of only frozen parameters is legal): their
    element ranges (`frozen_ranges()`) join whatever another rule owns in the launch's `skip` table, re-read at every step - value, moments and weight
    decay leave them alone bit for bit; their gradient segments are zero (engine), so the clip norm is `clip_grad_norm_`'s over the trainable parameters.

    `deterministic_norm` (class default False, True in FusedMuon; may be set on an instance): take the clip norm as a fixed-order sum (`tfx_sumsq_det`)
    instead of `tfx_sumsq`'s atomic one, whose last bits - and with them the clip coefficient of every element - change from run to run.  False is the
    step FusedAdam always took."""

    deterministic_norm = False
    _GROUP_KEYS = _ADAM_KEYS          # what a parameter group of this rule carries
    _RULE_LAUNCH = 'tfx_adam_step_groups', 'tfx_adam_group_args'      # the rule's entry point over the flat buffer and its args struct
    _rule_fields = lambda self: {}    # hook: the by-value fields that struct has behind tfx_adam_group_args', checked
    lr, betas, eps, weight_decay = (_group_alias(k) for k in _ADAM_KEYS[:4])

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0., max_grad_norm=None, process_group=None,
                 average_grads=True, *, param_groups=None, decoupled_weight_decay=False, _other_rule_params=()):
        # a SelfMaskedRepTraining wrapper: the student's flat buffer as for the bare model, the prediction head's parameters (PyTorch
        # parameters with autograd gradients) by the route of the external ones
        outer = model
        head_params = list(model.head_parameters()) if hasattr(model, 'head_parameters') else []
        if head_params:
            model = model.student
        self.model = model
        self.max_grad_norm = max_grad_norm
        self.group = process_group
        self.average = average_grads
        self.step_count = 0
        self.always_sync = False        # run the collective even at world size 1 (exercises the RCCL path on a 1-GPU box)
        self.time_exchange = False      # bench.py: bracket the exchange section of every step with events on the compute stream (`exchange_ms`)
        self._xev = []
        self.m = self.v = self.sumsq = None
        self._sumsq_partials = None     # scratch of the fixed-order clip norm (`deterministic_norm`)
        self._range_tab = None          # device copy of `group_ranges()` and what it was built for
        self.reducer = None             # set by `overlap_grad_sync`: the exchange then runs in layer groups during the backward
        # parameters that live OUTSIDE the flat buffer: the positional-embedding MLPs and the user's pre / post transformer encoder-decoder
        # modules (PyTorch modules with autograd gradients).  They are few and small: a stock Adam steps them, under the SAME global clip
        # coefficient (their squared gradient norm is added to the flat buffer's before the fused kernel reads it)
        self.ext_params = (list(model.external_parameters()) if hasattr(model, 'external_parameters') else []) + head_params
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay))
        defaults = {k: defaults[k] for k in self._GROUP_KEYS}
        super().__init__(self._resolve_groups(outer, param_groups, _other_rule_params, self._GROUP_KEYS), defaults)
        self._ext_key, self.ext_opt = None, None
        self._sync_ext_opt()

    # ------------------------------------------------------------------ parameter groups
    @staticmethod
    def _resolve_groups(model, param_groups, other_rule_params=(), keys=_ADAM_KEYS):
        """`param_groups` (parameters or names) as torch's list of group dicts over `model.parameters()`: unnamed parameters join group 0;
        `other_rule_params` (a subclass steps them by another rule) leave whatever group names them"""
        params = list(model.parameters())
        known = {id(p) for p in params}
        other = {id(p) for p in other_rule_params}
        by_name = dict(model.named_parameters())
        if hasattr(model, 'student'):
            by_name.update((n, p) for n, p in model.student.named_parameters() if n not in by_name)
        groups = [dict(g) for g in param_groups] if param_groups is not None else [dict(params=params)]
        if not groups:
            raise ValueError('param_groups is empty')
        if len(groups) > capi.ENUMS['TFX_ADAM_MAX_GROUPS']:
            raise ValueError(f"{len(groups)} parameter groups: the fused Adam launch takes at most {capi.ENUMS['TFX_ADAM_MAX_GROUPS']}")
        seen = set()
        for g in groups:
            unknown = set(g) - set(keys) - {'params'}
            if unknown:
                raise ValueError(f'unknown keys in a parameter group: {sorted(unknown)} (taken: params, {", ".join(keys)})')
            listed = g.get('params', [])
            listed = [listed] if torch.is_tensor(listed) or isinstance(listed, str) else list(listed)
            out = []
            for p in listed:
                if isinstance(p, str):
                    if p not in by_name:
                        raise ValueError(f'parameter group names {p!r}, which is no parameter of the model')
                    p = by_name[p]
                if id(p) not in known:
                    raise ValueError('a parameter group holds a tensor that is no parameter of the model')
                if id(p) in seen:
                    raise ValueError('a parameter appears in two parameter groups')
                seen.add(id(p))
                if id(p) not in other:
                    out.append(p)
            g['params'] = out
        groups[0]['params'] += [p for p in params if id(p) not in seen and id(p) not in other]
        return groups

    def _adam_groups(self):
        """the groups the Adam rule steps (a subclass keeps another rule's group behind them)"""
        return self.param_groups

    def _group_scalars(self, g):
        b1, b2 = g['betas']
        return float(g['lr']), float(b1), float(b2), float(g['eps']), float(g['weight_decay']), int(bool(g.get('decoupled_weight_decay', False)))

    def _membership(self):
        return tuple(tuple(id(p) for p in g['params']) for g in self.param_groups)

    def _flat_offsets(self):
        """id(parameter) -> (element offset, padded elements) of the parameters that are views into the flat buffer"""
        ps = self.model.store
        return {id(p): (ps.offsets[n][0], -(-p.numel() // 4) * 4) for n, p in ps.params.items()}

    def group_ranges(self):
        """the host form of tfx_adam_group_args.ranges: sorted (start, end, group) over the whole flat buffer, bounds multiples of 4 (a segment's
        padding belongs to it), adjacent segments of one group merged.  Segments another rule owns (FusedMuon's matrices: the kernel skips them) ride
        with their left neighbour."""
        flat = self._flat_offsets()
        owner = {}
        for k, g in enumerate(self._adam_groups()):
            for p in g['params']:
                if id(p) in flat:
                    owner[flat[id(p)][0]] = k
        out = []
        for off, size in sorted(flat.values()):
            k = owner.get(off, out[-1][2] if out else None)
            if out and out[-1][2] in (k, None):
                out[-1][1], out[-1][2] = off + size, k
            else:
                out.append([off, off + size, k])
        return [(a, b, k or 0) for a, b, k in out]

    def _range_table(self, ps):
        key = (ps.flat.data_ptr(), str(ps.flat.device), self._membership())
        if self._range_tab is None or self._range_tab[0] != key:
            host = self.group_ranges()
            self._range_tab = (key, torch.tensor(host, dtype=torch.int64, device=ps.flat.device).reshape(-1), len(host))
        return self._range_tab[1], self._range_tab[2]

    def _sync_ext_opt(self):
        """the stock Adam of the external parameters: one torch group per group that holds some, the group's scalars every step (AdamW's rule where
        the group is decoupled).  Rebuilt, state kept, when the membership of the groups changes."""
        if not self.ext_params:
            return
        ext = {id(p) for p in self.ext_params}
        key = self._membership()
        if self._ext_key != key:
            members = [(g, [p for p in g['params'] if id(p) in ext]) for g in self._adam_groups()]
            state = dict(self.ext_opt.state) if self.ext_opt is not None else {}
            self._ext_groups = [g for g, ps_ in members if ps_]
            self.ext_opt = self._new_ext_opt([dict(params=ps_) for _, ps_ in members if ps_])
            for p, st in state.items():
                self.ext_opt.state[p] = st
            self._ext_key = key
        for src, grp in zip(self._ext_groups, self.ext_opt.param_groups):   # a schedule that sets `opt.lr = ...` or a group's lr reaches these too
            self._put_ext_scalars(src, grp)

    def _new_ext_opt(self, groups):
        """the PyTorch optimizer of the external parameters: this class's rule"""
        return torch.optim.Adam(groups)

    def _put_ext_scalars(self, src, grp):
        lr, b1, b2, eps, wd, dec = self._group_scalars(src)
        grp['lr'], grp['betas'], grp['eps'], grp['weight_decay'], grp['decoupled_weight_decay'] = src['lr'], (b1, b2), eps, wd, bool(dec)

    @contextlib.contextmanager
    def no_sync(self):
        """gradient accumulation (reference practice: `accelerator.accumulate(model)`, train_text_only.py:40, 117 = DDP's `no_sync()` around every
        micro-batch but the last): a backward inside this context only ADDS into the flat gradient buffer - with the overlapped exchange no layer
        group leaves (the buffer still changes), with the plain exchange nothing differs (its one all-reduce runs in `step()`).  The last
        micro-batch's backward, outside the context, sends the accumulated groups out as they become final."""
        red = self.reducer
        if red is None:
            yield
            return
        prev, red.defer = red.defer, True
        try:
            yield
        finally:
            red.defer = prev

    def overlap_grad_sync(self, groups: int = 4, exchange_dtype=None):
        """exchange the gradients in `groups` layer groups DURING the backward (GradReducer) instead of one all-reduce after it;
        `exchange_dtype=torch.bfloat16` halves the bytes on the links (the sum is formed in bf16; master gradients stay fp32)"""
        self.reducer = GradReducer(self.model, self.group, groups, exchange_dtype)
        self.model._grad_reducer = self.reducer
        self.model._dp_groups = self.reducer.groups
        return self

    def _world(self):
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.group)
        return 1

    def sync_grads(self):
        """the ONE collective of a data-parallel step: all-reduce(sum) of the flat gradient buffer (RCCL over xGMI)."""
        world = self._world()
        pending = self.reducer is not None and bool(self.reducer.done or self.reducer.exchanged)
        # (`pending`: the backward took the overlapped path - it does whenever torch.distributed is initialised, also at world size 1, e.g.
        #  `torchrun --nproc-per-node 1` - so its handles must be waited for and the reducer re-armed here whatever the world size)
        if world > 1 or pending or (self.always_sync and dist.is_initialized()):
            timed = self.time_exchange and self.model.store.grad is not None and self.model.store.grad.is_cuda
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if pending:
                self.reducer.finish()                  # the groups went out during the backward: tail + wait
                self.reducer.begin()
            else:
                dist.all_reduce(self.model.store.grad, op=dist.ReduceOp.SUM, group=self.group)
            if self.ext_params:
                # the external parameters: one more (small) collective over ALL of them, in declaration order, zeros where this rank's batch
                # produced no gradient (ragged multi-modal data: a rank without a modality type, or with text only, has `grad is None` for that
                # type's MLP / encoder) - every rank issues the same collective and, below, the same Adam step
                flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in self.ext_params])
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
                off = 0
                for p in self.ext_params:
                    g = flat[off:off + p.numel()].view_as(p).to(p.dtype); off += p.numel()
                    if p.grad is None:
                        p.grad = g.clone()
                    else:
                        p.grad.copy_(g)
            if timed:
                e1.record(); self._xev.append((e0, e1))
        return world

    def exchange_ms(self):
        """mean time per step the compute stream spent in the exchange section of `step()` - the tail collective plus the wait for the groups still
        in flight, i.e. what the overlap did NOT hide (call after a device synchronize; `time_exchange` must be on)"""
        ms = [a.elapsed_time(b) for a, b in self._xev]
        self._xev = []
        return sum(ms) / len(ms) if ms else 0.0

    def step(self):
        ps = self.model.store
        if ps.grad is None:
            raise capi.TfxError('FusedAdam needs the model on an MI355X (model.cuda())')
        world = self.sync_grads()
        self._ensure_state(ps)
        stream = torch.cuda.current_stream(ps.flat.device).cuda_stream
        self.step_count += 1
        max_norm = float(self.max_grad_norm) if self.max_grad_norm else 0.
        gscale = (1.0 / world) if (self.average and world > 1) else 1.0
        ext_grads = [p.grad for p in self.ext_params if p.grad is not None]
        if max_norm > 0:
            if self.deterministic_norm:
                if self._sumsq_partials is None or self._sumsq_partials.device != ps.flat.device:
                    self._sumsq_partials = torch.zeros(capi.ENUMS['TFX_SUMSQ_DET_PARTIALS'], device=ps.flat.device)
                capi.check(capi.lib().tfx_sumsq_det(ps.grad.data_ptr(), ps.numel, self._sumsq_partials.data_ptr(), self.sumsq.data_ptr(), stream), 'tfx_sumsq_det')
            else:
                self.sumsq.zero_()
                capi.check(capi.lib().tfx_sumsq(ps.grad.data_ptr(), ps.numel, self.sumsq.data_ptr(), stream), 'tfx_sumsq')
            if ext_grads:
                self.sumsq += torch.stack([g.float().pow(2).sum() for g in ext_grads]).sum()
        if ext_grads:                                       # same scaling as adam_k: grad_scale * min(1, max_norm / (|g| grad_scale + 1e-6)), on the device
            coef = torch.full((), gscale, device=ps.flat.device)
            if max_norm > 0:
                coef = coef * (max_norm / (self.sumsq[0].sqrt() * gscale + 1e-6)).clamp(max=1.)
            for g in ext_grads:
                g.mul_(coef)
            self._sync_ext_opt()
            self.ext_opt.step()
        self._step_other_rules(ps, stream, max_norm, gscale)
        skip, nskip = self._skip_table(ps)
        groups = self._adam_groups()
        lr, beta1, beta2, eps, wd, decoupled = self._group_scalars(groups[0])
        common = dict(p=ps.flat, g=ps.grad, m=self.m, v=self.v, n=ps.numel, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=wd, max_norm=max_norm,
                      grad_scale=gscale, step=self.step_count, sumsq=self.sumsq, skip=skip, nskip=nskip)
        self._launch_rule(ps, stream, groups, decoupled, common)
        # the master changed behind autograd's back: new weights epoch (shadows rebuilt, kept decode plans dropped)
        ps.mark_dirty()

    def _group_table(self, ps, groups):
        """the fields of tfx_adam_group_args behind `decoupled` for more than one group: the device range table and the groups' records by value"""
        ranges, nrange = self._range_table(ps)
        rec = list(zip(*(self._group_scalars(g) for g in groups)))
        return dict(ranges=ranges, nrange=nrange, ngroup=len(groups), group_lr=rec[0], group_beta1=rec[1], group_beta2=rec[2], group_eps=rec[3],
                    group_weight_decay=rec[4], group_decoupled=rec[5])

    def _launch_rule(self, ps, stream, groups, decoupled, common):
        """the one launch over the flat buffer: the rule's entry point, the group table only for more than one group"""
        entry, args = self._RULE_LAUNCH
        fields = dict(self._rule_fields(), decoupled=decoupled, **(self._group_table(ps, groups) if len(groups) > 1 else {}))
        if entry == 'tfx_adam_step_groups' and len(groups) == 1 and not decoupled:      # the launch FusedAdam always made
            entry, args, fields = 'tfx_adam_step', 'tfx_adam_args', {}
        capi.call(entry, capi.make_args(args, **fields, **common), stream)

    def _step_other_rules(self, ps, stream, max_norm, gscale):
        """hook of subclasses that update part of the flat buffer by another rule, between the clip norm and the Adam launch; what they own there
        they name in `_other_rule_ranges`"""

    def _other_rule_ranges(self):
        """hook of subclasses: sorted, disjoint [start, end) element ranges (multiples of 4) another rule owns - Adam leaves them alone"""
        return []

    def frozen_ranges(self):
        """sorted, merged [start, end) element ranges of the flat buffer that belong to parameters with `requires_grad` False (multiples of 4: a
        segment's padding belongs to it).  No rule touches them: value, `exp_avg` / `exp_avg_sq`, Muon momentum and weight decay all stay, bit for bit."""
        return self.model.store.frozen_ranges()

    @staticmethod
    def merge_ranges(*lists):
        """the union of sorted range lists as one sorted list of disjoint [start, end) ranges (touching ranges merge)"""
        out = []
        for a, b in sorted(r for l in lists for r in l):
            if out and out[-1][1] >= a:
                out[-1][1] = max(out[-1][1], b)
            else:
                out.append([a, b])
        return [tuple(r) for r in out]

    def skip_table(self):
        """host form of tfx_adam_args.skip: what another rule owns merged with `frozen_ranges()`"""
        return self.merge_ranges(self._other_rule_ranges(), self.frozen_ranges())

    def _skip_table(self, ps):
        """the device skip table of the Adam launch and its length (None, 0 when nothing is skipped: the launch FusedAdam always made); rebuilt when the
        flat buffer moves or the frozen set changes"""
        key = (ps.flat.data_ptr(), str(ps.flat.device), ps.frozen_names(), self._skip_key())
        if self._skip_tab is None or self._skip_tab[0] != key:
            host = self.skip_table()
            dev = torch.tensor(host, dtype=torch.int64, device=ps.flat.device).reshape(-1) if host else None
            self._skip_tab = (key, dev, len(host))
        return self._skip_tab[1], self._skip_tab[2]

    _skip_tab = None

    def _skip_key(self):
        return None

    def _ensure_state(self, ps):
        """the moments and the clip norm's scalar, on the flat buffer's device (moments that exist move with it: a loaded state is not lost)"""
        if self.m is None or self.m.numel() != ps.numel:
            self.m = torch.zeros_like(ps.flat); self.v = torch.zeros_like(ps.flat)
        elif self.m.device != ps.flat.device:
            self.m, self.v = (self.m.to(ps.flat.device), self.v.to(ps.flat.device)) if self.step_count else (torch.zeros_like(ps.flat), torch.zeros_like(ps.flat))
        if self.sumsq is None or self.sumsq.device != ps.flat.device:
            self.sumsq = torch.zeros(1, device=ps.flat.device)

    # ------------------------------------------------------------------ state (torch.optim's format)
    def _other_rule_state(self, p):
        """hook of subclasses: the state entry of a flat-buffer parameter another rule steps (None: Adam's)"""
        return None

    def _load_other_rule_state(self, p, entry):
        return False

    def _rule_keys(self, g):
        """the scalars group `g` carries under its rule (a subclass keeps another rule's group)"""
        return self._GROUP_KEYS

    def _saved_under_this_rule(self, g, sg):
        """a saved group is this rule's when it carries every scalar of the rule and none that only another fused rule knows (`eps` in a group of
        the Adam-atan2 rule: Adam's)"""
        keys, known = set(self._rule_keys(g)), set(_ADAM_KEYS) | set(_ATAN2_KEYS) | set(FusedMuon._MUON_KEYS)
        return keys - {'decoupled_weight_decay'} <= set(sg) and not (set(sg) & known) - keys      # (torch.optim.Adam of older releases saves no decoupled_weight_decay)

    def _indexed_params(self):
        return [p for g in self.param_groups for p in g['params']]

    def state_dict(self):
        """`torch.optim.Optimizer.state_dict()`'s format: indices over the groups in order; per flat-buffer parameter `step` (the one step count),
        `exp_avg`, `exp_avg_sq` as views of `m` / `v`; the external parameters' entries are their stock Adam's.  Empty before the first step."""
        groups, start = [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != 'params'}
            packed['params'] = list(range(start, start + len(g['params'])))
            start += len(g['params'])
            groups.append(packed)
        state = {}
        flat = self._flat_offsets()
        for i, p in enumerate(self._indexed_params()):
            if id(p) in flat:
                if self.m is None or self.step_count == 0:
                    continue
                other = self._other_rule_state(p)
                if other is not None:
                    state[i] = other
                    continue
                off = flat[id(p)][0]
                state[i] = dict(step=torch.tensor(float(self.step_count)), exp_avg=self.m[off:off + p.numel()].view(p.shape),
                                exp_avg_sq=self.v[off:off + p.numel()].view(p.shape))
            elif self.ext_opt is not None and p in self.ext_opt.state and self.ext_opt.state[p]:
                state[i] = dict(self.ext_opt.state[p])
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, state_dict):
        """takes a `state_dict()` of this class or of `torch.optim.Adam` / `AdamW` over the same parameters in the same groups: the groups'
        scalars, the moments (copied into `m` / `v`; a missing entry means zeros) and the step count.  ValueError where group or parameter counts or
        shapes differ, and where the flat-buffer parameters' steps differ (the fused launch has one bias correction)."""
        saved = state_dict['param_groups']
        if len(saved) != len(self.param_groups):
            raise ValueError(f'loaded state dict has {len(saved)} parameter groups, the optimizer has {len(self.param_groups)}')
        index = {}
        for g, sg in zip(self.param_groups, saved):
            if len(sg['params']) != len(g['params']):
                raise ValueError(f"loaded state dict has a parameter group of {len(sg['params'])} parameters where the optimizer's has {len(g['params'])}")
            if sg.get('amsgrad') or sg.get('maximize'):
                raise ValueError('amsgrad / maximize states cannot be loaded: the fused Adam launch has neither')
            index.update(zip(sg['params'], g['params']))
        entries = {k: e for k, e in state_dict['state'].items() if e}
        for k in entries:
            if k not in index:
                raise ValueError(f'loaded state dict has an entry for parameter {k}, which no group holds')
        flat, ext = self._flat_offsets(), {id(p) for p in self.ext_params}
        steps = set()
        for k, e in entries.items():
            p = index[k]
            for name in ('exp_avg', 'exp_avg_sq', 'momentum_buffer'):
                if name in e and tuple(e[name].shape) != tuple(p.shape):
                    raise ValueError(f'loaded state of parameter {k}: {name} has shape {tuple(e[name].shape)}, the parameter {tuple(p.shape)}')
            if id(p) in flat and 'step' in e:
                steps.add(float(e['step']))
        if len(steps) > 1:
            raise ValueError(f'the loaded parameters are at different steps ({sorted(steps)}): the fused Adam launch has one bias correction for the whole buffer')
        for g, sg in zip(self.param_groups, saved):
            if self._saved_under_this_rule(g, sg):          # a group saved under another rule (Adam <-> Adam-atan2) brings its moments, not its scalars
                g.update({k: v for k, v in sg.items() if k != 'params'})
        ps = self.model.store
        self.step_count = int(steps.pop()) if steps else 0
        if entries or self.m is not None:
            self.m = self.v = None
            self._ensure_state(ps)
        if self.ext_opt is not None:
            self.ext_opt.state.clear()
        with torch.no_grad():
            for k, e in entries.items():
                p = index[k]
                if id(p) in flat:
                    if self._load_other_rule_state(p, e):
                        continue
                    if 'exp_avg' not in e or 'exp_avg_sq' not in e:
                        raise ValueError(f'loaded state of parameter {k} has no exp_avg / exp_avg_sq')
                    off = flat[id(p)][0]
                    self.m[off:off + p.numel()].view(p.shape).copy_(e['exp_avg'])
                    self.v[off:off + p.numel()].view(p.shape).copy_(e['exp_avg_sq'])
                elif id(p) in ext:
                    self.ext_opt.state[p] = {n: t if not torch.is_tensor(t) else t.detach().float().cpu().clone() if n == 'step' else t.to(p.device, p.dtype).clone()
                                             for n, t in e.items()}
        self._ext_key = None
        self._sync_ext_opt()

    def zero_grad(self, set_to_none: bool = True):
        ps = self.model.store
        if self.ext_opt is not None:
            self.ext_opt.zero_grad(set_to_none=set_to_none)
        if set_to_none:
            for p in ps.params.values():
                p.grad = None
        elif ps.grad is not None:
            ps.grad.zero_()


class _MuonTables:
    """device tables of one FusedMuon over one flat buffer: matrix descriptors, the bf16 workspace, the problem tables of the grouped products"""


def _muon_host_tables(segs, adjust_lr_fn=None):
    """the step's tables as host data (no device needed): matrix descriptors and the problems of the grouped products, with workspace OFFSETS
    (elements) where the device tables carry pointers.  `segs`: sorted (offset, rows, cols) of the matrices in the flat buffers."""
    mats, blk_mat, sq_prob, up_prob = [], [], [], []
    xw = abw = blk = sq_t = up_t = 0
    for i, (off, rows, cols) in enumerate(segs):
        pl = FusedMuon.plan(rows, cols)
        mp, np_ = pl['m_pad'], pl['n_pad']
        x_off, xt_off = xw, xw + mp * np_
        xw += 2 * mp * np_
        a_off, b_off = abw, abw + mp * mp
        abw += 2 * mp * mp
        flip = pl['flip']
        mats.append(dict(off=off, s_off=xt_off if flip else x_off, t_off=x_off if flip else xt_off, rows=rows, cols=cols,
                         ld_s=mp if flip else np_, ld_t=np_ if flip else mp, blk0=blk, lr_ratio=FusedMuon._lr_ratio(adjust_lr_fn, rows, cols),
                         x_off=x_off, xt_off=xt_off, a_off=a_off, b_off=b_off, sq_tile0=sq_t, up_tile0=up_t, **pl))
        blk_mat += [i] * pl['prep_blocks']; blk += pl['prep_blocks']
        sq_prob += [i] * pl['gram_tiles']; sq_t += pl['gram_tiles']
        up_prob += [i] * pl['update_tiles']; up_t += pl['update_tiles']
    return dict(mats=mats, blk_mat=blk_mat, sq_prob=sq_prob, up_prob=up_prob, x_elems=xw, ab_elems=abw)


def _muon_device_tables(H, dev):
    T = _MuonTables()
    T.H, T.nmat, T.nblk = H, len(H['mats']), len(H['blk_mat'])
    T.sq_tiles, T.up_tiles = len(H['sq_prob']), len(H['up_prob'])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    T.blk_mat, T.sq_prob, T.up_prob = i32(H['blk_mat']), i32(H['sq_prob']), i32(H['up_prob'])
    # zero-filled ONCE: the kernels write zeros (products of zeros) or nothing into the padding
    T.wsx = [torch.zeros(H['x_elems'], dtype=torch.bfloat16, device=dev) for _ in range(2)]
    T.wsab = torch.zeros(H['ab_elems'], dtype=torch.bfloat16, device=dev)
    T.partials = torch.zeros(T.nblk, device=dev)
    T.inv = torch.zeros(2 * T.nmat, device=dev)

    def upload(struct, rows):
        S = capi.STRUCTS[struct]
        names = {f for f, _ in capi.STRUCT_FIELDS[struct]}
        arr = (S * len(rows))()
        for a, r in zip(arr, rows):
            for k, v in r.items():
                if k in names:
                    setattr(a, k, v)
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

    T.mats = upload('tfx_muon_mat', H['mats'])
    x = [w.data_ptr() for w in T.wsx]
    ab, inv = T.wsab.data_ptr(), T.inv.data_ptr()

    def gram(cur, first):
        return upload('tfx_muon_gemm_problem', [dict(P=x[cur] + 2 * m['x_off'], Q=x[cur] + 2 * m['x_off'], C=ab + 2 * m['a_off'],
                                                     scale_acc=inv + 4 * (2 * i + 1) if first else None, M=m['m_pad'], N=m['m_pad'], K=m['n_pad'],
                                                     ldp=m['n_pad'], ldq=m['n_pad'], ldc=m['m_pad'], tile0=m['sq_tile0']) for i, m in enumerate(H['mats'])])

    def update(cur, first):
        s = lambda i: inv + 4 * (2 * i) if first else None
        return upload('tfx_muon_gemm_problem', [dict(P=x[cur] + 2 * m['xt_off'], Z=x[cur] + 2 * m['xt_off'], Q=ab + 2 * m['b_off'],
                                                     C=x[cur ^ 1] + 2 * m['xt_off'], Ct=x[cur ^ 1] + 2 * m['x_off'], scale_z=s(i), scale_acc=s(i),
                                                     M=m['n_pad'], N=m['m_pad'], K=m['m_pad'], ldp=m['m_pad'], ldz=m['m_pad'], ldq=m['m_pad'],
                                                     ldc=m['m_pad'], ldct=m['n_pad'], tile0=m['up_tile0']) for i, m in enumerate(H['mats'])])

    T.gram_first, T.gram = gram(0, True), [gram(0, False), gram(1, False)]
    T.update_first, T.update = update(0, True), [update(0, False), update(1, False)]
    T.poly = upload('tfx_muon_gemm_problem', [dict(P=ab + 2 * m['a_off'], Q=ab + 2 * m['a_off'], Z=ab + 2 * m['a_off'], C=ab + 2 * m['b_off'],
                                                   M=m['m_pad'], N=m['m_pad'], K=m['m_pad'], ldp=m['m_pad'], ldq=m['m_pad'], ldz=m['m_pad'],
                                                   ldc=m['m_pad'], tile0=m['sq_tile0']) for m in H['mats']])
    return T


def _muon_orthogonalize(T, g, buf, sumsq, max_norm, gscale, momentum, nesterov, eps, coefficients, ns, stream):
    """momentum + norms + ns Newton-Schulz iterations over all matrices of the tables `T`: 2 + 3 ns launches.  The final iterate is in T.wsx[ns & 1]."""
    if not 1 <= ns < 100:
        raise ValueError('ns_steps must be in 1 ... 99')
    a, b, c = (float(x) for x in coefficients)
    L = capi.lib()
    prep = capi.make_args('tfx_muon_prep_args', mats=T.mats, blk_mat=T.blk_mat, nmat=T.nmat, nblk=T.nblk, g=g, buf=buf, ws=T.wsx[0],
                          partials=T.partials, sumsq=sumsq, max_norm=max_norm, grad_scale=gscale, momentum=float(momentum), nesterov=int(bool(nesterov)))
    capi.call('tfx_muon_prep', prep, stream)
    capi.check(L.tfx_muon_norm(T.mats.data_ptr(), T.nmat, T.partials.data_ptr(), float(eps), T.inv.data_ptr(), stream), 'tfx_muon_norm')
    gemm = lambda tab, prob, tiles, al, be: capi.check(L.tfx_muon_gemm(tab.data_ptr(), prob.data_ptr(), tiles, al, be, stream), 'tfx_muon_gemm')
    for t in range(ns):
        cur = t & 1
        gemm(T.gram_first if t == 0 else T.gram[cur], T.sq_prob, T.sq_tiles, 0., 1.)
        gemm(T.poly, T.sq_prob, T.sq_tiles, b, c)
        gemm(T.update_first if t == 0 else T.update[cur], T.up_prob, T.up_tiles, a, 1.)


def newton_schulz(mats, ns_coefficients=(3.4445, -4.775, 2.0315), ns_steps=5, eps=1e-7):
    """`torch.optim._muon._zeropower_via_newtonschulz` (_muon.py:24-62) of a LIST of 2-D fp32 tensors on the MI355X through the grouped kernels of
    FusedMuon - all matrices per launch.  Returns the bf16 results in the inputs' own orientation."""
    dev = mats[0].device
    segs, off = [], 0
    for m in mats:
        if m.ndim != 2 or m.device != dev or not m.is_cuda:
            raise ValueError('newton_schulz takes 2-D tensors on one GPU')
        segs.append((off, m.shape[0], m.shape[1])); off += -(-m.numel() // 4) * 4
    g = torch.zeros(off, device=dev)
    for (o, r, c), m in zip(segs, mats):
        g[o:o + r * c].copy_(m.reshape(-1))
    T = _muon_device_tables(_muon_host_tables(segs), dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # momentum 0 without the Nesterov mix: u = g
    _muon_orthogonalize(T, g, torch.zeros_like(g), None, 0., 1., 0., False, eps, ns_coefficients, int(ns_steps), stream)
    ws = T.wsx[int(ns_steps) & 1]
    return [ws[d['s_off']:d['s_off'] + d['rows'] * d['ld_s']].view(d['rows'], d['ld_s'])[:, :d['cols']].clone() for d in T.H['mats']]


class FusedMuon(FusedAdam):
    """Muon over `model.muon_parameters()` (train_image_only.py:90: `MuonAdamAtan2(model.muon_parameters(), model.parameters(), ...)`), the fused
    Adam over everything else - one optimizer object, one `step()`.  Gradient exchange, `no_sync`, `overlap_grad_sync`, external parameters, the
    device-side global clip and `zero_grad` are FusedAdam's; the clip coefficient is the same for both shares.

    The Muon rule is `torch.optim.Muon`'s (torch/optim/_muon.py), with its keyword names and defaults - prefixed `muon_` where Adam has the name:
        buf = lerp(buf, g, 1 - momentum);  u = lerp(g, buf, momentum) if nesterov else buf
        X = u / max(|u|_F, muon_eps), transposed if rows > cols;  ns_steps x { A = X X^T; B = b A + c A A; X = a X + B X }  (bf16 operands, fp32 sums)
        p = p (1 - muon_lr muon_weight_decay) - adjust_lr(muon_lr, shape) X
    All matrices go through every stage together (csrc/muon.hip): the number of launches of a step does not depend on the depth, and nothing in
    the path is an atomic or an order-varying sum, so replicas that orthogonalise the same all-reduced gradient stay bit-identical.
    The momentum of a matrix lives in the Adam first-moment buffer at the matrix's own range (`momentum_buffer(p)`); Adam skips those ranges.
    Muon's share is the LAST parameter group, under torch.optim.Muon's key names (`muon_lr` and the other attributes alias it); the Adam share takes
    `param_groups` as FusedAdam does.  Every scalar (`lr`, `muon_lr`, `momentum`, ...) is re-read at each step."""

    deterministic_norm = True

    _MUON_KEYS = ('lr', 'weight_decay', 'momentum', 'nesterov', 'ns_coefficients', 'eps', 'ns_steps', 'adjust_lr_fn')       # torch.optim.Muon's group keys
    muon_lr, muon_weight_decay, momentum, nesterov, ns_coefficients, muon_eps, ns_steps, adjust_lr_fn = (_group_alias(k, -1) for k in _MUON_KEYS)

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0., max_grad_norm=None, process_group=None, average_grads=True, *,
                 muon_params=None, muon_lr=1e-3, muon_weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.775, 2.0315),
                 ns_steps=5, muon_eps=1e-7, adjust_lr_fn=None, param_groups=None, decoupled_weight_decay=False):
        muon = list(model.muon_parameters() if muon_params is None else muon_params)
        if not muon:
            raise ValueError('FusedMuon needs at least one matrix (use FusedAdam otherwise)')
        lora = {id(p) for p in model.store.lora.parameters()} if getattr(getattr(model, 'store', None), 'lora', None) else set()
        for p in muon:
            if id(p) in lora:
                raise NotImplementedError('LoRA adapter parameters in a Muon group are not supported: they are stepped by the Adam share (external parameters)')
            if p.ndim != 2:
                raise ValueError(f'Muon parameters must be 2-D matrices, got shape {tuple(p.shape)}')
        # the Adam share takes groups as FusedAdam does (the matrices leave whatever group lists them: `decay_groups(model, ...)` may be passed
        # as it is); Muon's share is the LAST group, under torch.optim.Muon's key names - a scheduler scales both learning rates
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, process_group=process_group,
                         average_grads=average_grads, param_groups=param_groups, decoupled_weight_decay=decoupled_weight_decay, _other_rule_params=muon)
        self.param_groups.append(dict(params=muon, lr=muon_lr, weight_decay=muon_weight_decay, momentum=momentum, nesterov=nesterov,
                                      ns_coefficients=ns_coefficients, eps=muon_eps, ns_steps=ns_steps, adjust_lr_fn=adjust_lr_fn))
        self._muon_group = True
        self._sync_ext_opt()
        self._tab = None

    @property
    def muon_params(self):
        return self.param_groups[-1]['params']

    _muon_group = False               # until the constructor has appended it

    def _adam_groups(self):
        return self.param_groups[:-1] if self._muon_group else self.param_groups

    def _rule_keys(self, g):
        return self._MUON_KEYS if self._muon_group and g is self.param_groups[-1] else super()._rule_keys(g)

    def _other_rule_state(self, p):
        if any(p is q for q in self.muon_params):
            return dict(momentum_buffer=self.momentum_buffer(p))
        return None

    def _load_other_rule_state(self, p, entry):
        if not any(p is q for q in self.muon_params):
            return False
        if 'momentum_buffer' in entry and entry['momentum_buffer'] is not None:
            self.momentum_buffer(p).copy_(entry['momentum_buffer'])
        return True

    # ------------------------------------------------------------------ host tables
    def muon_segments(self):
        """sorted (offset, rows, cols) of the Muon matrices in the flat buffer (every one must be a contiguous fp32 view into it)"""
        ps = self.model.store
        base, segs = ps.flat.data_ptr(), []
        ps.params_version()                                           # re-points parameters whose .data was re-assigned
        for p in self.muon_params:
            off = p.data_ptr() - base
            if p.dtype != torch.float32 or not p.is_contiguous() or off < 0 or off % 4 or off // 4 + p.numel() > ps.numel:
                raise ValueError('a Muon parameter must be a contiguous fp32 view into the model\'s flat parameter buffer')
            segs.append((off // 4, p.shape[0], p.shape[1]))
        segs.sort()
        for (o0, r0, c0), (o1, _, _) in zip(segs, segs[1:]):
            if o0 + r0 * c0 > o1:
                raise ValueError('Muon parameters overlap')
        return segs

    @staticmethod
    def _lr_ratio(adjust_lr_fn, rows, cols):                          # _muon.py:65-77
        if adjust_lr_fn is None or adjust_lr_fn == 'original':
            return max(1., rows / cols) ** 0.5
        if adjust_lr_fn == 'match_rms_adamw':
            return 0.2 * max(rows, cols) ** 0.5
        raise ValueError(f"adjust_lr_fn must be None, 'original' or 'match_rms_adamw', got {adjust_lr_fn!r}")

    @staticmethod
    def plan(rows, cols):
        """tfx_muon_plan (host only): dict of flip, m, n, m_pad, n_pad, gram_tiles, update_tiles, prep_blocks for a rows x cols parameter"""
        import ctypes
        keys = ('flip', 'm', 'n', 'm_pad', 'n_pad', 'gram_tiles', 'update_tiles', 'prep_blocks')
        out = [ctypes.c_int32() for _ in keys]
        capi.check(capi.lib().tfx_muon_plan(int(rows), int(cols), *[ctypes.byref(o) for o in out]), 'tfx_muon_plan')
        return {k: o.value for k, o in zip(keys, out)}

    def launches_per_step(self):
        """kernel launches of one step's optimizer share (clip norm, Muon chain, Adam) - independent of the number of matrices"""
        return capi.lib().tfx_muon_step_launches(int(self.ns_steps), len(self.muon_params))

    def _active_segments(self):
        """`muon_segments()` without the frozen matrices: those leave the Muon tables - no orthogonalisation, no apply, momentum untouched"""
        ps = self.model.store
        frozen = {ps.offsets[n][0] for n in ps.frozen_names()}
        return [s for s in self.muon_segments() if s[0] not in frozen]

    def _other_rule_ranges(self):
        return self.adam_skip_table()

    def _skip_key(self):
        return tuple(id(p) for p in self.muon_params)

    def skip_ranges(self):
        """sorted [start, end) element ranges of the flat buffer that Muon owns and Adam skips (adjacent matrices merged)"""
        out = []
        for off, r, c in self.muon_segments():
            if out and out[-1][1] == off:
                out[-1][1] = off + r * c
            else:
                out.append([off, off + r * c])
        return [tuple(x) for x in out]

    def adam_skip_table(self):
        """`skip_ranges()` as tfx_adam_args.skip takes them: whole groups of 4 elements.  Segments of the flat buffer start at multiples of 4 and are
        padded to one, so an end rounded up covers padding only"""
        skip = []
        for a, b in self.skip_ranges():
            if a % 4:
                raise ValueError('a Muon parameter must start at a multiple of 4 elements of the flat buffer')
            b = -(-b // 4) * 4
            if skip and skip[-1][1] >= a:
                skip[-1][1] = b
            else:
                skip.append([a, b])
        return [tuple(x) for x in skip]

    def host_tables(self):
        """the step's tables as host data (no device needed): matrix descriptors and the problems of the grouped products, with workspace OFFSETS
        (elements) where the device tables carry pointers"""
        return _muon_host_tables(self._active_segments(), self.adjust_lr_fn)

    def _tables(self, ps):
        # (the parameters are views into `flat`: they move only with it - `reflatten` - and a re-assigned `.data` is copied back and re-pointed by
        #  the forward's `params_version()`; the fused kernels read the flat buffer either way, as FusedAdam's do)
        key = (ps.flat.data_ptr(), str(ps.flat.device), self.adjust_lr_fn, ps.frozen_names())
        if self._tab is None or self._tab.key != key:
            H = self.host_tables()
            self._tab = _muon_device_tables(H, ps.flat.device) if H['mats'] else _MuonTables()      # (every matrix frozen: no Muon launch at all)
            self._tab.key, self._tab.nmat = key, len(H['mats'])
        return self._tab

    def momentum_buffer(self, p):
        """Muon's momentum of matrix `p`: a view of the first-moment buffer at the matrix's range (None before the first step)"""
        if self.m is None:
            return None
        off = (p.data_ptr() - self.model.store.flat.data_ptr()) // 4
        return self.m[off:off + p.numel()].view(p.shape)

    # ------------------------------------------------------------------ the step
    def _step_other_rules(self, ps, stream, max_norm, gscale):
        ns = int(self.ns_steps)
        T = self._tables(ps)
        if not T.nmat:
            return
        _muon_orthogonalize(T, ps.grad, self.m, self.sumsq, max_norm, gscale, self.momentum, self.nesterov, self.muon_eps, self.ns_coefficients, ns, stream)
        lr, wd = float(self.muon_lr), float(self.muon_weight_decay)
        app = capi.make_args('tfx_muon_apply_args', mats=T.mats, blk_mat=T.blk_mat, nmat=T.nmat, nblk=T.nblk, p=ps.flat, ws=T.wsx[ns & 1],
                             lr=lr, decay=1. - lr * wd)
        capi.call('tfx_muon_apply', app, stream)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The Adam-atan2 rule (Everett et al., "Scaling Exponents Across Parameterizations and Optimizers", 2024): the update  a atan2(m / bc1, b sqrt(v / bc2))
# in place of  (m / bc1) / (sqrt(v / bc2) + eps).  train_image_only.py:90 trains with `MuonAdamAtan2` of the adam_atan2_pytorch package, which is not
# vendored with the reference: the arithmetic below and in `tfx_adam_atan2_step` is RESTATED from the published definition (the defaults a = 1.27,
# b = 1, betas = (0.9, 0.99), lr = 1e-4 are the package's as published) and is parity-unpinned.  Not built: the package's `cautious_factor` and
# `regen_reg_rate`, Adam and atan2 groups in one launch, the package's own Muon arithmetic.

def _as_f32(x):
    return struct.unpack('f', struct.pack('f', float(x)))[0]


def _check_atan2_ab(a, b):
    if not (float(a) > 0. and float(b) > 0.):
        raise ValueError(f'the Adam-atan2 rule needs a > 0 and b > 0, got a = {a!r}, b = {b!r}')


class AdamAtan2(torch.optim.Optimizer):
    """The Adam-atan2 rule in fp32 PyTorch, for the parameters outside the flat buffer (FusedAdamAtan2 / FusedMuonAdamAtan2 step the external
    parameters with it) and as the rule's reference form.  The operations of `tfx_adam_atan2_step` (include/tfx.h), with its group semantics:
        w = p (1 - lr wd) if decoupled else p;  g += wd w for the L2 form;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g
        p = w - lr a atan2(m / bc1, b sqrt(v) / sqrt(bc2))
    No eps; zero gradient on zero state moves nothing; every element moves by at most lr a pi / 2.  State keys are torch.optim.Adam's."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), a=1.27, b=1., weight_decay=0., decoupled_weight_decay=False):
        _check_atan2_ab(a, b)
        super().__init__(params, dict(lr=lr, betas=betas, a=a, b=b, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay)))

    @torch.no_grad()
    def step(self):
        for grp in self.param_groups:
            # the scalars as the fused launch carries them: fp32 values
            lr, b1, b2, a, b, wd = (_as_f32(x) for x in (grp['lr'], *grp['betas'], grp['a'], grp['b'], grp['weight_decay']))
            _check_atan2_ab(a, b)
            dec = bool(grp.get('decoupled_weight_decay', False))
            for p in grp['params']:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st['step'] = torch.tensor(0.)
                    st['exp_avg'] = torch.zeros_like(p, dtype=torch.float32)
                    st['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32)
                st['step'] += 1
                t = int(st['step'])
                m, v = st['exp_avg'], st['exp_avg_sq']
                g = p.grad.float()
                w = p.float() * (1. - lr * wd) if dec and wd != 0. else p.float()
                if wd != 0. and not dec:
                    g = g + wd * w
                m.mul_(b1).add_(g, alpha=1. - b1)
                v.mul_(b2).addcmul_(g, g, value=1. - b2)
                theta = torch.atan2(m * (1. / (1. - b1 ** t)), v.sqrt() * (b / (1. - b2 ** t) ** 0.5))
                p.copy_(w - (lr * a) * theta)


class _Atan2Rule:
    """what turns FusedAdam / FusedMuon into their Adam-atan2 forms: groups without eps, optimizer-wide `a` and `b` (re-read at every step),
    `tfx_adam_atan2_step` as the launch over the flat buffer, AdamAtan2 for the external parameters"""

    _GROUP_KEYS = _ATAN2_KEYS
    _RULE_LAUNCH = 'tfx_adam_atan2_step', 'tfx_adam_atan2_args'

    @property
    def eps(self):
        raise AttributeError('the Adam-atan2 rule has no eps')

    def _group_scalars(self, g):
        b1, b2 = g['betas']
        return float(g['lr']), float(b1), float(b2), 0., float(g['weight_decay']), int(bool(g.get('decoupled_weight_decay', False)))

    def _new_ext_opt(self, groups):
        return AdamAtan2(groups, a=self.a, b=self.b)

    def _put_ext_scalars(self, src, grp):
        lr, b1, b2, _, wd, dec = self._group_scalars(src)
        grp['lr'], grp['betas'], grp['weight_decay'], grp['decoupled_weight_decay'], grp['a'], grp['b'] = src['lr'], (b1, b2), wd, bool(dec), self.a, self.b

    def _rule_fields(self):
        _check_atan2_ab(self.a, self.b)
        return dict(atan2_a=float(self.a), atan2_b=float(self.b))


class FusedAdamAtan2(_Atan2Rule, FusedAdam):
    """FusedAdam with the Adam-atan2 rule: global-norm clip + one `tfx_adam_atan2_step` launch over the flat fp32 buffer.  Parameter groups
    (`lr`, `betas`, `weight_decay`, `decoupled_weight_decay`; no `eps`: a group that names `eps`, `a` or `b` is a ValueError), `decay_groups`,
    `group_ranges()`, `no_sync`, `overlap_grad_sync`, `deterministic_norm`, the gradient exchange and the `torch.optim` state format are FusedAdam's.
    `a` and `b` are optimizer-wide attributes, re-read at every step.  The external parameters are stepped by AdamAtan2, under the same clip
    coefficient.  The moments mean what Adam's mean: a FusedAdam / torch.optim.Adam `state_dict()` loads here and the other way round - the
    moments and the step count carry over, the groups' scalars stay the loading optimizer's.
    Restated from the published rule, parity-unpinned (see above); `cautious_factor`, `regen_reg_rate` and mixed rules in one launch are not built."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.99), a=1.27, b=1., weight_decay=0., max_grad_norm=None, process_group=None, average_grads=True, *,
                 param_groups=None, decoupled_weight_decay=False):
        _check_atan2_ab(a, b)
        self.a, self.b = a, b
        super().__init__(model, lr=lr, betas=betas, weight_decay=weight_decay, max_grad_norm=max_grad_norm, process_group=process_group,
                         average_grads=average_grads, param_groups=param_groups, decoupled_weight_decay=decoupled_weight_decay)


class FusedMuonAdamAtan2(_Atan2Rule, FusedMuon):
    """train_image_only.py:90, `MuonAdamAtan2(model.muon_parameters(), model.parameters(), lr = 8e-4)`: FusedMuon with the Adam-atan2 rule for
    everything Muon does not own.  The Muon share - launches, arguments, bits - is FusedMuon's (`torch.optim.Muon`'s rule, NOT the package's own
    Muon arithmetic); `tfx_adam_atan2_step(skip)` takes the place of `tfx_adam_step(skip)` at the end of the chain, so a step has FusedMuon's
    launch count.  Restated from the published rule, parity-unpinned."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.99), a=1.27, b=1., weight_decay=0., max_grad_norm=None, process_group=None, average_grads=True, *,
                 muon_params=None, muon_lr=1e-3, muon_weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.775, 2.0315),
                 ns_steps=5, muon_eps=1e-7, adjust_lr_fn=None, param_groups=None, decoupled_weight_decay=False):
        _check_atan2_ab(a, b)
        self.a, self.b = a, b
        super().__init__(model, lr=lr, betas=betas, weight_decay=weight_decay, max_grad_norm=max_grad_norm, process_group=process_group,
                         average_grads=average_grads, muon_params=muon_params, muon_lr=muon_lr, muon_weight_decay=muon_weight_decay, momentum=momentum,
                         nesterov=nesterov, ns_coefficients=ns_coefficients, ns_steps=ns_steps, muon_eps=muon_eps, adjust_lr_fn=adjust_lr_fn,
                         param_groups=param_groups, decoupled_weight_decay=decoupled_weight_decay)
