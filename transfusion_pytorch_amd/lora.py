"""LoRA adapters on the attention and feed-forward matrices of a native Transfusion.

    add_lora_(model, rank=16)                      # freezes the base, attaches A [r, d_in] / B [d_out, r] pairs
    opt = FusedAdam(model, lr=1e-4)                # steps them as external parameters
    ...
    merge_lora_(model)                             # W <- W + s B A in the fp32 masters, adapters gone

An adapted nn.Linear weight reads W_eff = W + s B A, s = (alpha or rank) / rank; biases are untouched.

* Forward, data gradients and every inference path run their unchanged launch lists: `ParamStore.refresh_shadows` casts the bf16 shadows of an adapted
  matrix from an fp32 scratch that `tfx_lora_merge` fills with W_eff (for to_qk / to_v: the fused [q | k | v | gates] block) - an fp32 master rounded once,
  the numerics of full fine-tuning.  `merge_lora_` copies the same scratch into the masters: logits before and after are bit-identical.
* Adapter gradients are new launches of the backward list (engine.Plan._lora_launches): U = X A^T, dU = dY B (`tfx_lora_down`), dB^T = s U^T dY,
  dA = s dU^T X (`tfx_lora_grad`), on the operands the matrix's weight-gradient product reads, in the kernels' physical layouts; the small operand
  matrices A_phys / B^T_phys are rebuilt with the maps of params.py on every shadow refresh, and the gradient stores map back to the parameter's order.
* The adapters are nn.Parameters of the model under `lora.<module path>.A` / `.B` (state_dict, load_state_dict, parameters()); the trainable ones join
  `external_parameters()`, so the fused optimizers step, clip and exchange them by their route for external parameters.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch
from torch import nn

from . import capi
from .params import _Holder, geglu_phys_to_ref_rows, head_phys_to_ref_rows

TARGETS = ('to_qk', 'to_v', 'to_out', 'net.0', 'net.3')
_MODULE = {'to_qk': '1.fn.to_qk.0', 'to_v': '1.fn.to_v.0', 'to_out': '1.fn.to_out.1', 'net.0': '2.fn.net.0', 'net.3': '2.fn.net.3'}
# matrices that take no adapter (a clear error instead of a silent no-op)
_REFUSED = ('to_gates', 'to_text_logits', 'text_embed', 'to_film', 'to_ada_ln_zero', 'to_time_cond', 'latent_to_model_projs', 'model_to_latent_projs', 'skip', '0')
MAX_RANK = 64
_uid = itertools.count(1)


def r_pad_of(rank: int) -> int:
    return 32 if rank <= 32 else 64


class Adapter:
    """one (A, B) pair and what the kernels need of it"""

    def __init__(self, md, layer: int, target: str, rank: int, scale: float, device):
        d, hd, hdk, di, dip = md.dim, md.hd, md.hdk, md.di, md.dip
        self.layer, self.target, self.r, self.r_pad, self.s = layer, target, rank, r_pad_of(rank), float(scale)
        self.path = f'transformer.layers.{layer}.{_MODULE[target]}'
        self.weight = self.path + '.weight'
        heads = head_phys_to_ref_rows(md.heads, md.dim_head, md.gates)
        pad64 = md.dim_head != 64
        # (d_in, d_out, physical K of X, physical N of dY, physical K column -> column of A, physical N column -> row of B); None = identity
        if target == 'to_qk':
            geo = (d, 2 * hd, d, 2 * hdk, None, heads[:2 * hdk] if pad64 else None)
        elif target == 'to_v':
            v = heads[2 * hdk:3 * hdk]
            geo = (d, hd, d, hdk, None, np.where(v >= 0, v - 2 * hd, -1) if pad64 else None)
        elif target == 'to_out':
            geo = (hd, d, hdk, d, heads[:hdk] if pad64 else None, None)
        elif target == 'net.0':
            geo = (d, 2 * di, d, 2 * dip, None, geglu_phys_to_ref_rows(di, dip))
        else:
            geo = (di, d, dip, d, np.where(np.arange(dip) < di, np.arange(dip), -1) if di != dip else None, None)
        self.d_in, self.d_out, self.k_phys, self.n_phys, self._in_map, self._out_map = geo
        A = torch.empty(rank, self.d_in, device=device)
        nn.init.kaiming_uniform_(A, a=5 ** 0.5)                   # as nn.Linear initialises its weight
        self.A = nn.Parameter(A)
        self.B = nn.Parameter(torch.zeros(self.d_out, rank, device=device))
        self.allocate(device)

    @property
    def trainable(self):
        return self.A.requires_grad or self.B.requires_grad

    def allocate(self, device):
        """the device buffers the launch lists hold pointers to: the persistent fp32 gradients, the bf16 operands, the fp32 W_eff scratch"""
        self.uid = next(_uid)
        self.device = device
        self.gA = self.gB = None                                   # views of the set's flat gradient buffer (LoraSet.allocate_grads)
        self.A_phys = torch.zeros(self.r_pad, self.k_phys, device=device, dtype=torch.bfloat16)
        self.BT_phys = torch.zeros(self.r_pad, self.n_phys, device=device, dtype=torch.bfloat16)
        self.scratch = None if self.target in ('to_qk', 'to_v') else torch.empty(self.d_out, self.d_in, device=device)
        def dev_map(m):
            if m is None:
                return None, None, None
            m = np.ascontiguousarray(m, dtype=np.int32)
            pos = np.nonzero(m >= 0)[0]
            return (torch.from_numpy(m).to(device), torch.from_numpy(pos.astype(np.int64)).to(device), torch.from_numpy(m[pos].astype(np.int64)).to(device))
        self.in_map, self._in_pos, self._in_ref = dev_map(self._in_map)
        self.out_map, self._out_pos, self._out_ref = dev_map(self._out_map)
        self.A.grad = self.B.grad = None

    @torch.no_grad()
    def build_operands(self):
        """A_phys [r_pad, K_phys] and B^T_phys [r_pad, N_phys] in bf16: the adapter in the physical layout of the matrix it belongs to (head padding, GEGLU
        row order, the di -> dip padding); rows past the rank and padding columns stay zero"""
        r = self.r
        if self.in_map is None:
            self.A_phys[:r].copy_(self.A)
        else:
            self.A_phys[:r].index_copy_(1, self._in_pos, self.A.index_select(1, self._in_ref).to(torch.bfloat16))
        if self.out_map is None:
            self.BT_phys[:r].copy_(self.B.t())
        else:
            self.BT_phys[:r].index_copy_(1, self._out_pos, self.B.index_select(0, self._out_ref).t().to(torch.bfloat16))

    def grad_pairs(self):
        return ((self.A, self.gA), (self.B, self.gB))


class LoraSet:
    """the adapters of one model, kept by its ParamStore (`store.lora`)"""

    def __init__(self, md):
        self.md = md
        self.adapters = {}              # path -> Adapter, in (layer, target) order
        self.fused = {}                 # layer -> fp32 scratch of the fused [q | k | v | gates] block
        self.epoch = next(_uid)

    def __bool__(self):
        return bool(self.adapters)

    def get(self, layer, target):
        return self.adapters.get(f'transformer.layers.{layer}.{_MODULE[target]}')

    def sort(self):
        self.adapters = dict(sorted(self.adapters.items(), key=lambda kv: (kv[1].layer, TARGETS.index(kv[1].target))))
        self.epoch = next(_uid)
        self.allocate_grads()

    def allocate_grads(self):
        """the persistent fp32 gradients of every adapter as views of ONE buffer (a fresh accumulation is one fill, as for the native gradients); the
        launch lists hold their addresses, so every adapter gets a new uid"""
        ads = list(self.adapters.values())
        if not ads:
            return
        sizes = [n for a in ads for n in (a.r * a.d_in, a.d_out * a.r)]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + (n + 3) // 4 * 4)                # 16-byte aligned views
        self.gflat = torch.zeros(offs[-1], device=ads[0].device)
        for k, a in enumerate(ads):
            a.gA = self.gflat[offs[2 * k]:offs[2 * k] + a.r * a.d_in].view(a.r, a.d_in)
            a.gB = self.gflat[offs[2 * k + 1]:offs[2 * k + 1] + a.d_out * a.r].view(a.d_out, a.r)
            a.uid = next(_uid)
            a.A.grad = a.B.grad = None

    def parameters(self):
        return [p for a in self.adapters.values() for p in (a.A, a.B)]

    def version(self):
        return sum(a.A._version + a.B._version for a in self.adapters.values()) + (self.epoch << 20)

    def key(self):
        """what a backward list depends on: which adapters train, and the buffers their launches point at"""
        return tuple((a.path, a.uid, a.A.requires_grad, a.B.requires_grad) for a in self.adapters.values() if a.trainable)

    def trainable_layers(self):
        return [a.layer for a in self.adapters.values() if a.trainable]

    def to(self, device):
        """after the model moved: the parameters were moved by nn.Module._apply, the device buffers are made again"""
        self.fused = {}
        for a in self.adapters.values():
            a.allocate(device)
        self.epoch = next(_uid)
        self.allocate_grads()

    def _merge(self, stream, W, ldw, out, ldo, N, K, a):
        kw = dict(W=W, ldw=ldw, Weff=out, ldo=ldo, N=N, K=K, r=0, s=0.)
        if a is not None:
            A, B = a.A.data, a.B.data
            assert A.is_contiguous() and B.is_contiguous() and A.dtype == B.dtype == torch.float32
            kw.update(A=A, lda=K, B=B, ldb=a.r, r=a.r, s=a.s)
        capi.call('tfx_lora_merge', capi.make_args('tfx_lora_merge_args', **kw), stream)

    def merged_sources(self, ps, stream):
        """fill the W_eff scratches (tfx_lora_merge) and return {weight name: device address the shadow casts read instead of the master}.  The fused
        projection's entry stands under its first member, to_qk - where refresh_shadows takes the block's base address"""
        md = self.md
        d, hd = md.dim, md.hd
        src = {}
        for layer in sorted({a.layer for a in self.adapters.values() if a.scratch is None}):
            buf = self.fused.get(layer)
            if buf is None or buf.device != ps.flat.device:
                buf = self.fused[layer] = torch.empty(md.nq, d, device=ps.flat.device)
            base = f'transformer.layers.{layer}.1.fn.to_qk.0.weight'
            for r0, r1, a in ((0, 2 * hd, self.get(layer, 'to_qk')), (2 * hd, 3 * hd, self.get(layer, 'to_v')), (3 * hd, md.nq, None)):
                if r1 > r0:
                    self._merge(stream, ps.ptr(base, r0 * d), d, buf.data_ptr() + 4 * r0 * d, d, r1 - r0, d, a)
            src[base] = buf.data_ptr()
        for a in self.adapters.values():
            if a.scratch is not None:
                self._merge(stream, ps.ptr(a.weight), a.d_in, a.scratch.data_ptr(), a.d_in, a.d_out, a.d_in, a)
                src[a.weight] = a.scratch.data_ptr()
        return src

    def build_operands(self):
        for a in self.adapters.values():
            a.build_operands()

    def ensure_grads(self):
        """`.grad` of a trainable A / B is a view of its persistent buffer, zeroed when the gradient was None (a fresh accumulation); a frozen one has None"""
        pairs = [pg for a in self.adapters.values() for pg in a.grad_pairs()]
        fresh = [(p, g) for p, g in pairs if p.requires_grad and (p.grad is None or p.grad.data_ptr() != g.data_ptr())]
        if len(fresh) == sum(1 for p, _ in pairs if p.requires_grad):
            self.gflat.zero_()                                      # every trainable adapter starts over: one fill
        else:
            for _, g in fresh:
                g.zero_()
        for p, g in pairs:
            if not p.requires_grad:
                p.grad = None
        for p, g in fresh:
            p.grad = g


# ---------------------------------------------------------------------------------------------------- public surface
def _store(model):
    return model.store


def has_lora(model) -> bool:
    return bool(getattr(getattr(model, 'store', None), 'lora', None))


def require_no_lora(model, what: str):
    """the combinations that are not built: refuse them while adapters are attached"""
    if has_lora(model):
        raise NotImplementedError(f'{what} on a model with LoRA adapters attached is not supported: call merge_lora_(model) (or remove_lora_) first')


def _register(model, a: Adapter):
    m = model
    parts = ('lora.' + a.path).split('.')
    for i, part in enumerate(parts):
        nxt_is_index = i + 1 < len(parts) and parts[i + 1].isdigit()
        if part.isdigit():
            idx = int(part)
            while len(m) <= idx:
                m.append(None)
            if m[idx] is None:
                m[idx] = nn.ModuleList() if nxt_is_index else _Holder()
            m = m[idx]
        else:
            if not hasattr(m, part):
                setattr(m, part, nn.ModuleList() if nxt_is_index else _Holder())
            m = getattr(m, part)
    m.register_parameter('A', a.A)
    m.register_parameter('B', a.B)


def add_lora_(model, rank=16, alpha=None, targets=TARGETS, layers=None, freeze_base=True):
    """attach one adapter pair per (layer, target); returns the model.  A [rank, d_in] fp32 initialised as nn.Linear initialises its weight, B [d_out, rank]
    zeros, W_eff = W + (alpha or rank) / rank * B A.  `freeze_base`: requires_grad_(False) on every native parameter (switch some back on afterwards if
    wanted: an adapted matrix whose base also trains gets both gradients, taken at W_eff)."""
    ps, md = _store(model), model.md
    if not isinstance(rank, int) or isinstance(rank, bool) or not 1 <= rank <= MAX_RANK:
        raise ValueError(f'rank must be an integer in 1 .. {MAX_RANK}, got {rank!r}')
    targets = (targets,) if isinstance(targets, str) else tuple(targets)
    for t in targets:
        if t not in TARGETS:
            if any(t == n or t.startswith(n + '.') or t.endswith('.' + n) for n in _REFUSED):
                raise NotImplementedError(f'no LoRA adapters on {t!r}: only {TARGETS} take them (to_gates, the heads, the embeddings, the AdaLN tables and '
                                          'the skip projections are not built)')
            raise ValueError(f'unknown LoRA target {t!r}: one of {TARGETS}')
    layers = tuple(range(md.depth)) if layers is None else tuple(layers)
    for i in layers:
        if not isinstance(i, int) or not 0 <= i < md.depth:
            raise ValueError(f'layer {i!r} out of range: the model has layers 0 .. {md.depth - 1}')
    if len(set(layers)) != len(layers) or len(set(targets)) != len(targets):
        raise ValueError('a layer or target is named twice')
    cur = ps.lora if getattr(ps, 'lora', None) is not None else LoraSet(md)
    new = [(i, t) for i in layers for t in targets]
    for i, t in new:
        if cur.get(i, t) is not None:
            raise ValueError(f'transformer.layers.{i}.{_MODULE[t]} already has an adapter')
    scale = (alpha if alpha else rank) / rank
    for i, t in new:
        a = Adapter(md, i, t, rank, scale, ps.flat.device)
        cur.adapters[a.path] = a
    cur.sort()
    # registration in (layer, target) order, whatever the order of the calls: drop and re-register
    if hasattr(model, 'lora'):
        del model.lora
    for a in cur.adapters.values():
        _register(model, a)
    ps.lora = cur
    if freeze_base:
        for p in ps.params.values():
            p.requires_grad_(False)
    ps.mark_dirty()
    return model


def lora_parameters(model):
    """the adapter parameters in a stable order: by layer, then by target in the order of `TARGETS`, A before B"""
    return _store(model).lora.parameters() if has_lora(model) else []


def _detach(model):
    ps = _store(model)
    ps.lora = None
    if hasattr(model, 'lora'):
        del model.lora
    ps.mark_dirty()


@torch.no_grad()
def merge_lora_(model):
    """write W_eff into the fp32 master weights - the bits the shadows were cast from - and remove the adapters"""
    if not has_lora(model):
        return model
    ps = _store(model)
    ls, md = ps.lora, model.md
    if ps.flat.device.type != 'cuda':
        raise capi.TfxError('merge_lora_ runs tfx_lora_merge on the GPU: move the model there first (model.cuda())')
    src = ls.merged_sources(ps, model._stream())
    hd, d = md.hd, md.dim
    for a in ls.adapters.values():
        if a.scratch is not None:
            ps.params[a.weight].copy_(a.scratch)
        else:
            r0 = 0 if a.target == 'to_qk' else 2 * hd
            ps.params[a.weight].copy_(ls.fused[a.layer][r0:r0 + a.d_out])
    del src
    _detach(model)
    return model


def remove_lora_(model):
    """drop the adapters without merging: the model is the base model again"""
    if has_lora(model):
        _detach(model)
    return model
