"""Launch lists of real Plans built on the CPU, and a canonical digest of them.

`cpu_plan` is the one CPU plan builder of the suite (nothing is launched: the lists, their order and their argument structs are the product's own).
`digest(plan)` reduces every launch list of a plan to (item count, entry-point names, sha256 of the canonical items): two builds of the same plan give
the same digest whatever addresses their buffers got, and a change of one argument byte changes it.  `CASES` is the fixed matrix of plans whose digests
`tests/plan_digests.json` records (written by this file's `__main__`, compared by tests/test_plan_lists_cpu.py).

Names of the package this file relies on: the `Plan(...)` signature and its public setters, the list attributes `fwd`, `vel`, `rec`, `bwd`, `clean_bwd`,
`ar_tail`, `tap0`, `plan._src_tab`, `plan.tn_tables`, `capi.STRUCTS`, `capi.FUNCTIONS`, `engine.Side`."""
import bisect
import contextlib
import ctypes
import gc
import hashlib
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from transfusion_pytorch_amd import capi  # noqa: E402

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plan_digests.json')
LISTS = ('fwd', 'vel', 'rec', 'bwd', 'clean_bwd', 'ar_tail', 'tap0')
STATE = ('fwd_cond', 'fwd_embed_end', 'fwd_logits_end', 'fwd_pred_end', 'tap_final', 'bwd_end', 'bwd_cuts', 'tn_run', 'n_slots', 'pull', 'side', 'nbytes')
ENV = ('TFX_SIDE_STREAM', 'TFX_TN_DEFER', 'TFX_TN_GROUP', 'TFX_ATTN_QKNR', 'TFX_DECODE_PREFETCH', 'TFX_SC_PLAN')       # switches the builder reads
# positional entry points whose arguments are HOST pointers to args structs
NESTED = {'tfx_adaln_post_pre_fwd': ('tfx_adaln_post_args', 'tfx_adaln_pre_args'),
          'tfx_layer_end_fwd': ('tfx_adaln_post_args', 'tfx_attnres_args', 'tfx_adaln_pre_args'),
          'tfx_attnres_pull_bwd': ('tfx_attnres_pull_args', 'tfx_adaln_post_args'),
          'tfx_adaln_pre_post_bwd': ('tfx_adaln_pre_args', 'tfx_adaln_post_args')}
TN = 'tfx_gemm_tn_args'


# ---------------------------------------------------------------------------------------------------- the CPU plan
class _Shadows(dict):
    """stand-in for the bf16 kernel-layout copies: only addresses enter the lists, and offsets such as S['skip_t3'][d:] land inside the stand-in"""

    def __missing__(self, k):
        self[k] = torch.zeros(1 << 16, dtype=torch.bfloat16)
        return self[k]


def cpu_plan(depth=5, transformer=None, model=None, cache=None, **plan_kw):
    """(model, store, plan): a real Plan built on the CPU with stand-in `ps.grad` and `ps.shadows`.  `transformer` / `model`: extra keyword arguments of
    the Transformer / of Transfusion; `cache=(maxlen,)`: a KV cache [depth, b, maxlen, 2 hdk]; the rest goes to Plan (b, n, I, R have defaults)."""
    from transfusion_pytorch_amd import Transfusion
    from transfusion_pytorch_amd.engine import Plan
    from transfusion_pytorch_amd.params import geglu_phys_to_ref_rows, head_phys_to_ref_rows
    torch.manual_seed(0)
    m = Transfusion(num_text_tokens=16, dim_latent=(32, 8), transformer=dict(dict(dim=64, depth=depth, heads=1), **(transformer or {})), **(model or {}))
    ps, md = m.store, m.md
    ps.grad = torch.zeros(ps.numel)
    ps.shadows = _Shadows()
    ps._map('geglu', geglu_phys_to_ref_rows(md.di, md.dip))
    if md.dim_head != 64:
        ps._map('heads', head_phys_to_ref_rows(md.heads, md.dim_head, md.gates))
    kw = dict(b=2, n=64, I=4, R={0: 8, 1: 4})
    kw.update(plan_kw)
    if cache is not None:
        kw['cache'] = torch.zeros(md.depth, kw['b'], cache[0], 2 * md.hdk, dtype=torch.bfloat16)
    return m, ps, Plan(ps, **kw)


# ---------------------------------------------------------------------------------------------------- the digest
def nested_structs(item):
    """the args structs a positional launch passes by address (the fused token-wise launches), read where they live"""
    fn, a = item
    name = fn if isinstance(fn, str) else fn.__name__
    if name not in NESTED or not isinstance(a, (tuple, list)):
        return []
    return [capi.STRUCTS[s].from_address(v) for s, v in zip(NESTED[name], a) if v]


class _Digest:
    def __init__(self):
        # every live tensor storage: a device / tensor pointer of a list must point into one of them
        seen = set()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                  # (isinstance on a deprecated alias object of torch warns)
            tensors = [t for t in gc.get_objects() if isinstance(t, torch.Tensor)]
        for t in tensors:
            try:
                st = t.untyped_storage()
                if st.nbytes():
                    seen.add((st.data_ptr(), st.nbytes()))
            except Exception:
                pass
        self.allocs = sorted(seen)
        self.ids = {}

    def ptr(self, p, where):
        if not p:
            return 0
        k = bisect.bisect_right(self.allocs, (p, 1 << 62)) - 1
        if k >= 0 and self.allocs[k][0] <= p < self.allocs[k][0] + self.allocs[k][1]:
            base, n = self.allocs[k]
            return ('mem', self.ids.setdefault(base, len(self.ids)), n, p - base)
        raise AssertionError(f'{where}: pointer {p:#x} is inside no live tensor storage')

    def struct(self, a, name, where):
        out = []
        for f in a._fields_:
            nm, ty = f[0], f[1]
            v = getattr(a, nm)
            if ty is ctypes.c_void_p:
                if name == TN and nm == 'group_next' and v:
                    v = self.struct(capi.STRUCTS[TN].from_address(v), TN, where + '>group')
                elif name == TN and nm == 'table_host' and v:
                    n, rs = a.table_count, ctypes.sizeof(capi.STRUCTS[TN])
                    v = ([self.struct(capi.STRUCTS[TN].from_address(v + k * rs), TN, f'{where}>table[{k}]') for k in range(n)],
                         list((ctypes.c_int32 * n).from_address(v + n * rs)))
                else:
                    v = self.ptr(v, f'{where}.{nm}')
            elif isinstance(v, ctypes.Array):
                v = tuple(v)
            out.append((nm, v))
        return out

    def item(self, it, where):
        from transfusion_pytorch_amd.engine import Side
        fn, a = it
        nm = fn if isinstance(fn, str) else fn.__name__
        where = f'{where} {nm}'
        side = isinstance(it, Side)
        flops = getattr(a, '_algo_flops', None)
        if isinstance(a, ctypes.Structure):
            return (side, nm, self.struct(a, type(a).__name__, where), flops)
        if isinstance(a, (tuple, list)):
            argt = capi.FUNCTIONS[nm][1][:-1]
            assert len(argt) == len(a), where
            vals = []
            for k, (ty, v) in enumerate(zip(argt, a)):
                if ty is ctypes.c_void_p and v and nm in NESTED:
                    vals.append(self.struct(capi.STRUCTS[NESTED[nm][k]].from_address(v), NESTED[nm][k], f'{where}[{k}]'))
                elif ty is ctypes.c_void_p:
                    vals.append(self.ptr(v, f'{where}[{k}]'))
                elif ty is ctypes.c_float:
                    vals.append(float(v))
                else:
                    vals.append(int(v))
            return (side, nm, vals, flops)
        return (side, nm, a, flops)                            # fork / join: the event slot


def _sha(x):
    return hashlib.sha256(repr(x).encode()).hexdigest()


def digest(plan):
    """{'lists': {name: [items, [entry-point names], sha256] | None}, 'src_tab': sha256 | None, 'state': {...}} - plain JSON values"""
    D = _Digest()
    lists = {}
    for name in LISTS:
        L = getattr(plan, name, None)
        if L is None:
            lists[name] = None
            continue
        items = [D.item(it, f'{name}[{k}]') for k, it in enumerate(L)]
        lists[name] = [len(items), [it[1] for it in items], _sha(items)]
    src = None
    if getattr(plan, '_src_tab', None) is not None:
        SRC = capi.STRUCTS['tfx_attnres_src']
        raw = bytes(plan._src_tab.cpu().numpy().tobytes())
        recs = (SRC * (len(raw) // ctypes.sizeof(SRC))).from_buffer_copy(raw)
        src = _sha([D.struct(r, 'tfx_attnres_src', f'_src_tab[{j}]') for j, r in enumerate(recs)])
    state = {k: getattr(plan, k, None) for k in STATE}
    state['meta'] = {k: sorted([i, *v] for i, v in (getattr(getattr(plan, k, None), 'meta', None) or {}).items()) for k in ('fwd', 'bwd')}
    state['tn_tables'] = [[e[0], e[1], e[2], e[4]] for e in getattr(plan, 'tn_tables', None) or []]
    trains = plan.cache is None and len(plan.bwd) > 0
    state['recompute'] = [plan.recompute_range(i) for i in range(plan.md.depth)] if trains else None
    return json.loads(json.dumps({'lists': lists, 'src_tab': src, 'state': state}))


# ---------------------------------------------------------------------------------------------------- the case matrix
# a case is a generator of (stage, plan): the plan is digested at every stage, with everything the case holds still alive
def _one(**kw):
    def case():
        m, ps, plan = cpu_plan(**kw)
        yield 'built', plan
    return case


def _frozen(pick, lora_rank=0, **kw):
    def case():
        m, ps, plan = cpu_plan(**kw)
        key = ()
        if lora_rank:
            from transfusion_pytorch_amd import lora
            lora.add_lora_(m, rank=lora_rank)
            key = ps.lora.key()
            fz = frozenset(n for n, p in ps.params.items() if not p.requires_grad)
        else:
            fz = frozenset(n for n in ps.params if pick(n))
        plan.select_frozen(fz, key)
        yield 'frozen', plan
    return case


def below_heads(n):
    return n.startswith(('transformer.', 'text_embed', 'latent_to_model'))


def lower_half(n):
    """layers 0-1, the embeddings, latent_to_model, the time conditioning and the AdaLN weights: the backward ends at layer 2, whose `.3.` parameters train"""
    return (n.startswith(('transformer.layers.0.', 'transformer.layers.1.', 'text_embed', 'latent_to_model')) or 'to_time_cond' in n
            or '.to_film.' in n or '.to_ada_ln_zero.' in n)


def to_v_and_net0(n):
    return '.to_v.' in n or n.endswith('net.0.weight')


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def _setters():
    m, ps, plan = cpu_plan()
    rope = [(torch.ones(64, 32), torch.zeros(64, 32)), (torch.zeros(80, 32), torch.ones(80, 32))]
    eps = {t: torch.zeros(r, m.md.dim_latents[t]) for t, r in plan.R.items()}
    plan.set_segments(_i32(0, 64), _i32(64, 64))
    plan.set_rope_tables(*rope[0])
    plan.set_rows({0: 5, 1: 3})
    plan.set_loss_scales(0.5, {0: 0.25, 1: 0.125})
    plan.set_ce_vocab(12)
    for t, e in eps.items():
        plan.set_noise(t, e.data_ptr())
    yield 'set', plan
    new = frozenset(n for n in ps.params if to_v_and_net0(n))
    plan.select_frozen(new)
    yield 'new set', plan                                  # the list just built carries the tables, the segment count and the row counts of the step
    plan.select_frozen(frozenset(n for n in ps.params if lower_half(n)))
    yield 'second set', plan
    # the setters reach every kept list, whichever is current
    plan.set_segments(_i32(0, 32, 96), _i32(32, 64, 32))
    plan.set_rope_tables(*rope[1])
    plan.set_rows({0: 6, 1: 2})
    yield 'second set, set again', plan
    plan.select_frozen(new)
    yield 'new set, back', plan
    plan.select_frozen(frozenset())
    yield 'nothing frozen, back', plan


def _clean_setters():
    m, ps, plan = cpu_plan(model=dict(model_output_clean=True))
    eps = {t: torch.zeros(r, m.md.dim_latents[t]) for t, r in plan.R.items()}
    for t, e in eps.items():
        plan.set_noise(t, e.data_ptr())
    plan.set_rows({0: 5, 1: 3})
    yield 'latent by default', plan
    plan.set_clean_mode('model')
    yield 'model', plan
    plan.set_clean_mode('latent')
    yield 'latent', plan


def _taps():
    m, ps, plan = cpu_plan()
    D = m.md.depth
    g = torch.zeros(2, 64, 64, dtype=torch.bfloat16)
    plan.set_taps({0: g.float(), 3: g, D + 1: g}, 64)
    yield 'taps', plan
    plan.clear_taps()
    yield 'cleared', plan


def _ext_types():
    from torch import nn
    return dict(pre_post_transformer_enc_dec=(None, (nn.Linear(8, 64), nn.Linear(64, 8))))


CASES = {
    # training plans: name -> (environment, case)
    'plain': ({}, _one()),
    'one stream': ({'TFX_SIDE_STREAM': '0'}, _one()),
    'ckpt': ({}, _one(ckpt=True)),
    'ckpt, one stream': ({'TFX_SIDE_STREAM': '0'}, _one(ckpt=True)),
    'dp_groups 3': ({}, _one(dp_groups=3)),
    'tn_defer 2, dp_groups 3': ({}, _one(tn_defer=2, dp_groups=3)),
    'tn_defer all': ({}, _one(tn_defer='all')),
    'TFX_TN_GROUP 0': ({'TFX_TN_GROUP': '0'}, _one()),
    'TFX_ATTN_QKNR 0': ({'TFX_ATTN_QKNR': '0'}, _one()),
    'text only': ({}, _one(I=0, R={})),
    'depth 33 (push form)': ({}, _one(depth=33)),
    # model variants
    'no qk_rmsnorm': ({}, _one(transformer=dict(qk_rmsnorm=False))),
    'no gates': ({}, _one(transformer=dict(attn_kwargs=dict(gate_values=False)))),
    'laser': ({}, _one(transformer=dict(attn_laser=True))),
    'clean': ({}, _one(model=dict(model_output_clean=True))),
    'dim_head 32, heads 2': ({}, _one(transformer=dict(dim_head=32, heads=2))),
    'enc_dec type': ({}, lambda: _one(model=_ext_types())()),
    'add_pos_emb': ({}, _one(model=dict(add_pos_emb=True, modality_num_dim=1))),
    # frozen sets
    'frozen below the heads': ({}, _frozen(below_heads)),
    'frozen lower half': ({}, _frozen(lower_half)),
    'frozen to_v, net.0.weight': ({}, _frozen(to_v_and_net0)),
    'clean, model_to_latent frozen': ({}, _frozen(lambda n: n.startswith('model_to_latent'), model=dict(model_output_clean=True))),
    'lora rank 4': ({}, _frozen(None, lora_rank=4)),
    'ckpt, frozen lower half': ({}, _frozen(lower_half, ckpt=True)),
    # inference plans
    'inference': ({}, _one(training=False)),
    'decode': ({}, _one(training=False, cache=(96,), n=4)),
    'decode, laser': ({}, _one(training=False, cache=(96,), n=1, transformer=dict(attn_laser=True))),
    'compacted decode': ({}, _one(training=False, cache=(96,), n=4, tile_attn=True, units=(2, 8), ctl_rows=9, R={0: 4, 1: 4})),
    # state after the setters, hidden taps
    'setters': ({}, _setters),
    'clean, setters': ({}, _clean_setters),
    'taps': ({}, _taps),
}


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def run_case(name):
    """{stage: digest} of one case"""
    env, case = CASES[name]
    with _environment(env):
        out = {stage: digest(plan) for stage, plan in case()}
    gc.collect()
    return out


if __name__ == '__main__':
    with open(JSON_PATH, 'w') as f:
        json.dump({name: run_case(name) for name in CASES}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', JSON_PATH)
