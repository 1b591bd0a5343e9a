"""Chunked text head (Transfusion.set_text_head_chunking_, engine.Plan `chunk_rows`, tfx_ce_fwd / tfx_ce_bwd): what can be checked without a GPU - the switch,
the plan key, the C ABI tables, the launch lists of real chunked Plans built on the CPU (nothing is launched), and the float64 restatement the GPU tests
hold the kernels to against torch's own cross entropy."""
import copy
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _text_head_cases as C                                         # noqa: E402


def _model(depth=2):
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(0)
    return Transfusion(num_text_tokens=16, dim_latent=(32, 8), transformer=dict(dim=64, depth=depth, heads=1))


def _name(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


# ================================================================================================ the switch
def test_default_is_off_and_the_setter_validates():
    m = _model()
    assert m.text_head_chunk_rows is None
    assert m.set_text_head_chunking_(64) is m and m.text_head_chunk_rows == 64
    assert m.set_text_head_chunking_(16384).text_head_chunk_rows == 16384
    for bad in (0, -64, 1, 63, 65, 100, 4095):
        with pytest.raises(ValueError):
            m.set_text_head_chunking_(bad)
    for bad in (64.0, '64', True, False, (64,), [64]):
        with pytest.raises(TypeError):
            m.set_text_head_chunking_(bad)
    assert m.text_head_chunk_rows == 16384                              # a refused call changes nothing
    assert m.set_text_head_chunking_(None) is m and m.text_head_chunk_rows is None
    with pytest.raises(AttributeError):
        m.text_head_chunk_rows = 64                                     # read-only


def test_copies_carry_the_switch():
    m = _model().set_text_head_chunking_(128)
    assert copy.deepcopy(m).text_head_chunk_rows == 128
    assert m._clone_architecture().text_head_chunk_rows == 128
    assert copy.deepcopy(_model()).text_head_chunk_rows is None


def test_plan_key_carries_the_switch_for_text_loss_training_plans_only(monkeypatch):
    """`_plan` with the Plan class stubbed out: a text-loss training plan of each setting has a key of its own; inference plans and training plans of calls
    without a text loss (forward_modality) do not depend on the switch - and with the switch off Plan is called exactly as before (no new keyword)"""
    from transfusion_pytorch_amd import transfusion as T
    made = []

    class Stub:
        nbytes = 1

        def __init__(self, store, b, n, I, R, training=True, dp_groups=0, ckpt=False, **kw):
            self.training, self.kw = training, kw
            made.append(self)

        def select_frozen(self, *a):
            pass
    monkeypatch.setattr(T, 'Plan', Stub)
    monkeypatch.setenv('TFX_PLAN_BUDGET_GB', '1')
    m = _model()
    p_plain = m._plan(2, 64, 0, {}, True, text_loss=True)
    i_plain = m._plan(2, 64, 0, {}, False, text_loss=True)
    f_plain = m._plan(2, 64, 2, {0: 128}, True)
    assert all(p.kw == {} for p in made)
    m.set_text_head_chunking_(64)
    p64 = m._plan(2, 64, 0, {}, True, text_loss=True)
    assert p64 is not p_plain and p64.kw == {'chunk_rows': 64}
    assert m._plan(2, 64, 0, {}, False, text_loss=True) is i_plain    # inference: the switch is not looked at
    assert m._plan(2, 64, 2, {0: 128}, True) is f_plain               # a training plan without a text loss neither
    m.set_text_head_chunking_(128)
    p128 = m._plan(2, 64, 0, {}, True, text_loss=True)
    assert p128 is not p64 and p128.kw == {'chunk_rows': 128}
    assert len(m._plans) == 5 and len(made) == 5
    m.set_text_head_chunking_(None)
    assert m._plan(2, 64, 0, {}, True, text_loss=True) is p_plain and len(made) == 5


# ================================================================================================ the C ABI tables
def test_capi_tables_match_the_header():
    from transfusion_pytorch_amd import capi
    src = capi._strip_comments(open(capi.HEADER).read())
    body = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*tfx_ce_chunk_args\s*;', src).group(1)
    names = [re.sub(r'[\s*]', '', d) for decl in body.split(';') if decl.strip() for d in re.sub(r'^\s*(const\s+)?\w+', '', decl.strip()).split(',')]
    assert names == ['T', 'V', 'logits', 'ld', 'labels', 'lse', 'acc', 'grad_scale', 'scale_dev', 'dlogits', 'ld_d']
    f = capi.STRUCT_FIELDS['tfx_ce_chunk_args']
    assert [n for n, _ in f] == names
    ptrs = {'logits', 'labels', 'lse', 'acc', 'scale_dev', 'dlogits'}
    assert all((ty is ctypes.c_void_p) == (n in ptrs) for n, ty in f) and dict(f)['grad_scale'] is ctypes.c_float
    assert all(dict(f)[n] is ctypes.c_int32 for n in ('T', 'V', 'ld', 'ld_d'))
    for fn in ('tfx_ce_fwd', 'tfx_ce_bwd'):
        assert capi.FUNCTIONS[fn] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        assert 'TFX_OP_' + fn[4:].upper() in capi.ENUMS
    ops = [v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_')]
    assert len(ops) == len(set(ops)), 'two launch-list ops share a code'
    # the fused entry point and its struct are what they were
    assert [n for n, _ in capi.STRUCT_FIELDS['tfx_ce_args']] == ['T', 'V', 'logits', 'ld', 'labels', 'grad_scale', 'dlogits', 'ld_d', 'acc']
    assert capi.ENUMS['TFX_OP_CE_FWD_BWD'] == 18 and 'tfx_ce_fwd_bwd' in capi.FUNCTIONS


def test_library_exports_the_entry_points_and_refuses_bad_strides():
    """host logic only (no launch): NULL args, ld / ld_d that are no multiple of 8, V outside 1 .. ld, misaligned buffers return -1; T == 0 is a no-op"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    ok = dict(T=2, V=10, logits=base, ld=16, labels=base, lse=base, acc=base, grad_scale=1.0, scale_dev=None, dlogits=base, ld_d=16)
    for fn in (lib.tfx_ce_fwd, lib.tfx_ce_bwd):
        assert fn(None, None) == -1
        assert fn(ctypes.byref(capi.make_args('tfx_ce_chunk_args', **dict(ok, T=0))), None) == 0
        for bad in (dict(ld=12), dict(V=0), dict(V=17), dict(logits=base + 4), dict(T=-1), dict(logits=None), dict(labels=None), dict(lse=None)):
            assert fn(ctypes.byref(capi.make_args('tfx_ce_chunk_args', **dict(ok, **bad))), None) == -1, bad
    for bad in (dict(ld_d=12), dict(ld_d=8), dict(dlogits=base + 8), dict(dlogits=None)):
        assert lib.tfx_ce_bwd(ctypes.byref(capi.make_args('tfx_ce_chunk_args', **dict(ok, **bad))), None) == -1, bad
    assert lib.tfx_ce_fwd(ctypes.byref(capi.make_args('tfx_ce_chunk_args', **dict(ok, acc=None))), None) == -1


# ================================================================================================ chunked plans built on the CPU
def _cpu_plan(**kw):
    from _plan_digest import cpu_plan
    return cpu_plan(depth=2, **kw)


@pytest.mark.parametrize('rows,b', [(64, 3), (128, 3), (4096, 3)])
def test_chunked_plan_buffers_and_lists(rows, b, monkeypatch):
    """T = 192 rows: three chunks of 64 | 128 + a ragged 64 | one chunk (rows >= T).  The forward holds (logits product, tfx_ce_fwd) per chunk in front of
    the flow predictions, the backward (the same product, tfx_ce_bwd, the weight-gradient product, the d embed product) per chunk in front of everything
    else; every chunk's launches cover its own rows, and a backward product is the forward's argument for argument."""
    monkeypatch.delenv('TFX_SIDE_STREAM', raising=False)
    from transfusion_pytorch_amd.engine import Side
    m, ps, P = _cpu_plan(b=b, n=64, chunk_rows=rows)
    _, _, Q = _cpu_plan(b=b, n=64)
    md, T = m.md, b * 64
    R = min(rows, T)
    chunks = [(r0, min(R, T - r0)) for r0 in range(0, T, R)]
    assert P.chunk == R and Q.chunk is None
    assert not hasattr(P, 'logits') and not hasattr(P, 'dlogits')
    assert tuple(P.logits_c.shape) == (R, md.vp) and P.logits_c.dtype == torch.float32
    assert tuple(P.dlogits_c.shape) == (R, md.vp) and P.dlogits_c.dtype == torch.bfloat16
    assert tuple(P.ce_lse.shape) == (T,) and P.ce_lse.dtype == torch.float32
    assert P.nbytes == Q.nbytes - 6 * (T - R) * md.vp + 4 * T + 4
    # forward
    e0 = P.fwd_embed_end
    assert e0 == Q.fwd_embed_end and [_name(i) for i in P.fwd[:e0]] == [_name(i) for i in Q.fwd[:e0]]
    head = P.fwd[e0:P.fwd_logits_end]
    assert [_name(i) for i in head] == ['tfx_gemm_nt', 'tfx_ce_fwd'] * len(chunks)
    assert P.fwd_pred_end - P.fwd_logits_end == Q.fwd_pred_end - Q.fwd_logits_end
    assert [_name(i) for i in P.fwd[P.fwd_logits_end:]] == [_name(i) for i in Q.fwd[Q.fwd_logits_end:] if _name(i) != 'tfx_ce_fwd_bwd']
    q_nt = Q.fwd[e0][1]
    for k, (r0, rc) in enumerate(chunks):
        nt, ce = head[2 * k][1], head[2 * k + 1][1]
        assert (nt.M, nt.N, nt.K, nt.epi, nt.ldc) == (rc, q_nt.N, q_nt.K, q_nt.epi, q_nt.ldc) and nt.B == ps.shadows['logits'].data_ptr()
        assert nt.A == P.embed.data_ptr() + r0 * md.dim * 2 and nt.C == P.logits_c.data_ptr()
        assert (ce.T, ce.V, ce.ld, ce.ld_d) == (rc, md.vocab, md.vp, md.vp)
        assert ce.logits == P.logits_c.data_ptr() and ce.labels == P.labels.data_ptr() + 4 * r0 and ce.lse == P.ce_lse.data_ptr() + 4 * r0 and ce.acc == P.acc.data_ptr()
    assert all(k in P.fwd.meta for k in range(e0 + 1, P.fwd_logits_end, 2)), '_hbm accounting of the tfx_ce_fwd launches'
    # backward
    per = ['tfx_gemm_nt', 'tfx_ce_bwd', 'tfx_gemm_tn', 'tfx_gemm_nt']
    nb = len(per) * len(chunks)
    assert [_name(i) for i in P.bwd[:nb]] == per * len(chunks)
    assert not any(isinstance(i, Side) for i in P.bwd[:nb]), 'the chunk launches stay on the stream that writes dembed'
    assert 'tfx_ce_bwd' not in [_name(i) for i in P.bwd[nb:]]
    assert [_name(i) for i in P.bwd[nb:]] == [_name(i) for i in Q.bwd[2:]], 'behind the head the list is the plain plan\'s'
    for k, (r0, rc) in enumerate(chunks):
        nt, ce, tn, dx = (P.bwd[4 * k + j][1] for j in range(4))
        fnt = head[2 * k][1]
        assert bytes(nt) == bytes(fnt), 'the recompute is the forward\'s launch, argument for argument'
        assert (ce.T, ce.V, ce.ld, ce.ld_d) == (rc, md.vocab, md.vp, md.vp) and ce.lse == P.ce_lse.data_ptr() + 4 * r0 and ce.labels == P.labels.data_ptr() + 4 * r0
        assert ce.dlogits == P.dlogits_c.data_ptr() and ce.scale_dev == P.go_dev.data_ptr() and ce.logits == P.logits_c.data_ptr()
        assert (tn.M, tn.N, tn.K, tn.accumulate) == (rc, md.vocab, md.dim, 1) and tn.A == P.dlogits_c.data_ptr() and tn.B == P.embed.data_ptr() + r0 * md.dim * 2
        assert tn.C == ps.grad_ptr('to_text_logits.weight')
        assert (dx.M, dx.N, dx.K) == (rc, md.dim, md.vp) and dx.A == P.dlogits_c.data_ptr() and dx.C == P.dembed.data_ptr() + r0 * md.dim * 2
    assert all(4 * k + 1 in P.bwd.meta for k in range(len(chunks))), '_hbm accounting of the tfx_ce_bwd launches'
    assert P.bwd_cuts == Q.bwd_cuts == []
    # the per-step setters reach every chunk of both lists
    P.set_ce_vocab(11)
    P.set_loss_scales(0.25, {})
    ces = [i[1] for L in (P.fwd, P.bwd) for i in L if _name(i) in ('tfx_ce_fwd', 'tfx_ce_bwd')]
    assert len(ces) == 2 * len(chunks) and all(a.V == 11 and a.grad_scale == 0.25 for a in ces)


def test_chunked_plan_under_frozen_sets_checkpointing_and_exchange_groups():
    """text head frozen: no weight-gradient product in a chunk, the rest stays; the setters also reach the kept lists of other frozen sets; a checkpointed
    chunked plan keeps its recompute segments; the exchange cuts of a grouped backward are the plain plan's, behind the head"""
    m, ps, P = _cpu_plan(b=3, n=64, chunk_rows=64)
    full = [_name(i) for i in P.bwd]
    P.select_frozen(frozenset({'to_text_logits.weight'}))
    assert [_name(i) for i in P.bwd[:9]] == ['tfx_gemm_nt', 'tfx_ce_bwd', 'tfx_gemm_nt'] * 3
    assert [_name(i) for i in P.bwd].count('tfx_ce_bwd') == 3
    P.set_loss_scales(0.5, {})
    P.select_frozen(frozenset())
    assert [_name(i) for i in P.bwd] == full and all(i[1].grad_scale == 0.5 for i in P.bwd if _name(i) == 'tfx_ce_bwd')
    P.select_frozen(frozenset(ps.params))
    assert P.bwd_end == 0
    _, _, C2 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True)
    assert C2.ckpt and C2.chunk == 64 and [_name(i) for i in C2.bwd[:12]] == ['tfx_gemm_nt', 'tfx_ce_bwd', 'tfx_gemm_tn', 'tfx_gemm_nt'] * 3
    _, _, G = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2)
    _, _, H = _cpu_plan(b=3, n=64, dp_groups=2)
    assert [c[1:] for c in G.bwd_cuts] == [c[1:] for c in H.bwd_cuts] and G.bwd_cuts
    assert all(g[0] - h[0] == 12 - 2 for g, h in zip(G.bwd_cuts, H.bwd_cuts)), 'the head - 12 launches for 2 - is final before the first cut'


def test_switch_off_builds_the_plans_it_always_built():
    """Plan(...) without chunk_rows and with chunk_rows=None: the same lists, item for item (tests/test_plan_lists_cpu.py holds the digests)"""
    from _plan_digest import digest
    _, _, A = _cpu_plan(b=3, n=64)
    da = digest(A)
    _, _, B = _cpu_plan(b=3, n=64, chunk_rows=None)
    assert digest(B) == da and B.chunk is None and hasattr(B, 'logits') and hasattr(B, 'dlogits') and not hasattr(B, 'logits_c')
    _, _, I = _cpu_plan(b=3, n=64, chunk_rows=64, training=False)
    assert I.chunk is None and hasattr(I, 'logits'), 'an inference plan never chunks'


# ================================================================================================ the float64 restatement
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_restatement_agrees_with_torch_cross_entropy(case):
    T, V, ld = case
    lg, lab = C.inputs(T, V, ld)
    assert int((lab < 0).sum()) >= 1 and int((lab == 0).sum()) >= 1 and int((lab == V - 1).sum()) >= 1
    assert bool(torch.isnan(lg[lab < 0][:, :V]).all()) and bool((lg[:, V:] == C.PAD_VALUE).all())
    assert float(lg[0, :V].max()) == 80.0 and float(lg[0, :V].min()) < -78.0 and bool((lg[1, :V] == lg[1, 0]).all())
    scale = 0.37 * 0.003
    r = C.ce_ref(lg, lab, V, scale)
    x = torch.where((lab >= 0)[:, None], lg[:, :V].double(), torch.zeros(T, V, dtype=torch.float64)).requires_grad_(True)
    want = torch.nn.functional.cross_entropy(x, lab.long(), ignore_index=-1, reduction='sum')
    (want * scale).backward()
    assert abs(float(r.loss) - float(want.detach())) <= 1e-12 * max(1., abs(float(want.detach())))
    assert float(r.count) == float((lab >= 0).sum())
    assert float((r.d - x.grad).abs().max()) <= 1e-15
    assert bool((r.d[lab < 0] == 0).all()) and bool((r.lse[lab < 0] == 0).all())
    lse = torch.logsumexp(x.detach(), dim=1)
    assert float((r.lse - lse)[lab >= 0].abs().max()) <= 1e-12 * 160
    tol_lse, tol_loss, tol_d = C.bounds(r, V, scale)
    assert tol_lse.shape == (T,) and tol_d.shape == (T, V) and float(tol_loss) > 0
    assert bool((tol_lse[lab >= 0] > 0).all()) and bool((tol_d[lab >= 0] > 0).all()) and bool((tol_d[lab < 0] == 0).all())
    # the bounds are about rounding: far below the quantities they bound
    assert float(tol_lse.max()) <= 2e-4 and float(tol_loss) <= 1e-3 * max(1., abs(float(r.loss)))
