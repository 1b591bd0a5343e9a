"""Per-token losses, everything that runs without a GPU (cases, restatements and bounds: tests/_token_loss_cases.py): the float64 row term against torch, the
refusals, the plan key, `flow_index` against the packing contract, the C ABI, and a token-loss plan built on the CPU."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _loss_weight_cases as C                                       # noqa: E402
import _text_loss_terms_cases as R                                   # noqa: E402
import _token_loss_cases as K                                        # noqa: E402

NEW_FNS = {'tfx_ce_rows_fwd': 'tfx_ce_rows_args', 'tfx_mse_rows_fwd': 'tfx_mse_rows_args'}


def _name(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


# ================================================================================================ the restatements
@pytest.mark.parametrize('setting', K.SETTINGS, ids=R.setting_id)
def test_row_term_equals_torch_cross_entropy_per_row(setting):
    """F.cross_entropy(reduction = 'none', label_smoothing = e) + z lse^2, row by row; and the restatement the bounds hang on (ce_w_ref) says the same"""
    T, V, ld = R.CASES[1]
    z, e = R.f32(setting[0]), R.f32(setting[1])
    lg, lab = R.inputs(T, V, ld)
    got = K.row_term(lg, lab, V, *setting)
    keep = lab >= 0
    x = lg[keep][:, :V].double()
    want = torch.nn.functional.cross_entropy(x, lab[keep].long(), reduction='none', label_smoothing=e) + z * torch.logsumexp(x, dim=-1) ** 2
    assert float((got[keep] - want).abs().max()) <= 1e-12 * float(want.abs().max()) and not bool(got[~keep].any())
    w = C.weights(T, 'uniform')
    r = C.ce_w_ref(lg, lab, w, V, *setting)
    assert float((r.w * r.row - w.double() * got).abs().max()) <= 1e-12 * float(want.abs().max())
    tol_lse, tol_row = K.row_loss_bounds(r)
    live = keep & (w != 0)
    assert bool((tol_row[live] > 0).all()) and not bool(tol_row[~live].any()) and bool((tol_row[live] >= (r.w * tol_lse)[live]).all())
    assert float((tol_row / (r.w * r.row).abs().clamp(min=1e-30))[live].max()) < 1e-3, 'a bound this loose would hide a wrong term'


def test_row_sse_is_the_squared_error_per_row():
    from _decode_loss_cases import mse_inputs
    pred, flow, *_ = mse_inputs(37, 5, seed=1)
    w = C.weights(37, 'uniform')
    got = K.row_sse(pred, flow, w)
    want = w.double() * torch.nn.functional.mse_loss(pred.double(), flow.double(), reduction='none').sum(dim=1)
    assert float((got - want).abs().max()) <= 1e-13 and not bool(got[w == 0].any())
    assert abs(float(got.sum()) - float(C.mse_w_ref(pred, flow, w, 1.0)[0])) <= 1e-12 * float(got.sum())
    b = K.row_sse_bound(pred, flow, w, 64)
    assert bool((b[w != 0] > 0).all()) and float((b / got.clamp(min=1e-30))[w != 0].max()) < 1e-5


# ================================================================================================ the public surface
def test_the_switch_the_named_tuple_and_unchanged_signatures():
    """the per-token losses are a switch on the model (set_token_losses_, like the text loss terms and the head chunking): the three entry points keep the
    signatures they had - `loss_weights` stays their last and only keyword-only parameter (tests/test_loss_weights_cpu.py)"""
    from transfusion_pytorch_amd import TokenLosses, Transfusion
    assert TokenLosses._fields == ('text', 'text_weight', 'flow', 'flow_index')
    for fn in (Transfusion.forward, Transfusion.forward_text, Transfusion.forward_modality):
        ps = list(inspect.signature(fn).parameters.values())
        assert ps[-1].name == 'loss_weights' and [p.name for p in ps if p.kind is inspect.Parameter.KEYWORD_ONLY] == ['loss_weights']
    m = _model()
    assert m._token_losses is False and m.set_token_losses_() is m and m._token_losses is True and m.set_token_losses_(False)._token_losses is False
    for bad in (1, None, 'on'):
        with pytest.raises(ValueError):
            m.set_token_losses_(bad)
    import copy
    assert copy.deepcopy(m.set_token_losses_())._token_losses is False, 'a copy (an EMA teacher, a reference model) starts with the switch off'


def _model(**kw):
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(0)
    m = Transfusion(num_text_tokens=16, dim_latent=8, transformer=dict(dim=64, depth=1, heads=1), **kw)
    m._require_gpu = lambda: None                                    # the refusals stand in front of every device call
    return m


def test_refusals():
    m = _model()
    batch = [[torch.randint(0, 16, (4,)), torch.randn(3, 8)]]
    for kw in (dict(return_loss=False), dict(return_embed=True), dict(return_only_pred_flows=True), dict(return_kv_cache=True), dict(cache=object()),
               dict(decoding_text_or_modality='text')):
        with pytest.raises(ValueError, match='set_token_losses_'):
            m.set_token_losses_()(batch, **kw)
    with pytest.raises(NotImplementedError, match='forward_text'):
        m.set_token_losses_()(torch.randint(0, 16, (2, 8)))
    with pytest.raises(NotImplementedError, match='forward_modality'):
        m(torch.randn(2, 3, 8))
    with pytest.raises(NotImplementedError, match='velocity'):
        m.set_token_losses_()(batch, velocity_consistency_ema_model=object())
    with pytest.raises(NotImplementedError, match='velocity'):
        m.set_token_losses_().forward_modality(torch.randn(2, 3, 8), velocity_consistency_ema_model=object())
    with pytest.raises(ValueError, match='set_token_losses_'):
        m.set_token_losses_().forward_text(torch.randint(0, 16, (2, 8)), return_loss=False)
    with pytest.raises(ValueError, match='set_token_losses_'):
        m.set_token_losses_().forward_modality(torch.randn(2, 3, 8), return_loss=False)
    r = _model(reconstruction_loss_weight=0.5)
    with pytest.raises(NotImplementedError, match='reconstruction'):
        r.set_token_losses_()(batch)
    with pytest.raises(NotImplementedError, match='reconstruction'):
        r.set_token_losses_().forward_modality(torch.randn(2, 3, 8))


def test_plan_key_switch_off_is_the_parents_key(monkeypatch):
    from transfusion_pytorch_amd import transfusion as T
    made = []

    class Stub:
        nbytes = 1

        def __init__(self, store, b, n, I, R, training=True, dp_groups=0, ckpt=False, **kw):
            self.kw = kw
            made.append(self)

        def select_frozen(self, *a):
            pass
    monkeypatch.setattr(T, 'Plan', Stub)
    monkeypatch.setenv('TFX_PLAN_BUDGET_GB', '1')
    m = _model()
    p0 = m._plan(2, 64, 0, {}, True, text_loss=True)
    pw = m._plan(2, 64, 0, {}, True, text_loss=True, weighted=True)
    assert m._plan(2, 64, 0, {}, True, text_loss=True, token_losses=False) is p0 and m._plan(2, 64, 0, {}, True, text_loss=True, weighted=True, token_losses=False) is pw
    assert list(m._plans) == [(2, 64, 0, (), True, 0, False, None, None, False), (2, 64, 0, (), True, 0, False, None, None, True)], 'the keys of the parent'
    pt = m._plan(2, 64, 0, {}, True, text_loss=True, token_losses=True)
    assert pt.kw == {'token_losses': True} and pt is not p0 and pt is not pw
    assert m._plan(2, 64, 0, {}, True, text_loss=True, weighted=True, token_losses=True) is pt, 'keyed by the switch alone: weights ride on the same plan'
    i0 = m._plan(2, 64, 0, {}, False, text_loss=True)
    assert m._plan(2, 64, 0, {}, False, text_loss=True, token_losses=True) is i0, 'inference plans never look at the switch'
    assert len(made) == 4


@pytest.mark.parametrize('which', ['batch', 'signature'])
def test_flow_index_follows_the_packing_contract(which):
    from transfusion_pytorch_amd.packing import fast_signature, flow_row_index, scan_batch, scan_signature
    mods, want = K.flow_index_batch()
    P = scan_batch(mods, add_sos_eos=True, **C.PACK_KW) if which == 'batch' else scan_signature(*fast_signature(mods), add_sos_eos=True, **C.PACK_KW)
    got = flow_row_index(P)
    assert sorted(got) == [0, 1]
    for t in got:
        assert got[t].dtype.name == 'int64' and got[t].shape == (len(P.row_inst[t]), 2) and got[t].tolist() == [list(p) for p in want[t]], (t, got[t].tolist())
        # the contract: row k of the type sits at flat position row_pos[k] of its sample's row, inside the k-th instance's slots
        assert (P.row_pos[t] // P.n_full == got[t][:, 0]).all()
    assert 1 not in set(got[0][:, 0]) | set(got[1][:, 0]), 'the sample without modalities owns no row'


# ================================================================================================ the C ABI
def test_capi_tables_hold_the_new_entry_points():
    from transfusion_pytorch_amd import capi
    for fn in NEW_FNS:
        assert capi.FUNCTIONS[fn] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert (capi.ENUMS['TFX_OP_CE_ROWS_FWD'], capi.ENUMS['TFX_OP_MSE_ROWS_FWD']) == (62, 63)
    ops = [v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_')]
    assert len(ops) == len(set(ops)), 'two launch-list ops share a code'
    w = dict(capi.STRUCT_FIELDS['tfx_ce_w_chunk_args'])
    rows = capi.STRUCT_FIELDS['tfx_ce_rows_args']
    assert [n for n, _ in rows] == ['T', 'V', 'logits', 'ld', 'labels', 'lse', 'acc', 'z_weight', 'smoothing', 'aux', 'row_w', 'row_loss']
    assert all(w[n] == ty for n, ty in rows[:-1]) and rows[-1][1] is ctypes.c_void_p, 'the forward fields of tfx_ce_w_chunk_args, then row_loss'
    assert [n for n, _ in capi.STRUCT_FIELDS['tfx_mse_rows_args']] == ['R', 'dl', 'pred', 'ld_pred', 'flow', 'ld_d', 'acc', 'row_w', 'row_sse']
    # the structs and codes beside them are what they were
    assert [n for n, _ in capi.STRUCT_FIELDS['tfx_ce_w_chunk_args']][-1] == 'row_w' and [n for n, _ in capi.STRUCT_FIELDS['tfx_mse_w_args']][-1] == 'row_w'
    assert (capi.ENUMS['TFX_OP_CE_W_FWD_BWD'], capi.ENUMS['TFX_OP_CE_W_FWD'], capi.ENUMS['TFX_OP_CE_W_BWD'], capi.ENUMS['TFX_OP_MSE_W_FWD_BWD']) == (58, 59, 60, 61)


def test_library_exports_and_host_checks_return_before_any_launch():
    """host logic only: every pointer is host memory no kernel could touch, so a launch would fault"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    assert b'-tokloss' in lib.tfx_version()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    ok = dict(T=2, V=10, logits=base, ld=16, labels=base, lse=base, acc=base, z_weight=0., smoothing=0., aux=base, row_w=base, row_loss=base)
    mk = lambda **kw: ctypes.byref(capi.make_args('tfx_ce_rows_args', **dict(ok, **kw)))
    fn = lib.tfx_ce_rows_fwd
    assert fn(None, None) == -1 and fn(mk(T=0), None) == 0
    for bad in (dict(row_w=None), dict(row_loss=None), dict(T=0, row_loss=None), dict(z_weight=-1.), dict(smoothing=1.0), dict(ld=12), dict(V=0), dict(V=17),
                dict(logits=base + 4), dict(T=-1), dict(logits=None), dict(labels=None), dict(lse=None), dict(acc=None), dict(aux=None)):
        assert fn(mk(**bad), None) == -1, bad
    okm = dict(R=2, dl=4, pred=base, ld_pred=4, flow=base, ld_d=64, acc=base, row_w=base, row_sse=base)
    mm = lambda **kw: ctypes.byref(capi.make_args('tfx_mse_rows_args', **dict(okm, **kw)))
    fn = lib.tfx_mse_rows_fwd
    assert fn(None, None) == -1 and fn(mm(R=0), None) == 0
    for bad in (dict(row_w=None), dict(row_sse=None), dict(R=0, row_sse=None), dict(ld_d=48), dict(ld_d=0), dict(dl=65), dict(dl=5), dict(R=-1), dict(pred=None),
                dict(flow=None), dict(acc=None)):
        assert fn(mm(**bad), None) == -1, bad


def test_run_list_and_fingerprint_know_the_new_ops():
    from transfusion_pytorch_amd import capi
    from transfusion_pytorch_amd.engine import LaunchList
    c = capi.make_args('tfx_ce_rows_args', T=0, row_w=64, row_loss=64)
    m = capi.make_args('tfx_mse_rows_args', R=0, ld_d=64, row_w=64, row_sse=64)
    L = LaunchList([('tfx_ce_rows_fwd', c), ('tfx_mse_rows_fwd', m)])
    failed = ctypes.c_int32(-1)
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == 0 and failed.value == -1
    m.row_sse = None
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == -1 and failed.value == 1
    m.row_sse = 64

    def fp():
        out = ctypes.c_int64()
        assert capi.lib().tfx_list_fingerprint(L.native(), len(L), ctypes.byref(out)) == 0
        return out.value
    f0 = fp()
    c.row_loss = 128
    f1 = fp()
    m.row_sse = 128
    assert len({f0, f1, fp()}) == 3, 'the fingerprint hashes the last field of both structs'


# ================================================================================================ plans built on the CPU
def _cpu_plan(**kw):
    from _plan_digest import cpu_plan
    return cpu_plan(depth=2, **kw)


def test_plans_without_the_switch_are_what_they_were():
    from _plan_digest import digest
    _, _, A = _cpu_plan(b=3, n=64)
    _, _, B = _cpu_plan(b=3, n=64, token_losses=False)
    assert digest(B) == digest(A) and not B.token_losses and not B.weighted and B.nbytes == A.nbytes and not hasattr(B, 'row_loss') and not len(B.seed)
    _, _, W = _cpu_plan(b=3, n=64, weighted=True)
    _, _, X = _cpu_plan(b=3, n=64, weighted=True, token_losses=False)
    assert digest(X) == digest(W) and X.nbytes == W.nbytes
    _, _, I = _cpu_plan(b=3, n=64, token_losses=True, training=False)
    assert not I.token_losses and not I.weighted, 'an inference plan never looks at the switch'


@pytest.mark.parametrize('terms', [None, (1e-4, 0.1)], ids=['plain', 'text_terms'])
@pytest.mark.parametrize('rows', [None, 64], ids=['whole_head', 'rows64'])
def test_token_loss_plan_runs_the_split_losses_and_nothing_else_differs(rows, terms):
    from transfusion_pytorch_amd import capi
    kw = dict(chunk_rows=rows) if rows else {}
    kt = dict(text_terms=terms) if terms else {}
    _, _, Q = _cpu_plan(b=3, n=64, weighted=True, **kw, **kt)
    _, _, P = _cpu_plan(b=3, n=64, token_losses=True, **kw, **kt)
    assert P.token_losses and P.weighted and P.reg == Q.reg
    swap = {'tfx_ce_w_fwd_bwd': 'tfx_ce_rows_fwd', 'tfx_ce_w_fwd': 'tfx_ce_rows_fwd', 'tfx_mse_w_fwd_bwd': 'tfx_mse_rows_fwd'}
    assert [_name(i) for i in P.fwd] == [swap.get(_name(i), _name(i)) for i in Q.fwd]
    fused = {'tfx_ce_fwd_bwd', 'tfx_ce_reg_fwd_bwd', 'tfx_ce_w_fwd_bwd', 'tfx_mse_fwd_bwd'}
    assert not fused & {_name(i) for L in (P.fwd, P.bwd, P.seed, P.vel, P.rec) for i in L}
    assert [_name(i) for i in P.bwd] == [_name(i) for i in Q.bwd], 'the chunked head keeps tfx_ce_w_bwd in the list; the whole head keeps its two products'
    native = [t for t in P.R if t not in P.ext]
    assert [_name(i) for i in P.seed] == ([] if rows else ['tfx_ce_w_bwd']) + ['tfx_mse_w_fwd_bwd'] * len(native)
    assert (P.fwd_embed_end, P.fwd_logits_end, P.fwd_pred_end, P.bwd_cuts, P.bwd_end) == (Q.fwd_embed_end, Q.fwd_logits_end, Q.fwd_pred_end, Q.bwd_cuts, Q.bwd_end)
    # buffers: acc and aux keep their layout; the row sums of every native type ride behind them in the one zeroed buffer
    assert P.acc.numel() == Q.acc.numel() and P.aux.data_ptr() == P.acc.data_ptr() + 4 * P.acc.numel()
    o = P.aux.data_ptr() + 8
    for t in native:
        lt = P.lat[t]
        assert lt['row_sse'].data_ptr() == o and lt['row_sse'].shape == lt['weff_row'].shape == (P.R[t],)
        o += 4 * P.R[t]
    assert P._acc_all.numel() == P.acc.numel() + 2 + sum(P.R[t] for t in native)
    assert P.row_loss.shape == P.weff_text.shape == P.ce_lse.shape == (P.T,)
    # the forward structs: the chunk's (or the whole buffer's) logits, the step's weights, the row outputs
    z32, e32 = (ctypes.c_float(terms[0]).value, ctypes.c_float(terms[1]).value) if terms else (0., 0.)
    fw = [i[1] for i in P.fwd if _name(i) == 'tfx_ce_rows_fwd']
    bw = [i[1] for L in (P.bwd, P.seed) for i in L if _name(i) == 'tfx_ce_w_bwd']
    assert len(fw) == len(bw) == (3 if rows else 1)
    for a, g in zip(fw, bw):
        assert isinstance(a, capi.STRUCTS['tfx_ce_rows_args']) and isinstance(g, capi.STRUCTS['tfx_ce_w_chunk_args'])
        r0 = (a.row_w - P.w_text.data_ptr()) // 4
        assert (a.labels - P.labels.data_ptr(), a.row_loss - P.row_loss.data_ptr(), a.lse - P.ce_lse.data_ptr()) == (4 * r0,) * 3 and a.T == (64 if rows else P.T)
        assert (a.z_weight, a.smoothing, a.aux, a.acc) == (z32, e32, P.aux.data_ptr(), P.acc.data_ptr())
        assert a.logits == g.logits == (P.logits_c if rows else P.logits).data_ptr()
        # the backward: effective row weights, no other scale, the forward's lse
        assert (g.row_w, g.lse, g.labels, g.T) == (P.weff_text.data_ptr() + 4 * r0, a.lse, a.labels, a.T) and g.grad_scale == 1.0 and not g.scale_dev
        assert g.dlogits == (P.dlogits_c if rows else P.dlogits).data_ptr() and (g.z_weight, g.smoothing) == (z32, e32)
    for t, g in zip(native, [i[1] for i in P.seed if _name(i) == 'tfx_mse_w_fwd_bwd']):
        a, lt = P._mse_args[t], P.lat[t]
        assert isinstance(a, capi.STRUCTS['tfx_mse_rows_args']) and (a.row_w, a.row_sse, a.R, a.ld_d) == (lt['w_row'].data_ptr(), lt['row_sse'].data_ptr(), P.R[t], g.ld_d)
        assert (g.row_w, g.dpred, g.pred, g.flow, g.acc, g.grad_scale, g.accumulate) == (lt['weff_row'].data_ptr(), lt['dpred'].data_ptr(), a.pred, a.flow, P.seed_acc.data_ptr(), 2.0, 0)
    # the per-step setters: V reaches every struct, the loss scales are remembered for the backward, set_rows reaches both halves
    P.set_ce_vocab(11); P.set_loss_scales(0.25, {t: 0.5 for t in native})
    assert all(a.V == 11 for a in fw + bw) and all(g.grad_scale == 1.0 for g in bw) and P.ce_seed == 0.25 and P.mse_seed == {t: 0.25 for t in native}
    P.set_rows({t: r - 1 for t, r in P.R.items()})
    assert all(P._mse_args[t].R == P.R[t] - 1 for t in native) and all(i[1].R == P.R[t] - 1 for t, i in zip(native, [i for i in P.seed if _name(i) == 'tfx_mse_w_fwd_bwd']))


def test_effective_row_weights():
    """w (go x d loss / d row value + d total / d row value); None = nobody used the output; rows past the real ones stay 0"""
    _, _, P = _cpu_plan(b=3, n=64, token_losses=True)
    native = [t for t in P.R if t not in P.ext]
    P.set_loss_scales(0.25, {t: 0.5 for t in native})
    g0 = torch.Generator().manual_seed(0)
    P.w_text.copy_(torch.rand(P.T, generator=g0))
    go = torch.tensor(2.0)
    P.set_token_loss_seeds(go)
    assert torch.equal(P.weff_text, P.w_text * 0.5)
    gt = torch.randn(P.T, generator=g0)
    for t in native:
        P.lat[t]['w_row'].copy_(torch.rand(P.R[t], generator=g0)); P.lat[t]['w_row'][-2:] = 0
    gr = {native[0]: torch.randn(P.R[native[0]] - 2, generator=g0)}
    P.set_token_loss_seeds(go, gt, gr)
    assert torch.allclose(P.weff_text, P.w_text * (0.5 + gt), rtol=1e-6, atol=0)
    for t in native:
        w, k = P.lat[t]['w_row'], P.R[t] - 2
        want = w * 0.5
        if t in gr:
            want[:k] = w[:k] * (0.5 + gr[t])
        assert torch.allclose(P.lat[t]['weff_row'], want, rtol=1e-6, atol=0) and not bool(P.lat[t]['weff_row'][k:].any())


def test_token_loss_plan_under_frozen_sets_checkpointing_and_exchange_groups():
    m, ps, P = _cpu_plan(b=3, n=64, chunk_rows=64, token_losses=True)
    full = [_name(i) for i in P.bwd]
    P.select_frozen(frozenset({'to_text_logits.weight'}))
    assert [_name(i) for i in P.bwd[:9]] == ['tfx_gemm_nt', 'tfx_ce_w_bwd', 'tfx_gemm_nt'] * 3
    P.set_ce_vocab(13)
    P.select_frozen(frozenset())
    assert [_name(i) for i in P.bwd] == full and all(i[1].V == 13 and i[1].grad_scale == 1.0 for i in P.bwd if _name(i) == 'tfx_ce_w_bwd')
    _, _, C2 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True, token_losses=True)
    _, _, C0 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True)
    assert C2.ckpt and C2._recompute == C0._recompute
    _, _, G = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2, token_losses=True)
    _, _, H = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2)
    assert G.bwd_cuts == H.bwd_cuts and G.bwd_cuts
