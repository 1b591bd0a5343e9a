"""Per-token loss weights, everything that runs without a GPU (cases and restatements: tests/_loss_weight_cases.py): the weight layout of both scanners
against hand-written tables, the refusals, the float64 restatements against torch, the C ABI (structs, codes, host checks), and a weighted plan built on the CPU."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _loss_weight_cases as C                                       # noqa: E402
import _text_loss_terms_cases as R                                   # noqa: E402

W_FNS = ('tfx_ce_w_fwd_bwd', 'tfx_ce_w_fwd', 'tfx_ce_w_bwd', 'tfx_mse_w_fwd_bwd')
LAYOUTS = [('text_only',), ('modality_first',), ('modality_last',), ('two_types',), ('adjacent',),
           ('text_only', 'two_types', 'none', 'adjacent', 'modality_last', 'modality_first')]


def _name(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


def _scan(mods, which):
    from transfusion_pytorch_amd.packing import fast_signature, scan_batch, scan_signature
    if which == 'batch':
        return scan_batch(mods, add_sos_eos=True, **C.PACK_KW)
    return scan_signature(*fast_signature(mods), add_sos_eos=True, **C.PACK_KW)


# ================================================================================================ the weight layout
@pytest.mark.parametrize('which', ['batch', 'signature'])
@pytest.mark.parametrize('names', LAYOUTS, ids='+'.join)
def test_token_grid_equals_the_hand_written_table(names, which):
    from transfusion_pytorch_amd.packing import lay_loss_weights
    mods, lw, grid, w_inst = C.layout_batch(names)
    P = _scan(mods, which)
    got, gi = lay_loss_weights(P, lw, torch.device('cpu'))
    assert got.shape == grid.shape == (P.b, P.n_full) and got.dtype == torch.float32
    assert torch.equal(got, grid), (names, got.tolist(), grid.tolist())
    assert torch.equal(gi, w_inst)
    # inserted tokens and [eos] sit where the table says: the row's ids are special exactly where the packer put them
    assert all(int(P.text_host[i, 0]) == C.PACK_KW['sos_id'] and int(P.text_host[i, P.lens[i] - 1]) == C.PACK_KW['eos_id'] for i in range(P.b))


@pytest.mark.parametrize('names', LAYOUTS, ids='+'.join)
def test_both_scanners_yield_the_same_layout(names):
    mods = C.layout_batch(names)[0]
    A, B = _scan(mods, 'batch'), _scan(mods, 'signature')
    for f in ('part_b', 'part_start', 'part_len', 'part_inst', 'eos_dest'):
        a, b = getattr(A, f), getattr(B, f)
        assert a.shape == b.shape and (a == b).all(), f


def test_zero_d_tensors_and_numbers_are_the_same_weight():
    from transfusion_pytorch_amd.packing import lay_loss_weights
    mods, lw, grid, w_inst = C.layout_batch(('two_types', 'adjacent'))
    P = _scan(mods, 'batch')
    lw_t = [[torch.tensor(w) if isinstance(w, float) else w for w in s] for s in lw]
    got, gi = lay_loss_weights(P, lw_t, torch.device('cpu'))
    assert torch.equal(got, grid) and torch.equal(gi, w_inst)


def test_refusals_of_the_layout():
    from transfusion_pytorch_amd.packing import lay_loss_weights
    mods, lw, _, _ = C.layout_batch(('two_types', 'text_only'))
    P = _scan(mods, 'batch')
    cpu = torch.device('cpu')
    lay = lambda w: lay_loss_weights(P, w, cpu)
    lay(lw); lay([None, None])
    nan, inf = float('nan'), float('inf')
    bad = [
        [None],                                                     # one entry per sample
        [[1.0, 1.0], None],                                         # one entry per part
        [[1.0, 1.0, 1.0, 1.0], None],
        [None, 1.0],                                                # a sample takes a list
        [[-0.5, None, None], None], [[nan, None, None], None], [[inf, None, None], None],
        [[torch.tensor(-1.0), None, None], None], [[None, torch.tensor([0.5, nan]), None], None], [[None, torch.tensor([0.5, -1e-9]), None], None],
        [[None, torch.tensor([0.5, 0.5, 0.5]), None], None],        # a text tensor of another length
        [[torch.tensor([1.0, 1.0]), None, None], None],             # a modality part takes one weight
        [[None, torch.ones(1, 2), None], None],                     # 2-D
        [[None, torch.tensor([1, 1]), None], None],                 # an integer tensor
        [['1', None, None], None], [[True, None, None], None],
    ]
    for w in bad:
        with pytest.raises(ValueError):
            lay(w)


def test_checked_tensors_are_remembered_by_identity_and_version():
    """a tensor that passed is not read again while it is the same object at the same version; an in-place edit, or another tensor, is checked afresh"""
    from transfusion_pytorch_amd.packing import check_weight_tensors
    seen = {}
    w = torch.tensor([0.5, 1.0])
    check_weight_tensors([w], [w], seen)
    assert list(seen) == [id(w)] and seen[id(w)][0]() is w and seen[id(w)][1] == w._version
    poisoned = torch.tensor([float('nan'), 1.0])
    check_weight_tensors([w], [poisoned], seen)                       # remembered: the copy that stands for it is not looked at
    w[0] = -1.0                                                       # edited in place: another version
    with pytest.raises(ValueError):
        check_weight_tensors([w], [w], seen)
    with pytest.raises(ValueError):
        check_weight_tensors([torch.tensor([float('inf')])], [torch.tensor([float('inf')])], seen)
    with pytest.raises(ValueError):
        check_weight_tensors([poisoned], [poisoned], None)
    mods, lw, grid, _ = C.layout_batch(('two_types', 'text_only'))
    from transfusion_pytorch_amd.packing import lay_loss_weights
    P = _scan(mods, 'batch')
    seen = {}
    got, _ = lay_loss_weights(P, lw, torch.device('cpu'), seen=seen)
    assert torch.equal(got, grid) and len(seen) == sum(torch.is_tensor(w) for s in lw if s for w in s)
    lw[0][1][0] = -2.0
    with pytest.raises(ValueError):
        lay_loss_weights(P, lw, torch.device('cpu'), seen=seen)


def test_forward_signatures_take_the_weights_last_and_keyword_only():
    from transfusion_pytorch_amd import Transfusion
    for fn in (Transfusion.forward, Transfusion.forward_text, Transfusion.forward_modality):
        ps = list(inspect.signature(fn).parameters.values())
        assert ps[-1].name == 'loss_weights' and ps[-1].kind is inspect.Parameter.KEYWORD_ONLY and ps[-1].default is None
        assert sum(p.kind is inspect.Parameter.KEYWORD_ONLY for p in ps) == 1


# ================================================================================================ the restatements
@pytest.mark.parametrize('setting', C.SETTINGS, ids=R.setting_id)
@pytest.mark.parametrize('case', R.CASES[:3], ids=R.case_id)
def test_all_ones_equal_the_unweighted_restatement(case, setting):
    T, V, ld = case
    lg, lab = R.inputs(T, V, ld)
    a, b = C.ce_w_ref(lg, lab, torch.ones(T), V, *setting, 0.37), R.reg_ref(lg, lab, V, *setting, 0.37)
    assert torch.equal(a.d, b.d) and float(a.loss) == float(b.loss) and float(a.wsum) == float(b.count)
    assert float(a.ce_sum) == float(b.ce_sum) and float(a.sq_sum) == float(b.sq_sum)


@pytest.mark.parametrize('case', R.CASES[:3], ids=R.case_id)
def test_binary_weights_equal_torch_cross_entropy_over_the_kept_rows(case):
    T, V, ld = case
    lg, lab = R.inputs(T, V, ld)
    w = C.weights(T, 'binary')
    r = C.ce_w_ref(lg, lab, w, V)
    keep = (lab >= 0) & (w != 0)
    x = lg[keep][:, :V].double().requires_grad_(True)
    per = torch.nn.functional.cross_entropy(x, lab[keep].long(), reduction='none')
    assert abs(float(per.sum()) - float(r.loss)) <= 1e-12 * float(per.sum()) and float(r.wsum) == int(keep.sum())
    per.sum().backward()
    assert float((x.grad - r.d[keep]).abs().max()) <= 1e-14 and not bool(r.d[~keep].any())


@pytest.mark.parametrize('setting', C.SETTINGS, ids=R.setting_id)
def test_uniform_weights_equal_torch_weighted_rows(setting):
    """sum_t w_t (F.cross_entropy(label_smoothing = e, reduction = 'none') + z lse^2) and its autograd gradient; the weighted mean is F.cross_entropy's
    `weight` normalisation sum w r / sum w"""
    T, V, ld = R.CASES[1]
    z, e = R.f32(setting[0]), R.f32(setting[1])
    lg, lab = R.inputs(T, V, ld)
    w = C.weights(T, 'uniform')
    r = C.ce_w_ref(lg, lab, w, V, *setting, 0.37)
    keep = (lab >= 0) & (w != 0)
    assert 0.1 < float((w == 0).float().mean()) < 0.4
    x = lg[keep][:, :V].double().requires_grad_(True)
    per = torch.nn.functional.cross_entropy(x, lab[keep].long(), reduction='none', label_smoothing=e) + z * torch.logsumexp(x, dim=-1) ** 2
    tot = (w[keep].double() * per).sum()
    assert abs(float(tot) - float(r.loss)) <= 1e-12 * abs(float(tot))
    (0.37 * tot).backward()
    assert float((x.grad - r.d[keep]).abs().max()) <= 1e-13
    bounds = C.ce_w_bounds(r, 0.37)
    assert all(bool(torch.isfinite(torch.as_tensor(t)).all()) for t in bounds) and bool((bounds[5][keep] > 0).all()) and not bool(bounds[5][~keep].any())


def test_mse_restatement():
    from _decode_loss_cases import CLEAN_EPS, mse_inputs, mse_reference
    pred, flow, noise, times, row_inst, _ = mse_inputs(37, 5, seed=1)
    t_row = times[row_inst.long()]
    for clean in (None, CLEAN_EPS):
        loss1, g1 = C.mse_w_ref(pred, flow, torch.ones(37), 0.37, t_row, clean)
        loss0, g0 = mse_reference(pred, flow, noise, t_row, 0.37, clean_eps=clean)
        assert abs(float(loss1) - float(loss0)) <= 1e-12 * float(loss0) and float((g1 - g0).abs().max()) <= 1e-12
    w = C.weights(37, 'uniform')
    loss, g = C.mse_w_ref(pred, flow, w, 0.37)
    p = pred.double().requires_grad_(True)
    ref = (w.double()[:, None] * (p - flow.double()) ** 2).sum()
    (0.5 * 0.37 * ref).backward()
    assert abs(float(loss) - float(ref)) <= 1e-12 * float(ref) and float((g - p.grad).abs().max()) <= 1e-14 and not bool(g[w == 0].any())


# ================================================================================================ the C ABI
def test_capi_tables_hold_the_new_entry_points():
    from transfusion_pytorch_amd import capi
    for fn in W_FNS:
        assert capi.FUNCTIONS[fn] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        assert capi.ENUMS['TFX_OP_' + fn[4:].upper()] > capi.ENUMS['TFX_OP_CE_REG_BWD']
    ops = [v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_')]
    assert len(ops) == len(set(ops)), 'two launch-list ops share a code'
    row_w = [('row_w', ctypes.c_void_p)]
    assert capi.STRUCT_FIELDS['tfx_ce_w_args'] == capi.STRUCT_FIELDS['tfx_ce_reg_args'] + row_w
    assert capi.STRUCT_FIELDS['tfx_ce_w_chunk_args'] == capi.STRUCT_FIELDS['tfx_ce_reg_chunk_args'] + row_w
    plain = capi.STRUCT_FIELDS['tfx_mse_args']
    assert capi.STRUCT_FIELDS['tfx_mse_w_args'] == plain[:[n for n, _ in plain].index('recon_w')] + row_w
    # the structs beside them are what they were
    assert [n for n, _ in capi.STRUCT_FIELDS['tfx_ce_reg_args']][-3:] == ['z_weight', 'smoothing', 'aux']
    assert [n for n, _ in plain][-4:] == ['recon_w', 'recon_inst', 'recon_time', 'recon_mode']
    assert (capi.ENUMS['TFX_OP_CE_REG_FWD_BWD'], capi.ENUMS['TFX_OP_CE_REG_FWD'], capi.ENUMS['TFX_OP_CE_REG_BWD'], capi.ENUMS['TFX_OP_MSE_FWD_BWD']) == (55, 56, 57, 19)


def test_library_exports_the_entry_points_and_the_version_tag():
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    for fn in W_FNS:
        assert getattr(lib, fn) is not None
    assert b'-lossw' in lib.tfx_version()


def test_host_checks_return_before_any_launch():
    """host logic only: every pointer is host memory no kernel could touch, so a launch would fault.  NULL row_w returns -1 from all four entry points; the
    other rules are those of tfx_ce_reg_*; z_weight = smoothing = 0 is allowed (checked with T = 0, which returns before a launch)"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    ok = dict(T=2, V=10, logits=base, ld=16, labels=base, lse=base, acc=base, grad_scale=1.0, scale_dev=None, dlogits=base, ld_d=16, z_weight=0., smoothing=0., aux=base,
              row_w=base)
    mk = lambda **kw: ctypes.byref(capi.make_args('tfx_ce_w_chunk_args', **dict(ok, **kw)))
    for fn in (lib.tfx_ce_w_fwd, lib.tfx_ce_w_bwd):
        assert fn(None, None) == -1 and fn(mk(T=0), None) == 0
        for bad in (dict(row_w=None), dict(T=0, row_w=None), dict(z_weight=-1.), dict(smoothing=1.0), dict(ld=12), dict(V=0), dict(V=17), dict(logits=base + 4),
                    dict(T=-1), dict(logits=None), dict(labels=None), dict(lse=None)):
            assert fn(mk(**bad), None) == -1, bad
    for bad in (dict(ld_d=12), dict(dlogits=None)):
        assert lib.tfx_ce_w_bwd(mk(**bad), None) == -1, bad
    for bad in (dict(acc=None), dict(aux=None)):
        assert lib.tfx_ce_w_fwd(mk(**bad), None) == -1, bad
    okf = dict(T=2, V=10, logits=base, ld=16, labels=base, grad_scale=1.0, dlogits=base, ld_d=16, acc=base, z_weight=0., smoothing=0., aux=base, row_w=base)
    mf = lambda **kw: ctypes.byref(capi.make_args('tfx_ce_w_args', **dict(okf, **kw)))
    assert lib.tfx_ce_w_fwd_bwd(None, None) == -1 and lib.tfx_ce_w_fwd_bwd(mf(T=0), None) == 0
    for bad in (dict(row_w=None), dict(T=0, row_w=None), dict(T=-1), dict(V=0), dict(V=17), dict(ld_d=8), dict(logits=None), dict(labels=None), dict(dlogits=None),
                dict(acc=None), dict(aux=None), dict(smoothing=float('nan'))):
        assert lib.tfx_ce_w_fwd_bwd(mf(**bad), None) == -1, bad
    okm = dict(R=2, dl=4, pred=base, ld_pred=4, flow=base, grad_scale=1.0, dpred=base, ld_d=64, acc=base, row_w=base)
    mm = lambda **kw: ctypes.byref(capi.make_args('tfx_mse_w_args', **dict(okm, **kw)))
    assert lib.tfx_mse_w_fwd_bwd(None, None) == -1 and lib.tfx_mse_w_fwd_bwd(mm(R=0), None) == 0
    assert lib.tfx_mse_w_fwd_bwd(mm(row_w=None), None) == -1 and lib.tfx_mse_w_fwd_bwd(mm(R=0, row_w=None), None) == -1


def test_run_list_and_fingerprint_know_the_new_ops():
    from transfusion_pytorch_amd import capi
    from transfusion_pytorch_amd.engine import LaunchList
    a = capi.make_args('tfx_ce_w_args', T=0, row_w=64)
    c = capi.make_args('tfx_ce_w_chunk_args', T=0, row_w=64)
    m = capi.make_args('tfx_mse_w_args', R=0, row_w=64)
    L = LaunchList([('tfx_ce_w_fwd_bwd', a), ('tfx_ce_w_fwd', c), ('tfx_ce_w_bwd', c), ('tfx_mse_w_fwd_bwd', m)])
    failed = ctypes.c_int32(-1)
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == 0 and failed.value == -1
    m.row_w = None
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == -1 and failed.value == 3
    m.row_w = 64

    def fp():
        out = ctypes.c_int64()
        assert capi.lib().tfx_list_fingerprint(L.native(), len(L), ctypes.byref(out)) == 0
        return out.value
    f0 = fp()
    c.row_w = 128
    f1 = fp()
    m.row_w = 128
    assert len({f0, f1, fp()}) == 3, 'the fingerprint hashes the new field of every struct'


# ================================================================================================ plans built on the CPU
def _cpu_plan(**kw):
    from _plan_digest import cpu_plan
    return cpu_plan(depth=2, **kw)


def test_unweighted_plans_are_what_they_were():
    from _plan_digest import digest
    _, _, A = _cpu_plan(b=3, n=64)
    _, _, B = _cpu_plan(b=3, n=64, weighted=False)
    assert digest(B) == digest(A) and not B.weighted and B.aux is None and B.nbytes == A.nbytes and not hasattr(B, 'w_text')
    _, _, I = _cpu_plan(b=3, n=64, weighted=True, training=False)
    assert not I.weighted and I.aux is None, 'an inference plan never looks at the switch'


@pytest.mark.parametrize('terms', [None, (1e-4, 0.1)], ids=['plain', 'text_terms'])
@pytest.mark.parametrize('rows', [None, 64], ids=['whole_head', 'rows64'])
def test_weighted_plan_names_the_w_entry_points_and_nothing_else_differs(rows, terms):
    from transfusion_pytorch_amd import capi
    kw = dict(chunk_rows=rows) if rows else {}
    kt = dict(text_terms=terms) if terms else {}
    _, _, Q = _cpu_plan(b=3, n=64, **kw, **kt)
    _, _, P = _cpu_plan(b=3, n=64, weighted=True, **kw, **kt)
    assert P.weighted and not Q.weighted and P.reg == Q.reg

    def swap(n):
        if n.startswith('tfx_ce_'):
            return n.replace('tfx_ce_reg_' if n.startswith('tfx_ce_reg_') else 'tfx_ce_', 'tfx_ce_w_')
        return 'tfx_mse_w_fwd_bwd' if n == 'tfx_mse_fwd_bwd' else n
    got = [_name(i) for i in P.fwd]
    want = []
    for i in Q.fwd:                                                # the forward: a gather of the row weights ahead of every type's flow target
        if _name(i) == 'tfx_mse_fwd_bwd':
            want.append('tfx_gather_f32')
        want.append(swap(_name(i)))
    assert got == want
    assert [_name(i) for i in P.bwd] == [swap(_name(i)) for i in Q.bwd]
    assert [_name(i) for i in P.vel] == ['tfx_mse_w_fwd_bwd'] * len(Q.vel) and [_name(i) for i in P.rec] == [_name(i) for i in Q.rec] == ['tfx_mse_fwd_bwd'] * len(Q.rec)
    assert (P.fwd_embed_end, P.fwd_logits_end, P.fwd_pred_end, P.bwd_cuts, P.bwd_end) == (Q.fwd_embed_end, Q.fwd_logits_end, Q.fwd_pred_end, Q.bwd_cuts, Q.bwd_end)
    # buffers: acc keeps its layout, aux behind it, the three weight arrays
    assert P.acc.numel() == Q.acc.numel() and P.aux.numel() == 2 and P.aux.data_ptr() == P.acc.data_ptr() + 4 * P.acc.numel()
    assert P.w_text.shape == (P.T,) and P.w_inst.shape == (P.I,) and all(P.lat[t]['w_row'].shape == (r,) for t, r in P.R.items())
    assert all(b.dtype == torch.float32 for b in [P.w_text, P.w_inst] + [P.lat[t]['w_row'] for t in P.R])
    ces = [(i[1], k) for L in (P.fwd, P.bwd) for k, i in enumerate(L) if _name(i).startswith('tfx_ce_w_')]
    assert len(ces) == (6 if rows else 1)
    z32, e32 = (ctypes.c_float(terms[0]).value, ctypes.c_float(terms[1]).value) if terms else (0., 0.)
    seen = set()
    for a, _ in ces:
        assert isinstance(a, capi.STRUCTS['tfx_ce_w_chunk_args' if rows else 'tfx_ce_w_args'])
        assert (a.z_weight, a.smoothing, a.aux, a.acc) == (z32, e32, P.aux.data_ptr(), P.acc.data_ptr())
        r0 = (a.row_w - P.w_text.data_ptr()) // 4
        assert a.labels - P.labels.data_ptr() == 4 * r0 and 0 <= r0 < P.T and r0 + a.T <= P.T, 'row_w starts at the launch\'s first row, like the labels'
        seen.add(r0)
    assert seen == ({0, 64, 128} if rows else {0})
    for t in P.R:
        for a in (P._mse_args[t], P._vel_args[t]):
            assert isinstance(a, capi.STRUCTS['tfx_mse_w_args']) and a.row_w == P.lat[t]['w_row'].data_ptr() and a.R == P.R[t]
        assert isinstance(P._rec_args[t], capi.STRUCTS['tfx_mse_args'])
    # the per-step setters reach the new structs, set_rows the gather's count and the padding rows' weights
    P.set_ce_vocab(11); P.set_loss_scales(0.25, {t: 0.5 for t in P.R})
    assert all(a.V == 11 and a.grad_scale == 0.25 for a, _ in ces) and all(P._mse_args[t].grad_scale == 0.5 for t in P.R)
    for t in P.R:
        P.lat[t]['w_row'].fill_(3.)
    P.set_rows({t: r - 1 for t, r in P.R.items()})
    gathers = [i[1] for i in P.fwd if _name(i) == 'tfx_gather_f32']
    assert sorted(g[3] for g in gathers) == sorted(r - 1 for r in P.R.values()) and all(g[0] == P.w_inst.data_ptr() for g in gathers)
    assert all(P._mse_args[t].R == r - 1 and P._vel_args[t].R == r - 1 for t, r in P.R.items())
    assert all(float(P.lat[t]['w_row'][-1]) == 0. and float(P.lat[t]['w_row'][0]) == 3. for t in P.R), 'padding rows take weight 0'


def test_weighted_plan_under_frozen_sets_checkpointing_and_exchange_groups():
    m, ps, P = _cpu_plan(b=3, n=64, chunk_rows=64, weighted=True)
    full = [_name(i) for i in P.bwd]
    P.select_frozen(frozenset({'to_text_logits.weight'}))
    assert [_name(i) for i in P.bwd[:9]] == ['tfx_gemm_nt', 'tfx_ce_w_bwd', 'tfx_gemm_nt'] * 3
    P.set_loss_scales(0.5, {})
    P.select_frozen(frozenset())
    assert [_name(i) for i in P.bwd] == full and all(i[1].grad_scale == 0.5 for i in P.bwd if _name(i) == 'tfx_ce_w_bwd')
    _, _, C2 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True, weighted=True)
    _, _, C0 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True)
    assert C2.ckpt and C2._recompute == C0._recompute
    _, _, G = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2, weighted=True)
    _, _, H = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2)
    assert G.bwd_cuts == H.bwd_cuts and G.bwd_cuts


def test_plan_key_carries_the_presence_of_weights_never_their_values(monkeypatch):
    from transfusion_pytorch_amd import Transfusion
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
    torch.manual_seed(0)
    m = Transfusion(num_text_tokens=16, dim_latent=8, transformer=dict(dim=64, depth=1, heads=1))
    p0 = m._plan(2, 64, 0, {}, True, text_loss=True)
    pw = m._plan(2, 64, 0, {}, True, text_loss=True, weighted=True)
    assert p0.kw == {} and pw.kw == {'weighted': True} and pw is not p0
    assert m._plan(2, 64, 0, {}, True, text_loss=True, weighted=True) is pw and m._plan(2, 64, 0, {}, True, text_loss=True) is p0
    i0 = m._plan(2, 64, 0, {}, False, text_loss=True)
    assert m._plan(2, 64, 0, {}, False, text_loss=True, weighted=True) is i0, 'inference plans never look at the switch'
    assert len(made) == 3
