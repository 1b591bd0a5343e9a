"""Text loss terms - a z-loss and label smoothing in the native cross entropy (Transfusion.set_text_loss_terms_, engine.Plan `text_terms`, tfx_ce_reg_fwd_bwd /
tfx_ce_reg_fwd / tfx_ce_reg_bwd) - without a GPU: the float64 restatement the GPU tests hold the kernels to against torch's own cross entropy plus z *
logsumexp^2, the condition that the bounds cannot hide a dead term, the C ABI, the setter, the plan key, the copies, and the launch lists of real Plans built on
the CPU (nothing is launched)."""
import copy
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _text_loss_terms_cases as C                                   # noqa: E402

BOTH = [(c, s) for c in C.CASES for s in C.SETTINGS]
both_id = lambda v: C.case_id(v) if len(v) == 3 else C.setting_id(v)


def _model(depth=2):
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(0)
    return Transfusion(num_text_tokens=16, dim_latent=(32, 8), transformer=dict(dim=64, depth=depth, heads=1))


def _name(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


# ================================================================================================ the float64 restatement
@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_restatement_agrees_with_torch(case, setting):
    """sum over the valid rows of F.cross_entropy(label_smoothing=e) + z logsumexp^2, and its autograd gradient, in float64"""
    T, V, ld = case
    z, e = C.f32(setting[0]), C.f32(setting[1])
    lg, lab = C.inputs(T, V, ld)
    scale = 0.37 * 0.003
    r = C.reg_ref(lg, lab, V, *setting, scale)
    valid = lab >= 0
    x = torch.where(valid[:, None], lg[:, :V].double(), torch.zeros(T, V, dtype=torch.float64)).requires_grad_(True)
    lse = torch.logsumexp(x, dim=1)
    want = torch.nn.functional.cross_entropy(x, lab.long(), ignore_index=-1, reduction='sum', label_smoothing=e) + z * (lse[valid] ** 2).sum()
    (want * scale).backward()
    w = float(want.detach())
    assert abs(float(r.loss) - w) <= 1e-12 * max(1., abs(w))
    assert float((r.d - x.grad).abs().max()) <= 1e-14 * max(1., float(r.k.abs().max()))
    assert bool((r.d[~valid] == 0).all()) and bool((r.row[~valid] == 0).all())
    plain = C.ce_ref(lg, lab, V)
    assert abs(float(r.ce_sum) - float(plain.loss)) <= 1e-12 * abs(float(plain.loss)) and float(r.count) == float(valid.sum())
    assert abs(float(r.sq_sum) - float((lse.detach()[valid] ** 2).sum())) <= 1e-12 * float(r.sq_sum)
    tol_lse, tol_loss, tol_ce, tol_sq, tol_d = C.reg_bounds(r, scale)
    assert tol_d.shape == (T, V) and bool((tol_d[valid] > 0).all()) and bool((tol_d[~valid] == 0).all())
    # the bounds are about rounding: far below the quantities they bound
    assert float(tol_loss) <= 1e-3 * max(1., abs(float(r.loss))) and float(tol_sq) <= 1e-3 * float(r.sq_sum) and float(tol_ce) <= 1e-3 * abs(float(r.ce_sum))


def test_zero_weights_are_the_plain_restatement():
    T, V, ld = C.CASES[1]
    lg, lab = C.inputs(T, V, ld)
    r, b = C.reg_ref(lg, lab, V, 0., 0., 0.5), C.ce_ref(lg, lab, V, 0.5)
    assert torch.equal(r.d, b.d) and float(r.loss) == float(b.loss)


@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_bounds_cannot_hide_a_dead_term(case, setting):
    """under the NEW bounds a kernel that ignored the weights would be caught: every valid row has an element of the terms-off gradient more than 4 bounds from the
    terms-on reference, and the summed loss is more than 2 bounds away"""
    T, V, ld = case
    lg, lab = C.inputs(T, V, ld)
    scale = 0.0031
    r = C.reg_ref(lg, lab, V, *setting, scale)
    off = C.ce_ref(lg, lab, V, scale)
    _, tol_loss, _, _, tol_d = C.reg_bounds(r, scale)
    ratio = ((off.d - r.d).abs() / tol_d.clamp_min(1e-300))[r.valid].max(dim=1).values
    loss_ratio = abs(float(off.loss) - float(r.loss)) / float(tol_loss)
    print(f'  {C.case_id(case)} {C.setting_id(setting)}: per valid row the farthest element is {float(ratio.min()):.1f} .. {float(ratio.max()):.1f} bounds away; loss {loss_ratio:.1f} bounds')
    assert float(ratio.min()) > 4 and loss_ratio > 2


# ================================================================================================ the C ABI
REG = ('tfx_ce_reg_fwd_bwd', 'tfx_ce_reg_fwd', 'tfx_ce_reg_bwd')


def test_capi_tables_hold_the_new_entry_points():
    from transfusion_pytorch_amd import capi
    for fn in REG:
        assert capi.FUNCTIONS[fn] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        assert capi.ENUMS['TFX_OP_' + fn[4:].upper()] > capi.ENUMS['TFX_OP_CE_BWD']
    ops = [v for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_')]
    assert len(ops) == len(set(ops)), 'two launch-list ops share a code'
    extra = ['z_weight', 'smoothing', 'aux']
    for plain, reg in (('tfx_ce_args', 'tfx_ce_reg_args'), ('tfx_ce_chunk_args', 'tfx_ce_reg_chunk_args')):
        assert capi.STRUCT_FIELDS[reg] == capi.STRUCT_FIELDS[plain] + [('z_weight', ctypes.c_float), ('smoothing', ctypes.c_float), ('aux', ctypes.c_void_p)], reg
    # the plain entry points, their structs and codes are what they were
    assert [n for n, _ in capi.STRUCT_FIELDS['tfx_ce_args']] == ['T', 'V', 'logits', 'ld', 'labels', 'grad_scale', 'dlogits', 'ld_d', 'acc']
    assert (capi.ENUMS['TFX_OP_CE_FWD_BWD'], capi.ENUMS['TFX_OP_CE_FWD'], capi.ENUMS['TFX_OP_CE_BWD']) == (18, 31, 54)
    assert extra == [n for n, _ in capi.STRUCT_FIELDS['tfx_ce_reg_args']][-3:]


def test_library_exports_the_entry_points_and_the_version_tag():
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    for fn in REG:
        assert getattr(lib, fn) is not None
    v = lib.tfx_version()
    assert b'-textreg' in v and v.endswith(b'-textreg-frozen') and v.index(b'-odeab') < v.index(b'-textreg')


def test_host_checks_return_before_any_launch():
    """host logic only: every pointer below is host memory no kernel could touch, so a launch would fault - NULL args, bad weights, bad strides, missing buffers
    return -1; T == 0 is a no-op"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    nan, inf = float('nan'), float('inf')
    weights = (dict(z_weight=-1e-4), dict(z_weight=nan), dict(z_weight=inf), dict(smoothing=-0.1), dict(smoothing=1.0), dict(smoothing=1.5), dict(smoothing=nan))
    ok = dict(T=2, V=10, logits=base, ld=16, labels=base, lse=base, acc=base, grad_scale=1.0, scale_dev=None, dlogits=base, ld_d=16, z_weight=1e-4, smoothing=0.1, aux=base)
    mk = lambda **kw: ctypes.byref(capi.make_args('tfx_ce_reg_chunk_args', **dict(ok, **kw)))
    for fn in (lib.tfx_ce_reg_fwd, lib.tfx_ce_reg_bwd):
        assert fn(None, None) == -1
        assert fn(mk(T=0), None) == 0
        for bad in weights + (dict(ld=12), dict(V=0), dict(V=17), dict(logits=base + 4), dict(T=-1), dict(logits=None), dict(labels=None), dict(lse=None)):
            assert fn(mk(**bad), None) == -1, bad
        assert fn(mk(T=0, z_weight=-1.0), None) == -1, 'bad weights are refused whatever the row count'
    for bad in (dict(ld_d=12), dict(ld_d=8), dict(dlogits=base + 8), dict(dlogits=None)):
        assert lib.tfx_ce_reg_bwd(mk(**bad), None) == -1, bad
    for bad in (dict(acc=None), dict(aux=None)):
        assert lib.tfx_ce_reg_fwd(mk(**bad), None) == -1, bad
    okf = dict(T=2, V=10, logits=base, ld=16, labels=base, grad_scale=1.0, dlogits=base, ld_d=16, acc=base, z_weight=1e-4, smoothing=0.1, aux=base)
    mf = lambda **kw: ctypes.byref(capi.make_args('tfx_ce_reg_args', **dict(okf, **kw)))
    assert lib.tfx_ce_reg_fwd_bwd(None, None) == -1 and lib.tfx_ce_reg_fwd_bwd(mf(T=0), None) == 0
    for bad in weights + (dict(T=-1), dict(V=0), dict(V=17), dict(ld_d=8), dict(logits=None), dict(labels=None), dict(dlogits=None), dict(acc=None), dict(aux=None)):
        assert lib.tfx_ce_reg_fwd_bwd(mf(**bad), None) == -1, bad


def test_run_list_and_fingerprint_know_the_new_ops():
    """tfx_run_list forwards the three codes (T = 0: the entry points return before a launch) and tfx_list_fingerprint hashes their structs - the new fields too"""
    from transfusion_pytorch_amd import capi
    from transfusion_pytorch_amd.engine import LaunchList
    a = capi.make_args('tfx_ce_reg_args', T=0, z_weight=1e-4, smoothing=0.1)
    c = capi.make_args('tfx_ce_reg_chunk_args', T=0, z_weight=1e-4, smoothing=0.1)
    L = LaunchList([('tfx_ce_reg_fwd_bwd', a), ('tfx_ce_reg_fwd', c), ('tfx_ce_reg_bwd', c)])
    failed = ctypes.c_int32(-1)
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == 0 and failed.value == -1
    c.smoothing = 1.0
    assert capi.lib().tfx_run_list(L.native(), len(L), None, ctypes.byref(failed)) == -1 and failed.value == 1
    c.smoothing = 0.1

    def fp():
        out = ctypes.c_int64()
        assert capi.lib().tfx_list_fingerprint(L.native(), len(L), ctypes.byref(out)) == 0
        return out.value
    f0 = fp()
    a.z_weight = 2e-4
    f1 = fp()
    c.aux = 64
    assert len({f0, f1, fp()}) == 3


# ================================================================================================ the setter, the plan key, the copies
def test_default_is_off_and_the_setter_validates():
    m = _model()
    assert (m.text_z_loss_weight, m.text_label_smoothing) == (0., 0.) and m.text_loss_terms() is None
    assert m.set_text_loss_terms_(z_loss=1e-4, label_smoothing=0.1) is m
    assert (m.text_z_loss_weight, m.text_label_smoothing) == (1e-4, 0.1)
    assert m.set_text_loss_terms_(1, 0).text_z_loss_weight == 1.0 and isinstance(m.text_z_loss_weight, float)       # ints are numbers
    m.set_text_loss_terms_(1e-4, 0.1)
    for bad in (dict(z_loss=-1e-9), dict(z_loss=float('nan')), dict(z_loss=float('inf')), dict(label_smoothing=-0.1), dict(label_smoothing=1.0),
                dict(label_smoothing=1.5), dict(label_smoothing=float('nan')), dict(label_smoothing=float('inf'))):
        with pytest.raises(ValueError):
            m.set_text_loss_terms_(**bad)
    for bad in (True, False, '0.1', None, (0.1,), [0.1], torch.tensor(0.1)):
        with pytest.raises(TypeError):
            m.set_text_loss_terms_(z_loss=bad)
        with pytest.raises(TypeError):
            m.set_text_loss_terms_(label_smoothing=bad)
    assert (m.text_z_loss_weight, m.text_label_smoothing) == (1e-4, 0.1)          # a refused call changes nothing
    assert m.set_text_loss_terms_() is m and (m.text_z_loss_weight, m.text_label_smoothing) == (0., 0.)
    for name in ('text_z_loss_weight', 'text_label_smoothing'):
        with pytest.raises(AttributeError):
            setattr(m, name, 0.5)                                             # read-only


def test_copies_carry_the_setting_and_state_dict_does_not():
    m = _model().set_text_loss_terms_(1e-4, 0.1)
    for c in (copy.deepcopy(m), m._clone_architecture(), m.create_ema().ema_model):
        assert (c.text_z_loss_weight, c.text_label_smoothing) == (1e-4, 0.1)
    assert copy.deepcopy(_model()).text_z_loss_weight == 0.
    assert set(m.state_dict()) == set(_model().state_dict())
    fresh = _model()
    fresh.load_state_dict(m.state_dict())
    assert (fresh.text_z_loss_weight, fresh.text_label_smoothing) == (0., 0.)


def test_plan_key_carries_the_pair_for_text_loss_training_plans_only(monkeypatch):
    """`_plan` with the Plan class stubbed out: a text-loss training plan of each pair has a key of its own; inference plans and training plans of calls without a
    text loss (forward_modality) do not depend on it - and with both weights zero Plan is called exactly as before (no new keyword)"""
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
    m.set_text_loss_terms_(1e-4, 0.)
    pz = m._plan(2, 64, 0, {}, True, text_loss=True)
    assert pz is not p_plain and pz.kw == {'text_terms': (1e-4, 0.)}
    assert m._plan(2, 64, 0, {}, False, text_loss=True) is i_plain    # inference: the setting is not looked at
    assert m._plan(2, 64, 2, {0: 128}, True) is f_plain               # a training plan without a text loss neither
    m.set_text_loss_terms_(1e-4, 0.1)
    pze = m._plan(2, 64, 0, {}, True, text_loss=True)
    assert pze is not pz and pze.kw == {'text_terms': (1e-4, 0.1)}
    m.set_text_head_chunking_(64)
    pc = m._plan(2, 64, 0, {}, True, text_loss=True)
    assert pc.kw == {'chunk_rows': 64, 'text_terms': (1e-4, 0.1)}
    m.set_text_head_chunking_(None)
    assert len(m._plans) == 6 and len(made) == 6
    m.set_text_loss_terms_(0., 0.)
    assert m._plan(2, 64, 0, {}, True, text_loss=True) is p_plain and len(made) == 6


# ================================================================================================ plans built on the CPU
def _cpu_plan(**kw):
    from _plan_digest import cpu_plan
    return cpu_plan(depth=2, **kw)


def test_zero_weights_build_the_plans_they_always_built():
    from _plan_digest import digest
    _, _, A = _cpu_plan(b=3, n=64)
    for tt in (None, (0., 0.)):
        _, _, B = _cpu_plan(b=3, n=64, text_terms=tt)
        assert digest(B) == digest(A) and B.reg is None and B.aux is None and B.nbytes == A.nbytes and B.acc.numel() == A.acc.numel()
    _, _, I = _cpu_plan(b=3, n=64, text_terms=(1e-4, 0.1), training=False)
    assert I.reg is None and I.aux is None, 'an inference plan never looks at the terms'


@pytest.mark.parametrize('rows', [None, 64], ids=['whole_head', 'rows64'])
def test_plan_with_terms_swaps_the_cross_entropy_launches_and_nothing_else(rows):
    from transfusion_pytorch_amd import capi
    kw = dict(chunk_rows=rows) if rows else {}
    _, _, Q = _cpu_plan(b=3, n=64, **kw)
    m, ps, P = _cpu_plan(b=3, n=64, text_terms=(1e-4, 0.1), **kw)
    assert P.reg == (1e-4, 0.1) and Q.reg is None
    swap = lambda n: n.replace('tfx_ce_', 'tfx_ce_reg_')
    for name in ('fwd', 'bwd'):
        assert [_name(i) for i in getattr(P, name)] == [swap(_name(i)) for i in getattr(Q, name)], name
    assert (P.fwd_embed_end, P.fwd_logits_end, P.fwd_pred_end, P.bwd_cuts, P.bwd_end) == (Q.fwd_embed_end, Q.fwd_logits_end, Q.fwd_pred_end, Q.bwd_cuts, Q.bwd_end)
    assert P.fwd.meta == Q.fwd.meta and P.bwd.meta == Q.bwd.meta
    # acc keeps its layout; aux sits behind it in the same buffer, so one memset zeroes both
    assert P.acc.numel() == Q.acc.numel() and P.aux.numel() == 2 and P.aux.data_ptr() == P.acc.data_ptr() + 4 * P.acc.numel() and P.nbytes == Q.nbytes + 8
    P.acc.fill_(3.); P.aux.fill_(5.)
    P.zero_acc()
    assert not bool(P.acc.any()) and not bool(P.aux.any())
    Q.acc.fill_(3.); Q.zero_acc()
    assert not bool(Q.acc.any())
    ces = [i[1] for L in (P.fwd, P.bwd) for i in L if _name(i).startswith('tfx_ce_reg_')]
    assert len(ces) == (6 if rows else 1)
    z32, e32 = ctypes.c_float(1e-4).value, ctypes.c_float(0.1).value
    for a in ces:
        assert isinstance(a, capi.STRUCTS['tfx_ce_reg_chunk_args' if rows else 'tfx_ce_reg_args'])
        assert (a.z_weight, a.smoothing, a.aux, a.acc) == (z32, e32, P.aux.data_ptr(), P.acc.data_ptr())
    # the per-step setters reach the new structs
    P.set_ce_vocab(11); P.set_loss_scales(0.25, {})
    assert all(a.V == 11 and a.grad_scale == 0.25 for a in ces)
    # the plain plan's cross-entropy structs and the new ones agree field for field in what they share
    qs = [i[1] for L in (Q.fwd, Q.bwd) for i in L if _name(i).startswith('tfx_ce_')]
    Q.set_ce_vocab(11); Q.set_loss_scales(0.25, {})
    for a, q in zip(ces, qs):
        for f, _ in capi.STRUCT_FIELDS[type(q).__name__]:
            if f not in ('logits', 'labels', 'lse', 'acc', 'scale_dev', 'dlogits'):
                assert getattr(a, f) == getattr(q, f), f


def test_terms_under_frozen_sets_checkpointing_and_exchange_groups():
    """the `_reg` launches are ordinary list items: a frozen text head drops the chunk's weight-gradient product and keeps the rest, the setters reach the kept
    lists of other frozen sets, a checkpointed plan keeps its recompute segments, the exchange cuts are the plain plan's"""
    tt = (1e-4, 0.1)
    m, ps, P = _cpu_plan(b=3, n=64, chunk_rows=64, text_terms=tt)
    full = [_name(i) for i in P.bwd]
    P.select_frozen(frozenset({'to_text_logits.weight'}))
    assert [_name(i) for i in P.bwd[:9]] == ['tfx_gemm_nt', 'tfx_ce_reg_bwd', 'tfx_gemm_nt'] * 3
    P.set_loss_scales(0.5, {})
    P.select_frozen(frozenset())
    assert [_name(i) for i in P.bwd] == full and all(i[1].grad_scale == 0.5 for i in P.bwd if _name(i) == 'tfx_ce_reg_bwd')
    P.select_frozen(frozenset(ps.params))
    assert P.bwd_end == 0
    _, _, W = _cpu_plan(b=3, n=64, text_terms=tt)
    W.select_frozen(frozenset({'to_text_logits.weight'}))
    assert [_name(i) for i in W.fwd].count('tfx_ce_reg_fwd_bwd') == 1
    _, _, C2 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True, text_terms=tt)
    _, _, C0 = _cpu_plan(b=3, n=64, chunk_rows=64, ckpt=True)
    assert C2.ckpt and C2._recompute == C0._recompute and [_name(i) for i in C2.bwd[:4]] == ['tfx_gemm_nt', 'tfx_ce_reg_bwd', 'tfx_gemm_tn', 'tfx_gemm_nt']
    _, _, G = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2, text_terms=tt)
    _, _, H = _cpu_plan(b=3, n=64, chunk_rows=64, dp_groups=2)
    assert G.bwd_cuts == H.bwd_cuts and G.bwd_cuts
