"""Every token-wise kernel form of csrc/tokenwise.hip through the C ABI, per element, against the float64 references, derived bounds and guard bands of
tests/_tokenwise_cases.py (whose CPU test shows what this catches that the whole-tensor ratio of tests/test_kernels_gpu.py does not).  The test ids name the
paths: the widths 8 / 520 / 1032 (partly filled chunks) and 2048 (NC = 4, with the per-token fallback of the input side's segment forms), the second trip of
every capped grid-stride loop and of every segment form, the RoPE carry, balance=True segments with a 1030-token instance, stored against added table gradients,
tfx_layer_end_fwd with save / err, AttentionResidual at L = 33 / 64, mean / rstd, and the epsilon rows.  Every test prints `BOUND <form> <output> <worst error / bound>`
lines: profiles/tokenwise_bounds.txt is a copy of them."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from transfusion_pytorch_amd import capi  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tokenwise_cases as C  # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16
W = C.WIDTHS
wid = lambda d: f'd{d}' + {8: '-one_lane', 520: '-NC2_one_lane_in_chunk2', 1032: '-NC4_two_empty_chunks', 2048: '-NC4'}.get(d, '')


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def report(form, rep):
    for name, v in rep.items():
        print(f'BOUND {form:<44s} {name:<22s} {v:.3f}')


def seg_kw(c, on=True):
    return dict(seg_start=c.seg_start, seg_len=c.seg_len, n_seg=c.lay.n_seg) if on else {}


def pre_fwd_args(c, o):
    return capi.make_args('tfx_adaln_pre_args', T=c.T, d=c.d, x=c.x, u=o.u.view, tok_inst=c.tok, table=c.table, ld_table=c.ld, gamma_text=c.gamma_text,
                          mean=o.mean.view, rstd=o.rstd.view)


def pre_bwd_args(c, o, seg, use_add=False):
    return capi.make_args('tfx_adaln_pre_args', T=c.T, d=c.d, x=c.x, tok_inst=c.tok, table=c.table, ld_table=c.ld, gamma_text=c.gamma_text, mean=c.mean32, rstd=c.rstd32,
                          du=c.du, dx=o.dx.view, dtable=o.dtable.view, dgamma_text=o.dgamma_text.view, dx_add=c.add if use_add else None, **seg_kw(c, seg))


def post_args(c, out=None, o=None, seg=False, g=None, dtable=None, dbias=True):
    kw = dict(T=c.T, d=c.d, x=c.x, y=c.y, tok_inst=c.tok, table=c.table.data_ptr() + 4 * c.post_col0, ld_table=c.ld, layerscale=c.layerscale)
    if out is not None:
        kw.update(out=out)
    if o is not None:
        kw.update(g=c.g if g is None else g, dy=o.dy.view, dtable=(o.dtable.view if dtable is None else dtable).data_ptr() + 4 * c.post_col0,
                  dlayerscale=o.dlayerscale.view, dbias=o.dbias.view if dbias else None, **seg_kw(c, seg))
    return capi.make_args('tfx_adaln_post_args', **kw)


def call2(fn, a, b):
    capi.check(getattr(capi.lib(), fn)(ctypes.byref(a), ctypes.byref(b) if b is not None else None, stream()), fn)


# ---------------------------------------------------------------------------------------------- AdaLN, per-token forms at every width
@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_pre_fwd_u_mean_rstd(d):
    rep = {}
    for T in C.TOKENS:
        c = C.build_adaln(C.layout('scatter', T), d, DEV)
        o = C.outs_pre_fwd(c)
        capi.call('tfx_adaln_pre_fwd', pre_fwd_args(c, o), stream()); sync()
        C.check_outs(f'adaln_pre_fwd T={T} d={d}', [o.u, o.mean, o.rstd], rep)
    report(f'adaln_pre_fwd {wid(d)}', rep)


@pytest.mark.parametrize('d', (8, 64, 520, 1032), ids=wid)
def test_adaln_pre_epsilon_rows(d):
    """rows scaled by 2^-8 (variance about 1.5e-5: without the + 1e-5 their rstd is off by 30 %) and constant rows (variance 0: rstd = 1e-5 ** -0.5, u = beta or 0),
    forward and both backward forms"""
    rep = {}
    c = C.build_adaln(C.layout('runs', 130), d, DEV, eps_rows=True)
    var = c.x.double().var(-1, unbiased=False)
    assert float(c.rstd_ref.max()) > 316.2 and float(var[2]) == 0 and 0.8e-5 < float(var[1]) < 3e-5
    o = C.outs_pre_fwd(c)
    capi.call('tfx_adaln_pre_fwd', pre_fwd_args(c, o), stream()); sync()
    C.check_outs(f'adaln_pre_fwd eps rows d={d}', [o.u, o.mean, o.rstd], rep)
    for seg in (False, True):
        stored = seg and d <= 1024
        o = C.outs_pre_bwd(c, stored)
        capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o, seg), stream()); sync()
        C.check_outs(f'adaln_pre_bwd eps rows d={d} seg={seg}', [o.dx, o.dtable, o.dgamma_text], rep)
    report(f'adaln_pre eps_rows {wid(d)}', rep)


@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_pre_bwd_per_token_atomics_add_to_the_table(d):
    rep = {}
    for T in C.TOKENS:
        c = C.build_adaln(C.layout('scatter', T), d, DEV)
        for use_add in (False, True):
            o = C.outs_pre_bwd(c, False, use_add)
            capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o, False, use_add), stream()); sync()
            C.check_outs(f'adaln_pre_bwd per token T={T} d={d} dx_add={use_add}', [o.dx, o.dtable, o.dgamma_text], rep)
    report(f'adaln_pre_bwd per-token {wid(d)}', rep)


@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_post_fwd(d):
    rep = {}
    for T in C.TOKENS:
        c = C.build_adaln(C.layout('scatter', T), d, DEV)
        o = C.outs_post_fwd(c)
        capi.call('tfx_adaln_post_fwd', post_args(c, out=o.out.view), stream()); sync()
        C.check_outs(f'adaln_post_fwd T={T} d={d}', [o.out], rep)
    report(f'adaln_post_fwd {wid(d)}', rep)


@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_post_bwd_per_token_atomics_add_to_the_table(d):
    rep = {}
    for T in C.TOKENS:
        c = C.build_adaln(C.layout('scatter', T), d, DEV)
        o = C.outs_post_bwd(c, False)
        capi.call('tfx_adaln_post_bwd', post_args(c, o=o), stream()); sync()
        C.check_outs(f'adaln_post_bwd per token T={T} d={d}', [o.dy, o.dtable, o.dlayerscale, o.dbias], rep)
    report(f'adaln_post_bwd per-token {wid(d)}', rep)


# ---------------------------------------------------------------------------------------------- AdaLN, segment forms
SEG_LAYOUTS = [('runs', T) for T in C.TOKENS] + [('model', 0), ('all_text', 0), ('all_mod', 0), ('one_seg', 0)]


def _segment_layouts(d, balance):
    for kind, T in SEG_LAYOUTS:
        if kind == 'model' and d > 1032:
            continue                                   # (the 1030-token instance runs at every width up to 1032: NC = 1, 2 and 4)
        yield kind, C.layout(kind, T, balance=balance)


@pytest.mark.parametrize('balance', (False, True), ids=('balance=False', 'balance=True'))
@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_pre_bwd_segments_store_the_table_gradient(d, balance):
    """the segment form stores an instance's gradient into a table prefilled with the guard pattern (pad columns, the z columns and absent instances untouched);
    d > 1024 takes the per-token fallback, whose atomics add onto the finite initial values.  Against the float64 reference AND the per-token form."""
    rep = {}
    stored = d <= 1024
    for kind, lay in _segment_layouts(d, balance):
        c = C.build_adaln(lay, d, DEV)
        for use_add in (False, True):
            o = C.outs_pre_bwd(c, stored, use_add)
            capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o, True, use_add), stream()); sync()
            C.check_outs(f'adaln_pre_bwd segments {kind} T={c.T} d={d} dx_add={use_add}', [o.dx, o.dtable, o.dgamma_text], rep)
        o2 = C.outs_pre_bwd(c, False, True)
        capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o2, False, True), stream()); sync()
        C.check_outs(f'adaln_pre_bwd per token {kind} T={c.T} d={d}', [o2.dx, o2.dtable, o2.dgamma_text])
    report(f'adaln_pre_bwd segments{"" if stored else " (per-token fallback)"} {wid(d)} balance={balance}', rep)


@pytest.mark.parametrize('balance', (False, True), ids=('balance=False', 'balance=True'))
@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_post_bwd_segments_store_the_table_gradient(d, balance):
    """the output side's segment form exists at every width (NC = 4: one token per trip, 64 KiB of static LDS)"""
    rep = {}
    for kind, lay in _segment_layouts(d, balance):
        c = C.build_adaln(lay, d, DEV)
        o = C.outs_post_bwd(c, True)
        capi.call('tfx_adaln_post_bwd', post_args(c, o=o, seg=True), stream()); sync()
        C.check_outs(f'adaln_post_bwd segments {kind} T={c.T} d={d}', [o.dy, o.dtable, o.dlayerscale, o.dbias], rep)
    report(f'adaln_post_bwd segments {wid(d)} balance={balance}', rep)


def _fused_pre_post(c, fused, rep=None, label=''):
    """tfx_adaln_pre_post_bwd (or its two launches) on the 6d table: dx, dy, the shared table gradient, dgamma_text, dlayerscale against float64 - the output side's
    reference taken from the dx rows the launch stored"""
    stored = c.d <= 1024
    op, oq = C.outs_pre_bwd(c, stored), C.outs_post_bwd(c, True)
    a = pre_bwd_args(c, op, True)
    b = post_args(c, o=oq, seg=True, g=op.dx.view, dtable=op.dtable.view, dbias=False)
    if fused:
        call2('tfx_adaln_pre_post_bwd', a, b)
    else:
        capi.call('tfx_adaln_pre_bwd', a, stream()); capi.call('tfx_adaln_post_bwd', b, stream())
    sync()
    C.refill_post_bwd(c, oq, True, op.dx.view)
    tab = C.merge_tables(op.dtable, oq.dtable)
    C.check_outs(label, [op.dx, oq.dy, tab, op.dgamma_text, oq.dlayerscale], rep)
    assert torch.equal(oq.dbias.buf, oq.dbias.before), 'dbias was not given'
    return op.dx.view, oq.dy.view, tab.view, op.dgamma_text.view, oq.dlayerscale.view


@pytest.mark.parametrize('balance', (False, True), ids=('balance=False', 'balance=True'))
@pytest.mark.parametrize('d', W, ids=wid)
def test_adaln_pre_post_bwd_fused_and_its_two_launches(d, balance):
    """both against the float64 reference; rows and stored gradients of the two equal to the bit, atomically accumulated vectors within their bounds.
    d > 1024: the fused entry itself falls back to the two launches (per-token input side)."""
    rep = {}
    for kind, lay in _segment_layouts(d, balance):
        c = C.build_adaln(lay, d, DEV, wrappers=2)
        two = _fused_pre_post(c, False, None, f'two launches {kind} T={c.T} d={d}')
        one = _fused_pre_post(c, True, rep, f'tfx_adaln_pre_post_bwd {kind} T={c.T} d={d}')
        assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1]), 'fused rows differ from the two launches'
        if d <= 1024:
            assert torch.equal(two[2], one[2]), 'fused table gradient differs from the two launches'
    report(f'adaln_pre_post_bwd fused {wid(d)} balance={balance}', rep)


# ---------------------------------------------------------------------------------------------- RMSNorm, embedding
@pytest.mark.parametrize('d', W, ids=wid)
def test_rmsnorm_fwd_bwd_with_an_all_zero_row(d):
    rep = {}
    for T in C.TOKENS:
        c = C.build_rmsnorm(T, d, DEV, zero_row=True)
        o = C.outs_rmsnorm(c)
        a = capi.make_args('tfx_rmsnorm_args', T=T, d=d, x=c.x, y=o.y.view, gamma=c.gamma, dy=c.dy, dx=o.dx.view, dgamma=o.dgamma.view)
        capi.call('tfx_rmsnorm_fwd', a, stream()); capi.call('tfx_rmsnorm_bwd', a, stream()); sync()
        C.check_outs(f'rmsnorm T={T} d={d}', [o.y, o.dx, o.dgamma], rep)
    report(f'rmsnorm {wid(d)}', rep)


@pytest.mark.parametrize('d', W, ids=wid)
def test_embedding_fwd_exact_bwd_per_element(d):
    """ids of -1 on modality rows, repeated ids; modality rows of x and the rows of unused ids in dtable come back bit-identical"""
    rep = {}
    for kind, T in (('scatter', 1), ('scatter', 3), ('runs', 130), ('scatter', 1001)):
        c = C.build_embed(C.layout(kind, T), d, 40, DEV)
        assert T < 3 or (int(c.ids.min()) == -1 and int(c.used.sum()) < 40)
        o = C.outs_embed(c)
        a = capi.make_args('tfx_embed_args', T=c.T, d=d, text_ids=c.ids, tok_inst=c.tok, table=c.table, x=o.x.view, dx=c.dx, dtable=o.dtable.view)
        capi.call('tfx_embed_fwd', a, stream()); capi.call('tfx_embed_bwd', a, stream()); sync()
        C.check_outs(f'embed {kind} T={T} d={d}', [o.x, o.dtable], rep)
    report(f'embed {wid(d)}', rep)


# ---------------------------------------------------------------------------------------------- AttentionResidual
def attnres_args(c, of=None, ob=None, first=0):
    kw = dict(T=c.T, d=c.d, L=c.L, hiddens=c.H, stride_h=c.T * c.d, gamma=c.gamma, pq=c.pq)
    if of is not None:
        kw.update(out=of.out.view, save=of.save.view, err=of.err.view)
    if ob is not None:
        kw.update(g=c.g, g2=None if first else c.g2, dhiddens=ob.dhiddens.view, stride_dh=c.T * c.d, first=first, dgamma=ob.dgamma.view, dpq=ob.dpq.view)
    return capi.make_args('tfx_attnres_args', **kw)


def _attnres_case(T, d, L, rep_f, rep_b, zero_row=True):
    c = C.build_attnres(T, d, L, DEV, zero_row=zero_row)
    of = C.outs_attnres_fwd(c)
    capi.call('tfx_attnres_fwd', attnres_args(c, of), stream()); sync()
    C.check_attnres_fwd(f'attnres_fwd T={T} d={d} L={L}', c, of, rep_f)
    for first in (0, 1):
        ob = C.outs_attnres_bwd(c, first)
        capi.call('tfx_attnres_bwd', attnres_args(c, ob=ob, first=first), stream()); sync()
        C.check_outs(f'attnres_bwd T={T} d={d} L={L} first={first}', [ob.dhiddens, ob.dgamma, ob.dpq], rep_b)


@pytest.mark.parametrize('d', W, ids=wid)
def test_attnres_fwd_save_err_and_push_bwd_at_every_width(d):
    rep_f, rep_b = {}, {}
    for T in C.TOKENS:
        _attnres_case(T, d, 3, rep_f, rep_b)
    report(f'attnres_fwd {wid(d)}', rep_f); report(f'attnres_bwd push {wid(d)}', rep_b)


@pytest.mark.parametrize('d', (64, 520, 1032), ids=wid)
@pytest.mark.parametrize('L', (1, 2, 5, 33, 64), ids=lambda L: f'L{L}')
def test_attnres_depths_up_to_64_lanes_of_saved_state(L, d):
    """lane l keeps the state of hidden l: L = 33 and 64 reach the upper half of the wave.  `save` per element (entry 3 written as 0), out + err against the exact mix,
    an all-zero hidden row (the max(norm, 1e-12) branch)"""
    rep_f, rep_b = {}, {}
    _attnres_case(37, d, L, rep_f, rep_b, zero_row=L > 1)
    report(f'attnres_fwd L={L} {wid(d)}', rep_f); report(f'attnres_bwd push L={L} {wid(d)}', rep_b)


# ---------------------------------------------------------------------------------------------- second trips of the grid-stride loops
@pytest.mark.parametrize('kernel,d', [('adaln_pre_bwd_k', 64), ('adaln_post_bwd_k', 64), ('rmsnorm_bwd_k', 64), ('attnres_bwd_k', 64), ('rmsnorm_bwd_k', 1032)])
def test_second_trip_of_the_capped_per_token_kernels(kernel, d):
    """grid_capped stops at 1024 blocks of 4 waves: T = 4101 sends five tokens through a second trip"""
    T, rep = 4101, {}
    if kernel.startswith('adaln'):
        c = C.build_adaln(C.layout('scatter', T), d, DEV)
        if kernel == 'adaln_pre_bwd_k':
            o = C.outs_pre_bwd(c, False)
            capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o, False), stream()); sync()
            C.check_outs(kernel, [o.dx, o.dtable, o.dgamma_text], rep)
        else:
            o = C.outs_post_bwd(c, False)
            capi.call('tfx_adaln_post_bwd', post_args(c, o=o), stream()); sync()
            C.check_outs(kernel, [o.dy, o.dtable, o.dlayerscale, o.dbias], rep)
    elif kernel == 'rmsnorm_bwd_k':
        c = C.build_rmsnorm(T, d, DEV)
        o = C.outs_rmsnorm(c)
        a = capi.make_args('tfx_rmsnorm_args', T=T, d=d, x=c.x, y=o.y.view, gamma=c.gamma, dy=c.dy, dx=o.dx.view, dgamma=o.dgamma.view)
        capi.call('tfx_rmsnorm_fwd', a, stream()); capi.call('tfx_rmsnorm_bwd', a, stream()); sync()
        C.check_outs(kernel, [o.y, o.dx, o.dgamma], rep)
    else:
        _attnres_case(T, d, 3, {}, rep, zero_row=False)
    report(f'{kernel} second trip T={T} d{d}', rep)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pull_case(c, D=2):
    """a stack of D AttentionResiduals over D + 1 hiddens on the tokens of the AdaLN case `c`; the forward kernels supply the saved state.  Returns what
    tfx_attnres_pull_bwd needs for hidden l = 1 (sources: every layer; src[0] = layer 0 forms its <g, out> here)."""
    T, d = c.T, c.d
    g = C.gen(T, d, D, 9)
    p = SimpleNamespace()
    p.H = C.rn(g, D + 1, T, d, scale=2.0, device=DEV)
    p.gm = (torch.randn(D, d, generator=g) * 0.3).to(DEV); p.pq = (torch.randn(D, d, generator=g) * 0.5).to(DEV)
    p.G = C.rn(g, D, T, d, device=DEV)
    p.outs = torch.zeros(D, T, d, device=DEV, dtype=BF); p.errs = torch.zeros(D, T, d, device=DEV, dtype=BF)
    p.saves = [torch.zeros(T, j + 2, 4, device=DEV) for j in range(D)]
    for j in range(D):
        a = capi.make_args('tfx_attnres_args', T=T, d=d, L=j + 2, hiddens=p.H, stride_h=T * d, gamma=p.gm[j], pq=p.pq[j], out=p.outs[j], save=p.saves[j], err=p.errs[j])
        capi.call('tfx_attnres_fwd', a, stream())
    sync()
    p.own = [p.outs[j].double() + p.errs[j].double() for j in range(D)]
    p.dsum = torch.stack([(p.G[j].double() * p.own[j]).sum(-1) for j in range(D)]).float()
    p.wtab = torch.zeros(2, D, d, device=DEV)
    p.dgm = torch.zeros(D, d, device=DEV); p.dpq = torch.zeros(D, d, device=DEV)
    SRC = capi.STRUCTS['tfx_attnres_src']
    recs = (SRC * D)()
    for j in range(D):
        for k, v in dict(g=p.G[j], save=p.saves[j], dsum=p.dsum[j], w=p.wtab[0, j], dw=p.wtab[1, j], gamma=p.gm[j], pq=p.pq[j], dgamma=p.dgm[j], dpq=p.dpq[j]).items():
            setattr(recs[j], k, v.data_ptr())
        recs[j].L = j + 2
    p.tab = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(recs), ctypes.sizeof(recs))), dtype=torch.uint8).to(DEV)
    capi.check(capi.lib().tfx_attnres_prep(p.tab.data_ptr(), D, d, stream()), 'prep'); sync()
    return p


@pytest.mark.parametrize('form', ['adaln_pre_bwd_seg_k', 'adaln_post_bwd_seg_k', 'adaln_pre_post_bwd_seg_k', 'attnres_pull_reg_k'])
def test_second_segment_of_a_wave_in_the_segment_forms(form):
    """seg_grid caps at the resident blocks (at most 4 of 512 threads per CU): with 8 * 4 * CUs + 100 segments a wave takes a second segment"""
    n_seg = 8 * 4 * _cus() + 100
    d, rep = 64, {}
    lay = C.layout('many', balance=True, n_seg=n_seg)
    assert lay.n_seg == n_seg and set(lay.seg_len.tolist()) == set(range(1, 10)) and 35000 < lay.T < 50000
    c = C.build_adaln(lay, d, DEV, wrappers=2 if form == 'adaln_pre_post_bwd_seg_k' else 1)
    if form == 'adaln_pre_bwd_seg_k':
        o = C.outs_pre_bwd(c, True, True)
        capi.call('tfx_adaln_pre_bwd', pre_bwd_args(c, o, True, True), stream()); sync()
        C.check_outs(form, [o.dx, o.dtable, o.dgamma_text], rep)
    elif form == 'adaln_post_bwd_seg_k':
        o = C.outs_post_bwd(c, True)
        capi.call('tfx_adaln_post_bwd', post_args(c, o=o, seg=True), stream()); sync()
        C.check_outs(form, [o.dy, o.dtable, o.dlayerscale, o.dbias], rep)
    elif form == 'adaln_pre_post_bwd_seg_k':
        _fused_pre_post(c, True, rep, form)
    else:
        p = _pull_case(c)
        dh = C.new_out('dh', c.T, d, BF, DEV)
        oq = C.outs_post_bwd(c, True)
        a = capi.make_args('tfx_attnres_pull_args', T=c.T, d=d, l=1, n_src=2, h=p.H[1], src=p.tab.data_ptr(), out_own=p.outs[0], out_err=p.errs[0], dh=dh.view, **seg_kw(c))
        b = post_args(c, o=oq, seg=True, g=dh.view)
        call2('tfx_attnres_pull_bwd', a, b); sync()
        dh.ref, dh.tol, dws, dw_tols = C.pull_ref(p.H[1], [p.G[0], p.G[1]], p.saves, 1, p.own, [p.wtab[0, 0], p.wtab[0, 1]])
        C.refill_post_bwd(c, oq, True, dh.view)
        C.check_outs(form, [dh, oq.dy, oq.dtable, oq.dlayerscale, oq.dbias], rep)
        for j in range(2):
            rep[f'dw[{j}]'] = C.assert_elementwise(f'{form} dw[{j}]', p.wtab[1, j][None], dws[j][None], dw_tols[j][None])
    report(f'{form} second segment n_seg={n_seg}', rep)


def test_attnres_pull_register_form_small_batches():
    """the register pull form with its fused output side on the model's segments (the 1030-token instance in one wave) and one token per wave"""
    rep = {}
    for kind, segs in (('model', True), ('runs', False)):
        c = C.build_adaln(C.layout(kind, 130, balance=True), 64, DEV)
        p = _pull_case(c)
        dh = C.new_out('dh', c.T, 64, BF, DEV)
        oq = C.outs_post_bwd(c, segs)
        a = capi.make_args('tfx_attnres_pull_args', T=c.T, d=64, l=1, n_src=2, h=p.H[1], src=p.tab.data_ptr(), out_own=p.outs[0], out_err=p.errs[0], dh=dh.view, **seg_kw(c, segs))
        call2('tfx_attnres_pull_bwd', a, post_args(c, o=oq, seg=segs, g=dh.view)); sync()
        dh.ref, dh.tol, _, _ = C.pull_ref(p.H[1], [p.G[0], p.G[1]], p.saves, 1, p.own, [p.wtab[0, 0], p.wtab[0, 1]])
        C.refill_post_bwd(c, oq, segs, dh.view)
        C.check_outs(f'pull {kind}', [dh, oq.dy, oq.dtable, oq.dlayerscale, oq.dbias], rep)
    report('attnres_pull_reg_k + output side', rep)


# ---------------------------------------------------------------------------------------------- QK-norm + RoPE
@pytest.mark.parametrize('T,H,carry', [(5500, 3, True), (1400, 12, True), (2100, 8, False), (131, 2, False)],
                         ids=['T5500-H3-second_trip_carry', 'T1400-H12-second_trip_carry', 'T2100-H8-second_trip_no_carry', 'T131-H2-one_trip'])
def test_qk_norm_rope_rows_and_gain_gradients(T, H, carry):
    """the backward caps at 256 blocks of 1024 threads (32768 vectors a trip); its incremental (t, rem) update carries when 32768 % 2H != 0"""
    assert C.rope_carries(T, H) == carry and (T * 2 * H > C.QK_STRIDE) == (T > 131)
    c = C.build_qk(T, H, DEV)
    o = C.outs_qk(c)
    a = capi.make_args('tfx_qk_norm_rope_args', T=T, H=H, qkv=c.qkv, ld_qkv=c.ld, qk=o.qk.view, ld_qk=c.ld_qk, gamma_q=c.gq, gamma_k=c.gk, rot_pos=c.pos, cos_tab=c.cos,
                       sin_tab=c.sin, q_scale=c.q_scale, dqk=c.dqk, ld_dqk=2 * c.HD, dqkv=o.dqkv.view, ld_dqkv=c.ld_qk, dgamma_q=o.dgamma_q.view, dgamma_k=o.dgamma_k.view)
    capi.call('tfx_qk_norm_rope_fwd', a, stream()); capi.call('tfx_qk_norm_rope_bwd', a, stream()); sync()
    rep = C.check_outs(f'qk_norm_rope T={T} H={H}', [o.qk, o.dqkv, o.dgamma_q, o.dgamma_k])
    report(f'qk_norm_rope T={T} H={H}', rep)


# ---------------------------------------------------------------------------------------------- fused decode launches
def _layer_end(T, d, L, with_pre, rep):
    """tfx_layer_end_fwd with save and err == tfx_adaln_post_fwd + tfx_attnres_fwd (same save, err) + tfx_adaln_pre_fwd bit for bit, mean / rstd included; the three
    launches are held to float64, each stage's reference taken from the bf16 row the stage before it stored"""
    c = C.build_adaln(C.layout('scatter', T), d, DEV)
    r = C.build_attnres(T, d, L, DEV)
    res = []
    for fused in (False, True):
        H = r.H.clone()
        op, of, oq = C.outs_post_fwd(c), C.outs_attnres_fwd(r), C.outs_pre_fwd(c)
        hid = C.new_out('hidden', L * T, d, BF, DEV, init=H)
        last = hid.view[(L - 1) * T:]
        post = post_args(c, out=last)
        ar = capi.make_args('tfx_attnres_args', T=T, d=d, L=L, hiddens=hid.view, stride_h=T * d, gamma=r.gamma, pq=r.pq, out=of.out.view, save=of.save.view, err=of.err.view)
        pre = capi.make_args('tfx_adaln_pre_args', T=T, d=d, x=of.out.view, u=oq.u.view, tok_inst=c.tok, table=c.table, ld_table=c.ld, gamma_text=c.gamma_text,
                             mean=oq.mean.view, rstd=oq.rstd.view)
        if fused:
            capi.check(capi.lib().tfx_layer_end_fwd(ctypes.byref(post), ctypes.byref(ar), ctypes.byref(pre) if with_pre else None, stream()), 'tfx_layer_end_fwd')
        else:
            capi.call('tfx_adaln_post_fwd', post, stream()); capi.call('tfx_attnres_fwd', ar, stream())
            if with_pre:
                capi.call('tfx_adaln_pre_fwd', pre, stream())
        sync()
        res.append((hid.buf.clone(), of.out.buf.clone(), of.save.buf.clone(), of.err.buf.clone(), oq.u.buf.clone(), oq.mean.buf.clone(), oq.rstd.buf.clone()))
        # float64, stage by stage
        hid.ref = torch.cat([H[:L - 1].double().reshape(-1, d), c.out_ref]); hid.tol = torch.cat([torch.zeros((L - 1) * T, d, dtype=torch.float64, device=DEV), c.out_tol])
        st = C.attnres_state(hid.view.reshape(L, T, d).double(), r.gamma, r.pq)
        of.out.ref, of.out.tol = st.out, C.tol_bf16(st.out, st.E_out)
        of.save.ref = torch.stack([st.a, st.inv, st.s, torch.zeros_like(st.s)], -1).permute(1, 0, 2).reshape(T, L * 4)
        of.save.tol = torch.stack([st.a * st.rel_a[None], C.E(d, st.inv), st.es, torch.zeros_like(st.s)], -1).permute(1, 0, 2).reshape(T, L * 4)
        r2 = SimpleNamespace(out_ref=st.out, sum_tol=st.E_out + C.U16 * C.U16 * st.out.abs())
        C.check_out(f'layer_end fused={fused} ({T}, {d}, {L})', hid)
        rr = C.check_attnres_fwd(f'layer_end fused={fused} ({T}, {d}, {L})', r2, of, rep if fused else None)
        if with_pre:
            oq.u.ref, oq.u.tol, oq.mean.ref, rs, _, _ = C.pre_fwd_ref(of.out.view, c.tok, c.table, c.gamma_text)
            oq.mean.tol, oq.rstd.ref, oq.rstd.tol = C.E(d, of.out.view.double().abs().mean(-1)), rs, C.E(d, rs)
            C.check_outs(f'layer_end fused={fused} ({T}, {d}, {L})', [oq.u, oq.mean, oq.rstd], rep if fused else None)
        else:
            for o in (oq.u, oq.mean, oq.rstd):
                assert torch.equal(o.buf, o.before), 'no input side was given'
    for name, x, y in zip(('hidden L-1', 'out', 'save', 'err', 'u', 'mean', 'rstd'), *res):
        assert torch.equal(x, y), f'tfx_layer_end_fwd ({T}, {d}, {L}) pre={with_pre}: {name} differs from the three launches'


@pytest.mark.parametrize('with_pre', (True, False), ids=('with_pre', 'without_pre'))
@pytest.mark.parametrize('T,d,L', [(130, 520, 9), (64, 1032, 33), (300, 512, 3)])
def test_layer_end_fwd_with_save_and_err_equals_three_launches(T, d, L, with_pre):
    rep = {}
    _layer_end(T, d, L, with_pre, rep)
    report(f'layer_end_fwd save+err ({T}, {d}, {L}) pre={int(with_pre)}', rep)


@pytest.mark.parametrize('d', W, ids=wid)
def test_layer_end_and_post_pre_fwd_at_every_width(d):
    rep = {}
    _layer_end(131, d, 3, True, rep)
    report(f'layer_end_fwd {wid(d)}', rep)
    # tfx_adaln_post_pre_fwd == tfx_adaln_post_fwd + tfx_adaln_pre_fwd, bit for bit; both within the bounds (the input side from the stored row)
    c = C.build_adaln(C.layout('scatter', 131), d, DEV)
    res, rep = [], {}
    for fused in (False, True):
        op, oq = C.outs_post_fwd(c), C.outs_pre_fwd(c)
        post = post_args(c, out=op.out.view)
        pre = capi.make_args('tfx_adaln_pre_args', T=c.T, d=d, x=op.out.view, u=oq.u.view, tok_inst=c.tok, table=c.table, ld_table=c.ld, gamma_text=c.gamma_text,
                             mean=oq.mean.view, rstd=oq.rstd.view)
        if fused:
            call2('tfx_adaln_post_pre_fwd', post, pre)
        else:
            capi.call('tfx_adaln_post_fwd', post, stream()); capi.call('tfx_adaln_pre_fwd', pre, stream())
        sync()
        oq.u.ref, oq.u.tol, oq.mean.ref, rs, _, _ = C.pre_fwd_ref(op.out.view, c.tok, c.table, c.gamma_text)
        oq.mean.tol, oq.rstd.ref, oq.rstd.tol = C.E(d, op.out.view.double().abs().mean(-1)), rs, C.E(d, rs)
        C.check_outs(f'post_pre fused={fused} d={d}', [op.out, oq.u, oq.mean, oq.rstd], rep if fused else None)
        res.append((op.out.buf.clone(), oq.u.buf.clone(), oq.mean.buf.clone(), oq.rstd.buf.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y), 'tfx_adaln_post_pre_fwd differs from the two launches'
    report(f'adaln_post_pre_fwd {wid(d)}', rep)


# ---------------------------------------------------------------------------------------------- refused arguments
@pytest.mark.parametrize('d', (12, 2056), ids=('d_not_a_multiple_of_8', 'd_over_2048'))
def test_unsupported_widths_are_refused(d):
    """d % 8 != 0 or d > 2048 returns -1 from every entry that dispatches on the width, before anything is launched"""
    lib, s = capi.lib(), stream()
    t = torch.zeros(64, device=DEV)
    pre = capi.make_args('tfx_adaln_pre_args', T=4, d=d, seg_start=t, seg_len=t, n_seg=1)
    post = capi.make_args('tfx_adaln_post_args', T=4, d=d, seg_start=t, seg_len=t, n_seg=1)
    ar = capi.make_args('tfx_attnres_args', T=4, d=d, L=1, hiddens=t, out=t)
    for fn, a in (('tfx_adaln_pre_fwd', pre), ('tfx_adaln_pre_bwd', pre), ('tfx_adaln_post_fwd', post), ('tfx_adaln_post_bwd', post), ('tfx_attnres_fwd', ar), ('tfx_attnres_bwd', ar),
                  ('tfx_rmsnorm_fwd', capi.make_args('tfx_rmsnorm_args', T=4, d=d)), ('tfx_rmsnorm_bwd', capi.make_args('tfx_rmsnorm_args', T=4, d=d)),
                  ('tfx_embed_fwd', capi.make_args('tfx_embed_args', T=4, d=d)), ('tfx_embed_bwd', capi.make_args('tfx_embed_args', T=4, d=d))):
        assert getattr(lib, fn)(ctypes.byref(a), s) == -1, fn
    pre.n_seg = post.n_seg = 0
    for fn, a in (('tfx_adaln_pre_bwd', pre), ('tfx_adaln_post_bwd', post)):
        assert getattr(lib, fn)(ctypes.byref(a), s) == -1, fn + ' (per token)'
    post.out = pre.x = t.data_ptr()
    assert lib.tfx_adaln_post_pre_fwd(ctypes.byref(post), ctypes.byref(pre), s) == -1
    assert lib.tfx_layer_end_fwd(ctypes.byref(post), ctypes.byref(ar), None, s) == -1
    sync()


def test_attnres_depth_over_64_and_pull_width_over_1024_are_refused():
    lib, s = capi.lib(), stream()
    t = torch.zeros(64, device=DEV)
    ar = capi.make_args('tfx_attnres_args', T=4, d=64, L=65, hiddens=t, out=t)
    assert lib.tfx_attnres_fwd(ctypes.byref(ar), s) == -2 and lib.tfx_attnres_bwd(ctypes.byref(ar), s) == -2
    post = capi.make_args('tfx_adaln_post_args', T=4, d=64, out=t.data_ptr() + 64 * 4 * 64 * 2)
    assert lib.tfx_layer_end_fwd(ctypes.byref(post), ctypes.byref(ar), None, s) == -2
    for d in (1032, 2048):
        pull = capi.make_args('tfx_attnres_pull_args', T=4, d=d, l=1, n_src=2, h=t, src=t, dh=t, k1=t, ld_k1=8)
        assert lib.tfx_attnres_pull_bwd(ctypes.byref(pull), None, s) == -6, d
    sync()
