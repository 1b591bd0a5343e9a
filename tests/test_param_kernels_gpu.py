"""Every parameter-side entry point through the C ABI, per element, against the float64 references, derived bounds and guard bands of tests/_param_cases.py
(whose CPU test shows what this catches that the whole-tensor ratio of tests/test_kernels_gpu.py does not): tfx_colsum_bf16 in both kernel forms with row and
column maps (-1 entries included), tfx_muon_prep / _norm / _apply over one table of eight matrices, tfx_sumsq / tfx_sumsq_det up to the second trip of the
grid-stride loop, tfx_cast_rows / _t, tfx_ema_update, tfx_scale_bf16_dev, tfx_noise_mix, tfx_fourier, tfx_scatter_rows_bf16, and the empty / refused calls.
Every test prints `BOUND <form> <output> <worst error / bound>` lines: profiles/param_side_bounds.txt is a copy of them."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from transfusion_pytorch_amd import capi  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _param_cases as C  # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def report(form, rep):
    for name, v in rep.items():
        print(f'BOUND {form:<44s} {name:<22s} {v:.3f}')


def upd(rep, name, v):
    rep[name] = max(rep.get(name, 0.), v)


def rc_of(fn, *a):
    return getattr(capi.lib(), fn)(*a)


# ---------------------------------------------------------------------------------------------- colsum
def run_colsum(c):
    capi.check(rc_of('tfx_colsum_bf16', c.src.data_ptr(), c.ld, c.R, c.C, capi.ptr(c.colmap), capi.ptr(c.rowmap), c.out.view.data_ptr(), stream()), 'tfx_colsum_bf16')
    sync()
    return C.check_out(f'colsum {c.form} R={c.R} C={c.C} ld={c.ld} maps={c.maps}', c.out)


@pytest.mark.parametrize('maps', C.COLSUM_MAPS)
@pytest.mark.parametrize('C_ld', C.COLSUM8_SHAPES + C.COLSUM_SCALAR_SHAPES, ids=lambda s: f'C{s[0]}-ld{s[1]}')
def test_colsum_bf16_maps_tails_and_row_blocks(C_ld, maps):
    """both kernels at every R of the list: a map entry of -1 adds nothing (the rows in front of the source hold 1e4), repeated rows count twice, two columns
    mapped to one output add up, a column mapped to -1 and a column whose sum is zero leave `out` bit-identical"""
    Cc, ld = C_ld
    rep = {}
    for R in C.COLSUM_R:
        c = C.build_colsum(R, Cc, ld, maps, DEV)
        assert c.form == ('colsum8_k' if Cc % 8 == 0 and ld % 8 == 0 else 'colsum_k')
        upd(rep, 'out', run_colsum(c))
    report(f'colsum_bf16 {c.form} C={Cc} ld={ld} {maps}', rep)


# ---------------------------------------------------------------------------------------------- Muon
_MUON = {}


def muon_case(zero_mat=None):
    if zero_mat not in _MUON:
        from transfusion_pytorch_amd.optim import _muon_device_tables
        c = C.build_muon(device=DEV, zero_mat=zero_mat)
        c.T = _muon_device_tables(c.H, DEV)
        _MUON[zero_mat] = c
    return _MUON[zero_mat]


def run_prep(c, o, g=None):
    ss = torch.tensor([o.clip['sumsq']], dtype=torch.float32, device=DEV)
    a = capi.make_args('tfx_muon_prep_args', mats=c.T.mats, blk_mat=c.T.blk_mat, nmat=c.nmat, nblk=c.nblk, g=c.g if g is None else g, buf=o.buf.view, ws=o.ws.view,
                       partials=o.partials.view, sumsq=ss, max_norm=o.clip['max_norm'], grad_scale=o.clip['grad_scale'], momentum=o.momentum, nesterov=int(o.nesterov))
    capi.call('tfx_muon_prep', a, stream()); sync()


def run_norm(c, partials, out, eps=C.MUON_EPS):
    capi.check(rc_of('tfx_muon_norm', c.T.mats.data_ptr(), c.nmat, partials.data_ptr(), float(eps), out.view.data_ptr(), stream()), 'tfx_muon_norm'); sync()


@pytest.mark.parametrize('nesterov', (False, True), ids=('plain', 'nesterov'))
@pytest.mark.parametrize('momentum', C.MUON_MOMENTA)
def test_muon_prep_and_norm_per_element(momentum, nesterov):
    """one launch over eight matrices (ragged, flipped, one row, one column, 272 blocks) at flat offsets with gaps, under every clip setting: buf, both bf16
    copies, the padding (zero stays zero, poison stays poison), the gaps of g and buf, partials per block, then tfx_muon_norm on those partials"""
    c = muon_case()
    rep = {}
    for k, clip in enumerate(C.MUON_CLIPS):
        label = f'muon_prep mu={momentum} nesterov={nesterov} {clip}'
        o = C.muon_prep_outs(c, momentum, nesterov, clip, ws_poison=bool(k % 2))
        g0 = c.g.clone()
        run_prep(c, o)
        assert torch.equal(C._bits(c.g), C._bits(g0)), 'the gradient buffer was written'
        for out in (o.buf, o.ws, o.partials):
            upd(rep, out.name, C.check_out(label, out))
        s, t = o.ws.view[0, c.ps], o.ws.view[0, c.pt]
        assert torch.equal(C._bits(s), C._bits(t)), f'{label}: the transposed copy differs from the straight one in {int((C._bits(s) != C._bits(t)).sum())} elements'
        # against what torch.optim.Muon executes: fp32 torch.lerp on the CPU
        ub, uu = C.ulps(o.buf.view[0, c.fi], o.lerp_buf), C.ulps(s.float(), o.lerp_u.to(BF).float())
        print(f'{label}: buf vs torch.lerp worst {float(ub.max()):.2f} ulp; bf16(u) differs from bf16(torch.lerp) in {int((uu > 0).sum())} of {uu.numel()} elements')
        upd(rep, 'buf / 2 ulp of lerp', float(ub.max()) / 2)
        assert float(ub.max()) <= 2, f'{label}: buf is {float(ub.max())} ulp from torch.lerp'
        # u itself is seen only through its bf16 copy: an fp32 value within 2 ulp of torch's rounds to a bf16 within u16 + 4 u32 of torch's value
        near = (s.double() - o.lerp_u.double()).abs() <= (C.U16 + 4 * C.U32) * o.lerp_u.double().abs() + 2.0 ** -133
        assert bool(near.all()), f'{label}: bf16(u) is further from torch.lerp than its rounding in {int((~near).sum())} elements'
        nrm = C.muon_norm_out(c, o.partials.view[0].clone())
        run_norm(c, o.partials.view[0].clone(), nrm)
        upd(rep, 'inv', C.check_out(label + ' norm', nrm))
    report(f'muon_prep mu={momentum} {"nesterov" if nesterov else "plain"}', rep)


def test_muon_norm_of_an_all_zero_matrix_and_the_stride_loop():
    """a matrix with zero gradient and momentum: partials 0, inv = 1 / eps and 1 / eps^2; the 272-block matrix runs muon_norm's loop a second trip"""
    c = muon_case(zero_mat=1)
    o = C.muon_prep_outs(c, 0.95, True, C.MUON_CLIPS[0])
    run_prep(c, o)
    rep = C.check_outs('muon_prep zero matrix', [o.buf, o.ws, o.partials])
    m = c.H['mats'][1]
    assert float(o.partials.view[0, m['blk0']:m['blk0'] + m['prep_blocks']].abs().max()) == 0
    p = o.partials.view[0].clone()
    nrm = C.muon_norm_out(c, p)
    run_norm(c, p, nrm)
    rep['inv'] = C.check_out('muon_norm zero matrix', nrm)
    eps = C.f32(C.MUON_EPS)
    assert abs(float(nrm.view[0, 2]) * eps - 1) < 1e-6 and abs(float(nrm.view[0, 3]) * eps * eps - 1) < 1e-6
    assert c.H['mats'][-1]['prep_blocks'] == 272
    report('muon_norm zero matrix / 272 blocks', rep)


@pytest.mark.parametrize('decay', (1., 1 - 0.02 * 0.1), ids=('decay1', 'decay<1'))
def test_muon_apply_reads_the_straight_copy(decay):
    """p = p decay - lr ratio O with a distinct lr ratio per shape; the two copies in `ws` hold independent patterns; the gaps of p stay bit-identical"""
    c = muon_case()
    assert len({m['lr_ratio'] for m in c.H['mats']}) == c.nmat
    o = C.muon_apply_out(c, 0.02, decay)
    ws0 = c.ws_apply.clone()
    a = capi.make_args('tfx_muon_apply_args', mats=c.T.mats, blk_mat=c.T.blk_mat, nmat=c.nmat, nblk=c.nblk, p=o.view, ws=c.ws_apply, lr=o.lr, decay=o.decay)
    capi.call('tfx_muon_apply', a, stream()); sync()
    assert torch.equal(C._bits(c.ws_apply), C._bits(ws0))
    report(f'muon_apply decay={decay:g}', {'p': C.check_out(f'muon_apply decay={decay}', o)})


def test_newton_schulz_with_an_all_zero_matrix_among_others():
    from transfusion_pytorch_amd.optim import newton_schulz
    g = C.gen(5, 20)
    mats = [torch.randn(r, cc, generator=g).to(DEV) for r, cc in ((64, 64), (130, 40), (40, 130))]
    zero = torch.zeros(65, 63, device=DEV)
    a = newton_schulz(mats)
    b = newton_schulz([mats[0], zero, mats[1], mats[2]])
    sync()
    assert b[1].shape == (65, 63) and bool(torch.isfinite(b[1].float()).all()) and int((b[1] != 0).sum()) == 0
    for x, y in zip(a, [b[0], b[2], b[3]]):
        assert bool(torch.isfinite(x.float()).all()) and torch.equal(C._bits(x), C._bits(y))


# ---------------------------------------------------------------------------------------------- sumsq
@pytest.mark.parametrize('n', C.SUMSQ_N)
def test_sumsq_accumulates_and_sumsq_det_overwrites(n):
    c = C.build_sumsq(n, DEV)
    capi.check(rc_of('tfx_sumsq', c.g.data_ptr(), n, c.out.view.data_ptr(), stream()), 'tfx_sumsq')
    part = torch.full((capi.ENUMS['TFX_SUMSQ_DET_PARTIALS'],), float('nan'), device=DEV)
    capi.check(rc_of('tfx_sumsq_det', c.g.data_ptr(), n, part.data_ptr(), c.det.view.data_ptr(), stream()), 'tfx_sumsq_det'); sync()
    rep = C.check_outs(f'sumsq n={n}', [c.out, c.det])
    first = c.det.view.clone()
    C._bits(c.det.view).fill_(C.FILL_F32)
    capi.check(rc_of('tfx_sumsq_det', c.g.data_ptr(), n, part.data_ptr(), c.det.view.data_ptr(), stream()), 'tfx_sumsq_det'); sync()
    assert torch.equal(C._bits(c.det.view), C._bits(first)), 'tfx_sumsq_det differs between two runs'
    report(f'sumsq n={n}', rep)


# ---------------------------------------------------------------------------------------------- casts
@pytest.mark.parametrize('transposed', (False, True), ids=('cast_rows', 'cast_rows_t'))
@pytest.mark.parametrize('Rs,Cs', C.CAST_SHAPES)
def test_cast_rows_are_exact_copies(Rs, Cs, transposed):
    """bit-equal to torch's rounding; rows mapped to -1 or past the source, columns past Cs / Cd and the padding up to ld_dst are zero; guards intact; the source
    starts at an odd float offset and has 1e4 behind it"""
    for use_map in (False, True):
        for cd in ('lt', 'gt'):
            c = C.build_cast(Rs, Cs, use_map, cd, transposed, DEV)
            assert c.src.data_ptr() % 16 == 12 and c.Rd % 32 and c.ld % 32
            a = capi.make_args('tfx_cast_args', src=c.src, ld_src=Cs, Rs=Rs, Cs=Cs, rowmap=capi.ptr(c.rowmap), dst=c.out.view, ld_dst=c.ld, Rd=c.Rd, Cd=c.Cd)
            capi.call('tfx_cast_rows_t' if transposed else 'tfx_cast_rows', a, stream()); sync()
            assert C.check_out(f'cast t={transposed} {Rs}x{Cs} map={use_map} Cd={c.Cd}', c.out) == 0


# ---------------------------------------------------------------------------------------------- ema / scale
@pytest.mark.parametrize('decay', C.EMA_DECAYS)
def test_ema_update_tails_and_guards(decay):
    rep = {}
    for n in C.VEC_N:
        c = C.build_ema(n, decay, DEV)
        capi.check(rc_of('tfx_ema_update', c.out.view.data_ptr(), c.online.data_ptr(), n, c.decay, stream()), 'tfx_ema_update'); sync()
        upd(rep, 'ema', C.check_out(f'ema n={n} decay={decay}', c.out))
        if decay == 0:
            assert torch.equal(C._bits(c.out.view[0]), C._bits(c.online)), 'decay 0 must copy `online`'
    report(f'ema_update decay={decay:g}', rep)


@pytest.mark.parametrize('scale', C.SCALES, ids=('one', 'third', 'minus2'))
def test_scale_bf16_dev_tails_and_guards(scale):
    rep = {}
    for n in C.VEC_N:
        c = C.build_scale(n, scale, DEV, specials=(scale == 1.))
        capi.check(rc_of('tfx_scale_bf16_dev', c.out.view.data_ptr(), n, c.scale.data_ptr(), stream()), 'tfx_scale_bf16_dev'); sync()
        if scale == 1.:
            assert torch.equal(C._bits(c.out.buf), C._bits(c.out.before)), 'a scale of 1 must keep every bit'
        else:
            upd(rep, 'x', C.check_out(f'scale n={n} s={scale}', c.out))
    report(f'scale_bf16_dev s={scale:g}', rep)


# ---------------------------------------------------------------------------------------------- noise mix / fourier / scatter
def noise_args(c, eps=True, flow=True):
    return capi.make_args('tfx_noise_mix_args', R=c.R, dl=c.dl, x=c.x, eps=c.eps if eps else None, row_inst=c.row_inst, inst_time=c.times, xt=c.xt.view,
                          ld_xt=c.ld_xt, flow=c.flow.view if flow else None)


@pytest.mark.parametrize('R,dl,ld', C.NOISE_SHAPES)
def test_noise_mix(R, dl, ld):
    """t = 0 and t = 1 rows are bit-equal to bf16(eps) / bf16(x) (their bound is 0), pad columns zero; eps = NULL copies x and leaves `flow` alone; flow = NULL"""
    rep = {}
    c = C.build_noise(R, dl, ld, DEV)
    assert bool((c.times[c.row_inst.long()] == 0).any()) and (R < 3 or bool((c.times[c.row_inst.long()] == 1).any()))
    capi.call('tfx_noise_mix', noise_args(c), stream()); sync()
    upd(rep, 'xt', C.check_out(f'noise_mix R={R} dl={dl}', c.xt))
    assert C.check_out('noise_mix flow', c.flow) == 0
    c = C.build_noise(R, dl, ld, DEV)
    c.flow.mask[:] = False
    capi.call('tfx_noise_mix', noise_args(c, flow=False), stream()); sync()
    upd(rep, 'xt', C.check_out(f'noise_mix flow=NULL R={R}', c.xt))
    C.check_out('noise_mix flow=NULL', c.flow)
    c = C.build_noise(R, dl, ld, DEV, with_eps=False)
    capi.call('tfx_noise_mix', noise_args(c, eps=False), stream()); sync()
    assert C.check_out(f'noise_mix eps=NULL R={R}', c.xt) == 0
    C.check_out('noise_mix eps=NULL flow', c.flow)
    report(f'noise_mix R={R} dl={dl} ld={ld}', rep)


@pytest.mark.parametrize('I,half,ld', C.FOURIER_SHAPES)
def test_fourier(I, half, ld):
    c = C.build_fourier(I, half, ld, DEV)
    a = capi.make_args('tfx_fourier_args', I=I, half=half, times=c.times, w=c.w, out=c.out.view, ld=ld)
    capi.call('tfx_fourier', a, stream()); sync()
    report(f'fourier I={I} half={half} ld={ld}', {'out': C.check_out(f'fourier I={I} half={half}', c.out)})


@pytest.mark.parametrize('cols', C.SCATTER_COLS)
def test_scatter_rows_bf16(cols):
    c = C.build_scatter(cols, DEV)
    capi.check(rc_of('tfx_scatter_rows_bf16', c.src.data_ptr(), c.ld_src, cols, c.out.view.data_ptr(), c.ld_dst, c.rowmap.data_ptr(), c.R, stream()), 'scatter'); sync()
    assert C.check_out(f'scatter cols={cols}', c.out) == 0
    for bad in (cols + 4, 12):
        before = c.out.buf.clone()
        assert rc_of('tfx_scatter_rows_bf16', c.src.data_ptr(), c.ld_src, bad, c.out.view.data_ptr(), c.ld_dst, c.rowmap.data_ptr(), c.R, stream()) == -1
        sync()
        assert torch.equal(C._bits(c.out.buf), C._bits(before))


# ---------------------------------------------------------------------------------------------- empty and refused calls
def test_empty_calls_return_0_and_write_nothing_and_misaligned_pointers_are_refused():
    L, s = capi.lib(), stream()
    poison = torch.empty(4096, device=DEV)
    C._bits(poison).fill_(C.FILL_F32)
    before = poison.clone()
    P = poison.data_ptr()
    pb = poison.view(torch.int32).view(torch.float32)
    c = C.build_colsum(9, 8, 8, 'none', DEV)
    assert L.tfx_colsum_bf16(c.src.data_ptr(), 8, 0, 8, None, None, P, s) == 0 and L.tfx_colsum_bf16(c.src.data_ptr(), 8, 9, 0, None, None, P, s) == 0
    assert L.tfx_sumsq(P + 1024, 0, P, s) == 0
    assert L.tfx_sumsq_det(P + 1024, 0, P + 64, P, s) == 0                       # n = 0: the sum of nothing
    sync()
    assert float(poison[0]) == 0.
    C._bits(poison).fill_(C.FILL_F32)
    assert L.tfx_ema_update(P, P + 1024, 0, 0.5, s) == 0 and L.tfx_scale_bf16_dev(P, 0, P + 1024, s) == 0
    for fn, kw in (('tfx_cast_rows', dict(Rd=0, ld_dst=8, Cd=8)), ('tfx_cast_rows', dict(Rd=4, ld_dst=0, Cd=0)),
                   ('tfx_cast_rows_t', dict(Rd=0, ld_dst=8, Cd=8)), ('tfx_cast_rows_t', dict(Rd=4, ld_dst=0, Cd=0))):
        a = capi.make_args('tfx_cast_args', src=P + 1024, ld_src=4, Rs=4, Cs=4, dst=P, **kw)
        assert getattr(L, fn)(ctypes.byref(a), s) == 0, (fn, kw)
    a = capi.make_args('tfx_noise_mix_args', R=0, dl=4, x=P + 1024, eps=P + 2048, row_inst=P + 3072, inst_time=P + 3072, xt=P, ld_xt=8, flow=P)
    assert L.tfx_noise_mix(ctypes.byref(a), s) == 0
    a = capi.make_args('tfx_fourier_args', I=0, half=4, times=P + 1024, w=P + 1024, out=P, ld=16)
    assert L.tfx_fourier(ctypes.byref(a), s) == 0
    assert L.tfx_scatter_rows_bf16(P + 1024, 8, 8, P, 8, P + 2048, 0, s) == 0
    m = muon_case()
    a = capi.make_args('tfx_muon_prep_args', mats=m.T.mats, blk_mat=m.T.blk_mat, nmat=0, nblk=0, g=P, buf=P, ws=P, partials=P, max_norm=0., grad_scale=1., momentum=0.9)
    assert L.tfx_muon_prep(ctypes.byref(a), s) == 0
    assert L.tfx_muon_norm(m.T.mats.data_ptr(), 0, P, 1e-7, P, s) == 0
    a = capi.make_args('tfx_muon_apply_args', mats=m.T.mats, blk_mat=m.T.blk_mat, nmat=0, nblk=0, p=P, ws=P, lr=0.1, decay=1.)
    assert L.tfx_muon_apply(ctypes.byref(a), s) == 0
    # misaligned pointers (the kernels issue 16-byte accesses)
    assert L.tfx_sumsq_det(P + 4, 8, P + 64, P, s) == -1 and L.tfx_sumsq(P + 4, 8, P, s) == -1
    assert L.tfx_ema_update(P + 4, P + 1024, 8, 0.5, s) == -1 and L.tfx_ema_update(P, P + 1028, 8, 0.5, s) == -1
    sync()
    assert torch.equal(C._bits(pb), C._bits(before)), 'an empty or refused call wrote something'
