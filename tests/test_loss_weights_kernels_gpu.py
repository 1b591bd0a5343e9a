"""The loss-weight kernels on the GPU - tfx_ce_w_fwd / tfx_ce_w_bwd / tfx_ce_w_fwd_bwd / tfx_mse_w_fwd_bwd (include/tfx.h tfx_ce_w_args, tfx_mse_w_args) - on
the six shapes of the chunked head's tests and the MSE shapes of tests/_decode_loss_cases.py, under (z, e) in {(0, 0)} + the text-loss-term settings and the four
weight patterns of tests/_loss_weight_cases.py (restatements and bounds there):
  all ones    d logits, lse and d pred bit-equal to the unweighted entry points
  binary      d logits and lse bit-equal to the unweighted kernel run with the zero-weight labels set to -1; acc[1] exactly the count
  uniform     every element within the `_reg` bound scaled by the row's weight; acc and aux within the bound of a weighted sum of as many terms
  all zero    acc and aux untouched, outputs exact zeros."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_weight_cases as C                                         # noqa: E402
import _text_loss_terms_cases as R                                     # noqa: E402
import test_text_head_gpu as TH                                        # noqa: E402  (_written, sync, _stream)
from _decode_loss_cases import CLEAN_EPS, MSE_SHAPES, mse_inputs       # noqa: E402
from _gemm_cases import BF, assert_elementwise, assert_untouched, guarded          # noqa: E402

DEV = 'cuda'
sync, _stream = TH.sync, TH._stream
BOTH = [(c, s) for c in R.CASES for s in C.SETTINGS]
FUSED_BOTH = [(c, s) for c in R.FUSED_CASES for s in C.SETTINGS]
both_id = lambda v: R.case_id(v) if len(v) == 3 else R.setting_id(v)
GS = 0.0031


@functools.lru_cache(maxsize=None)
def _kcase(case):
    T, V, ld = case
    return R.inputs(T, V, ld, DEV)


def _w(case, pattern):
    return C.weights(case[0], pattern, seed=case[1]).to(DEV)


def _sums():
    acc = torch.tensor(R.ACC_INIT + (9.0, 9.0), device=DEV, dtype=torch.float32)
    aux = torch.tensor(R.AUX_INIT + (7.0, 7.0), device=DEV, dtype=torch.float32)
    return acc, aux


def _chunk_args(kind, case, setting, lg, lab, lse, acc, aux, dl=None, scale_dev=None, row_w=None):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    extra = dict(row_w=row_w) if kind == 'w' else {}
    return capi.make_args(f'tfx_ce_{kind}_chunk_args', T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, grad_scale=GS, scale_dev=scale_dev, dlogits=dl, ld_d=ld,
                          z_weight=setting[0], smoothing=setting[1], aux=aux, **extra)


def _chunk_run(kind, case, setting, lg, lab, row_w=None, scale_dev=None):
    """forward then backward of the chunk pair `kind` ('w' | 'reg'): (lse buffer, lse, d logits buffer, d logits, acc, aux)"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lbuf, lse = guarded(T, 1, torch.float32, DEV, 0)
    dbuf, dl = guarded(T, ld, BF, DEV, 0)
    acc, aux = _sums()
    a = _chunk_args(kind, case, setting, lg, lab, lse, acc, aux, dl, scale_dev, row_w)
    capi.call(f'tfx_ce_{kind}_fwd', a, _stream())
    capi.call(f'tfx_ce_{kind}_bwd', a, _stream())
    sync()
    return lbuf, lse, dbuf, dl, acc, aux


def _fused_run(kind, case, setting, lg, lab, row_w=None):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    dbuf, dl = guarded(T, ld, BF, DEV, 0)
    acc, aux = _sums()
    extra = dict(row_w=row_w) if kind == 'w' else {}
    capi.call(f'tfx_ce_{kind}_fwd_bwd', capi.make_args(f'tfx_ce_{kind}_args', T=T, V=V, logits=lg, ld=ld, labels=lab, grad_scale=GS, dlogits=dl, ld_d=ld, acc=acc,
                                                       z_weight=setting[0], smoothing=setting[1], aux=aux, **extra), _stream())
    sync()
    return dbuf, dl, acc, aux


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _check_sums(what, acc, aux, r, tols, binary=False):
    got = [float(acc[0].double()), float(acc[1].double()), float(aux[0].double()), float(aux[1].double())]
    want = [R.ACC_INIT[0] + float(r.loss), R.ACC_INIT[1] + float(r.wsum), R.AUX_INIT[0] + float(r.ce_sum), R.AUX_INIT[1] + float(r.sq_sum)]
    ratios = [abs(g - w) / float(t) for g, w, t in zip(got, want, tols[1:5])]
    print(f'  {what}: acc {got[0]:.6f} {got[1]:.6f} aux {got[2]:.6f} {got[3]:.6f}; error / bound ' + ' '.join(f'{x:.3f}' for x in ratios))
    assert max(ratios) <= 1, (what, got, want, ratios)
    if binary:
        assert got[1] == want[1], 'weights in {0, 1}: acc[1] is exactly the count'
    assert acc[2:].tolist() == [9.0, 9.0] and aux[2:].tolist() == [7.0, 7.0]


@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_chunk_pair_all_ones_and_binary_are_the_unweighted_bits(case, setting):
    T, V, ld = case
    lg, lab = _kcase(case)
    sd = torch.tensor([0.37, 55.0], device=DEV, dtype=torch.float32)
    _, lse0, _, dl0, acc0, aux0 = _chunk_run('reg', case, setting, lg, lab, scale_dev=sd)
    _, lse1, _, dl1, acc1, aux1 = _chunk_run('w', case, setting, lg, lab, _w(case, 'ones'), scale_dev=sd)
    assert torch.equal(_bits(lse1), _bits(lse0)) and torch.equal(_bits(dl1), _bits(dl0)), 'all ones: the `_reg` kernels\' lse and d logits to the bit'
    assert float(acc1[1]) == float(acc0[1])
    w = _w(case, 'binary')
    lab_b = torch.where(w == 0, torch.full_like(lab, -1), lab)
    assert bool(((w == 0) & (lab >= 0)).any()) or T < 8
    _, lse0, _, dl0, acc0, aux0 = _chunk_run('reg', case, setting, lg, lab_b, scale_dev=sd)
    lg_nan = torch.where((w == 0)[:, None], torch.full_like(lg, float('nan')), lg)            # a zero-weight row is not read
    lbuf, lse1, dbuf, dl1, acc1, aux1 = _chunk_run('w', case, setting, lg_nan, lab, w, scale_dev=sd)
    assert torch.equal(_bits(lse1), _bits(lse0)) and torch.equal(_bits(dl1), _bits(dl0)), 'binary: the `_reg` kernels on labels set to -1, to the bit'
    assert float(acc1[1]) == R.ACC_INIT[1] + int(((w != 0) & (lab >= 0)).sum()) == float(acc0[1])
    r = C.ce_w_ref(lg, lab, w, V, *setting, 1.0)
    _check_sums(f'binary {R.case_id(case)} {R.setting_id(setting)}', acc1, aux1, r, C.ce_w_bounds(r, 1.0), binary=True)


@pytest.mark.parametrize('scale_dev', [None, 0.37], ids=['no_scale_dev', 'scale_dev_0.37'])
@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_chunk_pair_uniform_weights_against_float64(case, setting, scale_dev):
    T, V, ld = case
    lg, lab = _kcase(case)
    w = _w(case, 'uniform')
    sd = None if scale_dev is None else torch.tensor([scale_dev, 55.0], device=DEV, dtype=torch.float32)
    scale = float(torch.tensor(GS, dtype=torch.float32).double()) * (1.0 if sd is None else float(sd[0].double()))
    r = C.ce_w_ref(lg, lab, w, V, *setting, scale)
    tols = C.ce_w_bounds(r, scale)
    lbuf0, _ = guarded(T, 1, torch.float32, DEV, 0)
    dbuf0, _ = guarded(T, ld, BF, DEV, 0)
    lg_nan = torch.where((w == 0)[:, None], torch.full_like(lg, float('nan')), lg)
    lbuf, lse, dbuf, dl, acc, aux = _chunk_run('w', case, setting, lg_nan, lab, w, scale_dev=sd)
    worst_l = assert_elementwise(f'tfx_ce_w_fwd {case} lse', lse.double(), r.lse[:, None], tols[0][:, None], tile=(4, 1))
    assert bool((lse[~r.valid] == 0).all()), 'ignored rows get lse 0'
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tols[5]
    worst_d = assert_elementwise(f'tfx_ce_w_bwd {case} {setting} dlogits', dl.double(), ref, tol, tile=(4, 512))
    assert not bool(_bits(dl[:, V:]).any()) and not bool(_bits(dl[~r.valid]).any()), 'pad columns and ignored rows: zero bits'
    assert_untouched(f'tfx_ce_w_fwd {case} lse', lbuf, lbuf0, TH._written(lbuf, T))
    assert_untouched(f'tfx_ce_w_bwd {case} dlogits', dbuf, dbuf0, TH._written(dbuf, T))
    print(f'  {R.case_id(case)} {R.setting_id(setting)} scale_dev {scale_dev}: worst error / bound lse {worst_l:.3f} d logits {worst_d:.3f}')
    _check_sums(f'uniform {R.case_id(case)} {R.setting_id(setting)}', acc, aux, r, tols)


@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_all_zero_weights_leave_the_sums_untouched_and_write_zeros(case, setting):
    """every row has weight 0 and every logit is NaN: nothing is read, nothing is added, the outputs are zero bits - the fused kernel included"""
    T, V, ld = case
    _, lab = _kcase(case)
    lg = torch.full((T, ld), float('nan'), device=DEV)
    lbuf0, _ = guarded(T, 1, torch.float32, DEV, 0)
    dbuf0, _ = guarded(T, ld, BF, DEV, 0)
    lbuf, lse, dbuf, dl, acc, aux = _chunk_run('w', case, setting, lg, lab, _w(case, 'zeros'))
    assert acc.tolist() == list(R.ACC_INIT) + [9.0, 9.0] and aux.tolist() == list(R.AUX_INIT) + [7.0, 7.0]
    assert not bool(_bits(lse).any()) and not bool(_bits(dl).any())
    assert_untouched('lse', lbuf, lbuf0, TH._written(lbuf, T)); assert_untouched('dlogits', dbuf, dbuf0, TH._written(dbuf, T))
    if case in R.FUSED_CASES:
        dbuf, dl, acc, aux = _fused_run('w', case, setting, lg, lab, _w(case, 'zeros'))
        assert acc.tolist() == list(R.ACC_INIT) + [9.0, 9.0] and aux.tolist() == list(R.AUX_INIT) + [7.0, 7.0] and not bool(_bits(dl).any())
        assert_untouched('fused dlogits', dbuf, dbuf0, TH._written(dbuf, T))


@pytest.mark.parametrize('case,setting', FUSED_BOTH, ids=both_id)
def test_fused_kernel_every_pattern(case, setting):
    """tfx_ce_w_fwd_bwd at the widths of both its paths (448: rows in registers, 1024: strided passes)"""
    T, V, ld = case
    lg, lab = _kcase(case)
    lg = torch.where(torch.isnan(lg), torch.zeros_like(lg), lg)             # (finite everywhere for the unweighted runs this one is compared with)
    poison = lambda w: torch.where((w == 0)[:, None], torch.full_like(lg, float('nan')), lg)      # a zero-weight row is not read: NaN there must not show
    _, dl0, acc0, _ = _fused_run('reg', case, setting, lg, lab)
    _, dl1, acc1, _ = _fused_run('w', case, setting, lg, lab, _w(case, 'ones'))
    assert torch.equal(_bits(dl1), _bits(dl0)) and float(acc1[1]) == float(acc0[1]), 'all ones: tfx_ce_reg_fwd_bwd\'s bits'
    w = _w(case, 'binary')
    _, dl0, acc0, _ = _fused_run('reg', case, setting, lg, torch.where(w == 0, torch.full_like(lab, -1), lab))
    assert bool(((w == 0) & (lab >= 0)).any()) or T < 8
    _, dl1, acc1, aux1 = _fused_run('w', case, setting, poison(w), lab, w)
    assert torch.equal(_bits(dl1), _bits(dl0)) and float(acc1[1]) == float(acc0[1]), 'binary: labels set to -1'
    assert bool(torch.isfinite(acc1).all()) and bool(torch.isfinite(aux1).all())
    w = _w(case, 'uniform')
    scale = float(torch.tensor(GS, dtype=torch.float32).double())
    r = C.ce_w_ref(lg, lab, w, V, *setting, scale)
    tols = C.ce_w_bounds(r, scale)
    dbuf0, _ = guarded(T, ld, BF, DEV, 0)
    dbuf, dl, acc, aux = _fused_run('w', case, setting, poison(w), lab, w)
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tols[5]
    worst = assert_elementwise(f'tfx_ce_w_fwd_bwd {case} {setting}', dl.double(), ref, tol, tile=(4, 512))
    assert not bool(_bits(dl[:, V:]).any()) and not bool(_bits(dl[~r.valid]).any())
    assert_untouched(f'tfx_ce_w_fwd_bwd {case} dlogits', dbuf, dbuf0, TH._written(dbuf, T))
    print(f'  {R.case_id(case)} {R.setting_id(setting)}: fused d logits worst error / bound {worst:.3f}')
    _check_sums(f'fused uniform {R.case_id(case)} {R.setting_id(setting)}', acc, aux, r, tols)


def test_null_row_w_returns_minus_one_before_any_launch():
    """every other pointer is NULL too: a launch would fault"""
    import ctypes
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    sp = ctypes.c_void_p(_stream())
    assert lib.tfx_ce_w_fwd(ctypes.byref(capi.make_args('tfx_ce_w_chunk_args', T=4, V=8, ld=8, ld_d=8)), sp) == -1
    assert lib.tfx_ce_w_bwd(ctypes.byref(capi.make_args('tfx_ce_w_chunk_args', T=4, V=8, ld=8, ld_d=8)), sp) == -1
    assert lib.tfx_ce_w_fwd_bwd(ctypes.byref(capi.make_args('tfx_ce_w_args', T=4, V=8, ld=8, ld_d=8)), sp) == -1
    assert lib.tfx_mse_w_fwd_bwd(ctypes.byref(capi.make_args('tfx_mse_w_args', R=4, dl=8, ld_pred=8, ld_d=64)), sp) == -1
    sync()


# ================================================================================================ the squared error
def _mse_run(fn, st, R_, dl, ldp, ldd, pred, flow, gs, old=None, **extra):
    from transfusion_pytorch_amd import capi
    pp = torch.full((R_, ldp), float('nan'), device=DEV); pp[:, :dl] = pred
    buf, dp = guarded(R_, ldd, BF, DEV, 0)
    if old is not None:
        dp.copy_(old)
    before = buf.clone()
    acc = torch.tensor([0.5, 9.0, 9.0, 9.0], device=DEV)
    capi.call(fn, capi.make_args(st, R=R_, dl=dl, pred=pp, ld_pred=ldp, flow=flow, grad_scale=gs, dpred=dp, ld_d=ldd, acc=acc, accumulate=int(old is not None), **extra), _stream())
    sync()
    assert_untouched(f'{fn} dpred', buf, before, TH._written(buf, R_))
    assert acc[1:].tolist() == [9.0, 9.0, 9.0]
    return dp, acc


@pytest.mark.parametrize('mode', ['plain', 'clean', 'plain_acc'])
@pytest.mark.parametrize('R_,dl,ldp,ldd', MSE_SHAPES)
def test_mse_w_every_pattern(R_, dl, ldp, ldd, mode):
    pred, flow, _, times, row_inst, _ = (t.to(DEV) for t in mse_inputs(R_, dl, seed=1))
    t_row = times[row_inst.long()]
    gs = 0.37
    clean = dict(row_inst=row_inst, inst_time=times, clean_eps=CLEAN_EPS) if mode == 'clean' else {}
    old = torch.randn(R_, ldd, generator=torch.Generator().manual_seed(9)).to(BF).to(DEV) if mode == 'plain_acc' else None
    ones = torch.ones(R_, device=DEV)
    dp0, acc0 = _mse_run('tfx_mse_fwd_bwd', 'tfx_mse_args', R_, dl, ldp, ldd, pred, flow, gs, old, **clean)
    dp1, acc1 = _mse_run('tfx_mse_w_fwd_bwd', 'tfx_mse_w_args', R_, dl, ldp, ldd, pred, flow, gs, old, row_w=ones, **clean)
    assert torch.equal(_bits(dp1), _bits(dp0)), 'all ones: tfx_mse_fwd_bwd\'s d pred to the bit'
    assert abs(float(acc1[0]) - float(acc0[0])) <= 1e-5 * float(acc0[0])
    w = C.weights(R_, 'uniform', seed=dl).to(DEV)
    pred_nan = torch.where((w == 0)[:, None], torch.full_like(pred, float('nan')), pred)          # a zero-weight row is not read
    dp, acc = _mse_run('tfx_mse_w_fwd_bwd', 'tfx_mse_w_args', R_, dl, ldp, ldd, pred_nan, flow, gs, old, row_w=w, **clean)
    loss, g = C.mse_w_ref(pred, flow, w, gs, t_row, CLEAN_EPS if mode == 'clean' else None)
    grown = float(acc[0].double()) - 0.5
    print(f'mse_w {mode} R {R_} dl {dl}: loss {float(loss):.6e}, acc grew by {grown:.6e} (rel {abs(grown - float(loss)) / float(loss):.2e})')
    assert abs(grown - float(loss)) <= 1e-5 * float(loss)
    oldv = old[:, :dl].double() if old is not None else torch.zeros_like(g)
    ref = g + oldv
    bound = 2. ** -8 * ref.abs() + 2. ** -22 * (g.abs() + oldv.abs())
    err = (dp[:, :dl].double() - ref).abs()
    print(f'mse_w {mode} R {R_} dl {dl}: worst d pred error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}')
    assert bool(torch.isfinite(dp[:, :dl].float()).all()) and bool((err <= bound).all()), float((err - bound).max())
    if old is None:
        assert bool((w == 0).any()) and not bool(_bits(dp[w == 0]).any()) and not bool(_bits(dp[:, dl:]).any()), 'zero-weight rows and pad columns: zero bits'
    else:
        assert torch.equal(_bits(dp[w == 0]), _bits(old[w == 0])) and torch.equal(_bits(dp[:, dl:]), _bits(old[:, dl:])), 'accumulate: zero-weight rows add nothing'
    dpz, accz = _mse_run('tfx_mse_w_fwd_bwd', 'tfx_mse_w_args', R_, dl, ldp, ldd, torch.full_like(pred, float('nan')), flow, gs, old, row_w=torch.zeros(R_, device=DEV), **clean)
    assert float(accz[0]) == 0.5 and (torch.equal(_bits(dpz), _bits(old)) if old is not None else not bool(_bits(dpz).any())), 'all zero: acc untouched, exact zeros'
