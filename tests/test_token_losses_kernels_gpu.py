"""The per-token loss kernels on the GPU - tfx_ce_rows_fwd and tfx_mse_rows_fwd (include/tfx.h tfx_ce_rows_args, tfx_mse_rows_args) - through the C ABI, on
the six shapes of the chunked head's tests and the MSE shapes of tests/_decode_loss_cases.py, under the four (z, e) settings and the four weight patterns of
tests/_loss_weight_cases.py (restatements and bounds: tests/_token_loss_cases.py):
  lse             bit-equal to tfx_ce_w_fwd on the same input (the same arithmetic), every row of every shape
  acc, aux        bit-equal to tfx_ce_w_fwd's wherever bits are defined - a launch that one block serves - and, on the whole shape, within the bound of
                  re-ordering the same per-block sums.  A block adds its sums with fp32 atomics, and the order in which the blocks of a launch arrive is the
                  hardware's: measured on an MI355X at 67 x 1000 (17 blocks), z = e = 0, all-ones weights, acc[0] came out 724.9859 from tfx_ce_rows_fwd and
                  724.9860 from tfx_ce_w_fwd, one unit in the last place - the figure tfx_ce_w_fwd shows against itself, which is why
                  tests/test_loss_weights_kernels_gpu.py compares acc[0] of two launches to 1e-5.  The same holds for tfx_mse_rows_fwd's acc below.
  row_loss        every element within tol_row; ignored and zero-weight rows exactly 0 with NaN logits in them; guard bands untouched
  row_sse         every element within tol_sse; acc bit-equal to tfx_mse_w_fwd_bwd's, with model_output_clean on and off; zero-weight rows unread."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_weight_cases as C                                         # noqa: E402
import _text_loss_terms_cases as R                                     # noqa: E402
import _token_loss_cases as K                                          # noqa: E402
import test_text_head_gpu as TH                                        # noqa: E402  (_written, sync, _stream)
from _decode_loss_cases import CLEAN_EPS, MSE_SHAPES, mse_inputs       # noqa: E402
from _gemm_cases import BF, U32, assert_elementwise, assert_untouched, guarded     # noqa: E402

DEV = 'cuda'
sync, _stream = TH.sync, TH._stream
BOTH = [(c, s) for c in R.CASES for s in K.SETTINGS]
both_id = lambda v: R.case_id(v) if len(v) == 3 else R.setting_id(v)


@functools.lru_cache(maxsize=None)
def _kcase(case):
    T, V, ld = case
    return R.inputs(T, V, ld, DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _sums():
    return (torch.tensor(R.ACC_INIT + (9.0, 9.0), device=DEV, dtype=torch.float32), torch.tensor(R.AUX_INIT + (7.0, 7.0), device=DEV, dtype=torch.float32))


def _fwd(fn, st, case, setting, lg, lab, w, rows=None, **extra):
    """`rows`: launch over the first `rows` rows only"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    T = T if rows is None else rows
    lbuf, lse = guarded(T, 1, torch.float32, DEV, 0)
    acc, aux = _sums()
    capi.call(fn, capi.make_args(st, T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, z_weight=setting[0], smoothing=setting[1], aux=aux, row_w=w, **extra), _stream())
    sync()
    return lbuf, lse, acc, aux


@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_ce_rows_fwd_every_pattern(case, setting):
    T, V, ld = case
    lg, lab = _kcase(case)
    for pattern in K.PATTERNS:
        w = C.weights(T, pattern, seed=V).to(DEV)
        lg_in = torch.where((w == 0)[:, None], torch.full_like(lg, float('nan')), lg)            # a zero-weight row is not read (ignored rows hold NaN already)
        _, lse0, acc0, aux0 = _fwd('tfx_ce_w_fwd', 'tfx_ce_w_chunk_args', case, setting, lg_in, lab, w)
        rbuf0, _ = guarded(T, 1, torch.float32, DEV, 0)
        rbuf, rows = guarded(T, 1, torch.float32, DEV, 0)
        lbuf, lse, acc, aux = _fwd('tfx_ce_rows_fwd', 'tfx_ce_rows_args', case, setting, lg_in, lab, w, row_loss=rows)
        what = f'{R.case_id(case)} {R.setting_id(setting)} {pattern}'
        print(f'  {what}: acc {acc.tolist()} | w_fwd {acc0.tolist()}; aux {aux.tolist()} | {aux0.tolist()}')
        assert torch.equal(_bits(lse), _bits(lse0)), 'lse: tfx_ce_w_fwd\'s bits'
        r = C.ce_w_ref(lg, lab, w, V, *setting)
        tol_lse, tol_row = K.row_loss_bounds(r)
        # the sums: one block (four rows of a narrow shape, one row of a wide one) has no order to differ in - bits; the whole launch: the same per-block
        # sums in another order, (blocks + 1) u (|init| + sum of magnitudes) either way round
        one = 1 if ld > R.WIDE_LD else min(T, 4)
        _, _, a1, x1 = _fwd('tfx_ce_w_fwd', 'tfx_ce_w_chunk_args', case, setting, lg_in, lab, w, rows=one)
        _, _, a2, x2 = _fwd('tfx_ce_rows_fwd', 'tfx_ce_rows_args', case, setting, lg_in, lab, w, rows=one, row_loss=torch.empty(one, device=DEV))
        assert torch.equal(_bits(a1), _bits(a2)) and torch.equal(_bits(x1), _bits(x2)), 'acc and aux of a one-block launch: tfx_ce_w_fwd\'s bits'
        blocks = min(T, 2048) if ld > R.WIDE_LD else min(-(-T // 4), 1024)
        order = 2 * (blocks + 1) * U32
        mag = [float((r.w * ((1 - r.e) * (r.lse_all.abs() + r.picked.abs()) + r.e * (r.lse_all.abs() + r.mu.abs()) + r.z * r.sq)).sum()), float(r.w.sum()),
               float((r.w * (r.lse_all.abs() + r.picked.abs())).sum()), float((r.w * r.sq).sum())]
        init = list(R.ACC_INIT) + list(R.AUX_INIT)
        for k, (a, b) in enumerate(zip(acc[:2].tolist() + aux[:2].tolist(), acc0[:2].tolist() + aux0[:2].tolist())):
            assert abs(a - b) <= order * (abs(init[k]) + mag[k]), ('the sums of the two launches differ by more than an order of atomics can', k, a, b)
        assert acc[2:].tolist() == [9.0, 9.0] and aux[2:].tolist() == [7.0, 7.0]
        assert pattern == 'uniform' or float(acc[1]) == float(acc0[1]), 'weights in {0, 1}: acc[1] is the count, exact in any order'
        worst = assert_elementwise(f'tfx_ce_rows_fwd {what} row_loss', rows.double(), (r.w * r.row)[:, None], tol_row[:, None], tile=(4, 1))
        dead = ~r.valid | (w == 0)
        assert not bool(_bits(rows[dead]).any()), 'ignored and zero-weight rows: exactly 0'
        assert_untouched(f'{what} row_loss', rbuf, rbuf0, TH._written(rbuf, T))
        assert_untouched(f'{what} lse', lbuf, guarded(T, 1, torch.float32, DEV, 0)[0], TH._written(lbuf, T))
        # the row values are the terms of the sum: their float64 total is acc[0]'s growth, within the bound of that sum
        grown = float(acc[0].double()) - R.ACC_INIT[0]
        assert abs(grown - float(rows.double().sum())) <= float(C.ce_w_bounds(r)[1]), 'acc[0] is the sum of the row values'
        print(f'  {what}: row_loss worst error / bound {worst:.3f}')
        if pattern == 'zeros':
            assert acc.tolist() == list(R.ACC_INIT) + [9.0, 9.0] and aux.tolist() == list(R.AUX_INIT) + [7.0, 7.0]


def test_null_pointers_return_minus_one_before_any_launch():
    """every other pointer is NULL too: a launch would fault"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    sp = ctypes.c_void_p(_stream())
    assert lib.tfx_ce_rows_fwd(ctypes.byref(capi.make_args('tfx_ce_rows_args', T=4, V=8, ld=8)), sp) == -1
    assert lib.tfx_mse_rows_fwd(ctypes.byref(capi.make_args('tfx_mse_rows_args', R=4, dl=8, ld_pred=8, ld_d=64)), sp) == -1
    sync()


# ================================================================================================ the squared error
@pytest.mark.parametrize('mode', ['plain', 'clean'])
@pytest.mark.parametrize('R_,dl,ldp,ldd', MSE_SHAPES)
def test_mse_rows_fwd(R_, dl, ldp, ldd, mode):
    from transfusion_pytorch_amd import capi
    pred, flow, _, times, row_inst, _ = (t.to(DEV) for t in mse_inputs(R_, dl, seed=1))
    clean = dict(row_inst=row_inst, inst_time=times, clean_eps=CLEAN_EPS) if mode == 'clean' else {}
    for pattern in ('ones', 'uniform', 'zeros'):
        w = C.weights(R_, pattern, seed=dl).to(DEV)
        pp = torch.full((R_, ldp), float('nan'), device=DEV); pp[:, :dl] = pred
        pp[w == 0] = float('nan')                                                        # a zero-weight row is not read
        dp = torch.zeros(R_, ldd, dtype=BF, device=DEV)
        acc0 = torch.tensor([0.5, 9.0, 9.0, 9.0], device=DEV)
        capi.call('tfx_mse_w_fwd_bwd', capi.make_args('tfx_mse_w_args', R=R_, dl=dl, pred=pp, ld_pred=ldp, flow=flow, grad_scale=0.37, dpred=dp, ld_d=ldd, acc=acc0,
                                                      accumulate=0, row_w=w, **clean), _stream())
        sbuf, sse = guarded(R_, 1, torch.float32, DEV, 0)
        sse.zero_()
        before = sbuf.clone()
        acc = torch.tensor([0.5, 9.0, 9.0, 9.0], device=DEV)
        capi.call('tfx_mse_rows_fwd', capi.make_args('tfx_mse_rows_args', R=R_, dl=dl, pred=pp, ld_pred=ldp, flow=flow, ld_d=ldd, acc=acc, row_w=w, row_sse=sse), _stream())
        sync()
        print(f'  mse_rows {mode} {pattern} R {R_} dl {dl}: acc {float(acc[0])!r} | w_fwd_bwd {float(acc0[0])!r}')
        # acc: bits where one block serves the launch (four rows of 64 elements: 256 threads), the re-ordering bound of the per-block sums on the whole shape
        a1, a2 = torch.tensor([0.5, 9.0], device=DEV), torch.tensor([0.5, 9.0], device=DEV)
        capi.call('tfx_mse_w_fwd_bwd', capi.make_args('tfx_mse_w_args', R=4, dl=dl, pred=pp, ld_pred=ldp, flow=flow, grad_scale=0.37, dpred=torch.zeros(4, ldd, dtype=BF, device=DEV),
                                                      ld_d=ldd, acc=a1, accumulate=0, row_w=w, **clean), _stream())
        capi.call('tfx_mse_rows_fwd', capi.make_args('tfx_mse_rows_args', R=4, dl=dl, pred=pp, ld_pred=ldp, flow=flow, ld_d=ldd, acc=a2, row_w=w,
                                                     row_sse=torch.zeros(4, device=DEV)), _stream())
        sync()
        assert ldd == 64 and torch.equal(_bits(a1), _bits(a2)), 'acc of a one-block launch: tfx_mse_w_fwd_bwd\'s bits'
        blocks = min(-(-R_ * ldd // 256), 2048)
        total = float(K.row_sse(pred, flow, w).sum())
        assert abs(float(acc[0]) - float(acc0[0])) <= 2 * (blocks + 1) * U32 * (0.5 + total) and acc[1:].tolist() == [9.0, 9.0, 9.0]
        worst = assert_elementwise(f'tfx_mse_rows_fwd {mode} {pattern} row_sse', sse.double(), K.row_sse(pred, flow, w)[:, None], K.row_sse_bound(pred, flow, w, ldd)[:, None], tile=(4, 1))
        assert not bool(_bits(sse[w == 0]).any()), 'zero-weight rows add nothing'
        assert_untouched('row_sse', sbuf, before, TH._written(sbuf, R_))
        print(f'  mse_rows {mode} {pattern} R {R_} dl {dl}: row_sse worst error / bound {worst:.3f}')
