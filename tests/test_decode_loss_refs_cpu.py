"""The references of tests/_decode_loss_cases.py against something other than the kernels they judge (no GPU, no library):

  ode_reference     a staggered whole solve against torchdiffeq's fixed-grid midpoint odeint of every sample on its own
  draw_reference    the reference's sampling steps (T:591-605, T:2695-2698) restated in torch
  mse_reference     its autograd gradient against the closed form include/tfx.h states, every mode combination
"""
import pytest
import torch

from _decode_loss_cases import (CFG_SCALE, CLEAN_EPS, F64, MSE_MODES, ODE_SHAPE, SAMPLE_MODES, SOLVE_S, draw_reference, draw_targets, mse_closed_form,
                                mse_inputs, mse_reference, ode_evals, ode_reference, solve_field, solve_fields, solve_pred, solve_rows0, solve_schedule,
                                solve_steps, u_for)
from oracle.shims.torchdiffeq import odeint


# ---------------------------------------------------------------------------------------------- ODE
@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
def test_ode_reference_staggered_solve_equals_odeint(H, compact):
    B, Lc, Lq, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['Lq'], 5
    dmax = ODE_SHAPE['dmax']
    ts, evals = ode_evals(SOLVE_S)
    assert len(evals) == 2 * (SOLVE_S - 1)
    y0, c, cu = solve_fields(B, Lc, dl)
    y = torch.full((B, Lc, dmax), float('nan'), dtype=F64); y[:, :, :dl] = y0
    ym = torch.full((B, Lc, dmax), float('nan'), dtype=F64)
    seen_modes = set()
    for step in range(solve_steps(evals)):
        sched = solve_schedule(step, evals)
        modes = [s[0] for s in sched]
        seen_modes.update(modes)
        if step == 3:
            assert len({(s[0], s[2]) for s in sched}) == B, 'every sample at its own evaluation'
        if step == 14:
            assert 3 in modes and (1 in modes or 2 in modes), 'a finished sample next to running ones'
        ctl = torch.tensor([modes, [s[1] for s in sched]], dtype=F64)
        rows0, n_rows = solve_rows0(B, H, Lc, sched, seed=step) if compact else (None, None)
        field = lambda x: solve_pred(x, sched, c, cu, H, Lq, rows0)             # noqa: E731
        _, y, ym, _, _, _ = ode_reference(y, ym, ctl, field, H, Lq, dl, CFG_SCALE, rows0=rows0, n_rows=n_rows)
    assert seen_modes == {0, 1, 2, 3}
    for i in range(B):
        want = odeint(solve_field(c[i], cu[i], H), y0[i], ts, method='midpoint')[-1]
        err = float((y[i, :, :dl] - want).abs().max())
        assert err <= 1e-12, (i, err)
    assert torch.isnan(y[:, :, dl:]).all() and torch.isnan(ym[:, :, dl:]).all(), 'columns >= dl are never written'


def test_ode_reference_masks():
    """what the two calls may write: idle samples nothing, finished samples only their staged rows, negative rows in either half no update"""
    B, Lc, Lq, dl, dmax = 5, 3, 4, 2, 3
    y, ym = torch.randn(B, Lc, dmax, dtype=F64), torch.randn(B, Lc, dmax, dtype=F64)
    ctl = torch.tensor([[1, 2, 0, 3, 1], [0.5, 0.25, 9., 9., 2.]], dtype=F64)
    rows0 = [0, 3, -1, 6, 9, 12, -1, 15, 18, -1]
    pred = torch.randn(21, dl, dtype=F64)
    x, y1, ym1, x_w, y_w, ym_w = ode_reference(y, ym, ctl, pred, 2, Lq, dl, 2., sel=[1, 1, 1, 1, 1], rows0=rows0, n_rows=21)
    assert x_w.sum() == 6 * Lc * dl and not x_w[15:18].any()
    assert torch.equal(x[3:6], ym[1, :, :dl]) and torch.equal(x[0:3], y[0, :, :dl]) and torch.equal(x[18:21], y[3, :, :dl])
    assert ym_w[0, :, :dl].all() and ym_w.sum() == Lc * dl, 'sample 0 (mode 1) writes its midpoint; sample 4 has no null-text rows'
    assert not y_w.any(), 'sample 1 (mode 2) has no null-text rows: no update'
    assert torch.equal(y1, y)
    u = pred[12:15]
    assert torch.allclose(ym1[0, :, :dl], y[0, :, :dl] + 0.5 * (u + 2. * (pred[0:3] - u)), rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------- draw
def restated_text_only_logits(logits, V, V_draw, T, min_p):
    """generate_text_only's three lines (T:2695-2697) on one batch of rows: divide by the temperature, min_p_filter over ALL logits, masked_fill_ of
    everything but the text tokens with -finfo.max"""
    l = logits[:, :V].to(F64) / T
    probs = l.softmax(-1)
    l = torch.where(probs < min_p * probs.amax(-1, keepdim=True), float('-inf'), l)
    l[:, V_draw:] = -torch.finfo(l.dtype).max
    return l


@pytest.mark.parametrize('V,V_draw', [(390, 390), (390, 256), (70, 64), (300, 1)])
@pytest.mark.parametrize('T,min_p', SAMPLE_MODES)
def test_draw_reference_equals_the_restated_sampling_steps(V, V_draw, T, min_p):
    torch.manual_seed(7)
    logits = torch.randn(64, V + 2) * 3.
    logits[:, V:] = 1e9
    if V_draw < V:
        logits[::2, V_draw:V] -= 12.                       # half of the rows: text survivors (almost) for sure
    keep, q = draw_reference(logits, V, V_draw, T, min_p)
    l = restated_text_only_logits(logits, V, V_draw, T, min_p)
    p = l.softmax(-1)
    some = keep.any(-1)
    assert some.sum() >= 16 and (V_draw < V or some.all())
    assert torch.equal(p[some, :V_draw] > 0, keep[some]) and bool((p[some, V_draw:] == 0).all()), 'same support'
    assert float((p[some, :V_draw] - q[some] / q[some].sum(-1, keepdim=True)).abs().max()) <= 1e-12
    # the cells u_for aims at are the cells of that distribution's inverse CDF
    for r, ks in enumerate(draw_targets(keep, q)):
        for k in ks:
            u = float(u_for(q[r:r + 1], torch.tensor([k])))
            cdf = p[r, :V_draw].cumsum(-1)
            assert int((cdf > u).float().argmax()) == k, (r, k)


@pytest.mark.parametrize('T,min_p', SAMPLE_MODES[:2])
def test_restated_steps_return_the_first_masked_column_when_no_text_token_survives(T, min_p):
    """every text logit is filtered (-inf), every masked column holds -finfo.max, which absorbs the Gumbel noise: argmax takes the first of them"""
    import math
    V, V_draw = 390, 256
    torch.manual_seed(8)
    logits = torch.randn(16, V) * 3.
    gap = 2. * (-T * math.log(min_p))
    logits[:, V_draw:] = -20.
    logits[torch.arange(16), V_draw + 1 + torch.arange(16) * 7] = logits[:, :V_draw].amax(-1) + gap
    keep, q = draw_reference(logits, V, V_draw, T, min_p)
    assert not keep.any()
    l = restated_text_only_logits(logits, V, V_draw, T, min_p)
    assert bool((l[:, :V_draw] == float('-inf')).all())
    for seed in range(8):
        torch.manual_seed(seed)
        log = lambda t: torch.log(t.clamp(min=1e-20))                          # noqa: E731  (T:292-301: log, gumbel_noise, gumbel_sample)
        noise = -log(-log(torch.rand_like(l)))
        assert bool(((l + noise).argmax(-1) == V_draw).all())


# ---------------------------------------------------------------------------------------------- MSE
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('mode', sorted(MSE_MODES))
def test_mse_reference_autograd_equals_the_closed_form(mode, accumulate):
    clean, rmode = MSE_MODES[mode]
    R, dl = 37, 5
    pred, flow, noise, times, row_inst, w = mse_inputs(R, dl)
    t_row = times[row_inst.long()]
    assert bool((t_row == 0).any()) and bool((t_row == 1).any()) and bool(((1 - t_row) < CLEAN_EPS).any())
    kw = dict(clean_eps=CLEAN_EPS if clean else None, recon_w=w if rmode is not None else None, recon_mode=rmode or 0)
    old = torch.randn(R, dl, dtype=F64) if accumulate else None
    loss, g = mse_reference(pred, flow, noise, t_row, 0.37, old=old, **kw)
    want = mse_closed_form(pred, flow, t_row, 0.37, **kw)
    if accumulate:
        want = want + old
    assert float((g - want).abs().max()) <= 1e-10
    t = t_row.double()[:, None]
    r = (pred.double() - flow.double()) if rmode is None else (1 - t) * pred.double() - (t if rmode == 0 else 1.) * flow.double()
    ws = 1. if rmode is None else w.double()[:, None]
    assert abs(float(loss) - float((ws * r * r).sum())) <= 1e-10 * float(loss)
