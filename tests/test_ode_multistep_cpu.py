"""Adams-Bashforth multistep solvers (`odeint_kwargs['method']` in ab2 / ab3 / ab4): everything that needs no GPU - the coefficients against
tests/_ode_ab_cases.py's own copy and their order conditions in exact rationals, the evaluation schedule and the control block, the fp64 yardstick
`ab_solve` (its observed order of convergence; the start-up rule to the bit on short grids), the constructor, the C ABI and its host-side checks."""
import math
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _ode_ab_cases as AB                                                                  # noqa: E402
import _ode_rk_cases as RK                                                                  # noqa: E402
from _decode_loss_cases import F64, ODE_SHAPE, solve_field, solve_fields                   # noqa: E402
from transfusion_pytorch_amd import capi, ode                                               # noqa: E402

GRIDS = [2, 3, 4, 5, 8, 16]


# ---------------------------------------------------------------------------------------------- 1. coefficients
@pytest.mark.parametrize('method', AB.METHODS)
def test_coefficients_are_exact_fractions_of_exactly_their_order(method):
    P, start, beta = AB.MULTISTEP[method]
    ms = ode.MULTISTEP[method]
    assert ode.MULTISTEP_METHODS == tuple(AB.METHODS) == ('ab2', 'ab3', 'ab4') and ode.HIST_SLOTS == AB.HIST_SLOTS == 3
    assert ms.order == P and ms.start == start and list(ms.beta) == beta and len(beta) == P
    assert all(isinstance(b, Fr) for b in ms.beta), 'exact fractions'
    assert ode.TABLEAUS[start].order == P, 'the start-up rule has the order of the method'
    assert set(ode.TABLEAUS) == set(RK.TABLEAUS) and not set(ode.MULTISTEP) & set(ode.TABLEAUS), 'the tableau names stay as they are'
    # y_{n+1} - y_n = dt sum_j beta_j g_{n-j} is exact for polynomials g of degree m  <=>  sum_j beta_j (-j)^m = 1 / (m + 1)
    moment = lambda m: sum((b * Fr(-j) ** m for j, b in enumerate(beta)), Fr(0))
    for m in range(P):
        assert moment(m) == Fr(1, m + 1), (method, m)
    assert moment(P) != Fr(1, P + 1), f'{method} would be of order {P + 1}'


# ---------------------------------------------------------------------------------------------- 2. schedule and control block
@pytest.mark.parametrize('S', GRIDS)
@pytest.mark.parametrize('method', AB.METHODS)
def test_schedule_counts_times_weights_and_slots(method, S):
    P, start, beta = AB.MULTISTEP[method]
    ns, N = RK.stages(start), S - 1
    sched = ode.ode_schedule(method, S)
    ts = torch.linspace(0, 1, S)
    assert len(sched) == AB.forwards(method, S) == ns * min(P - 1, N) + max(0, N - (P - 1))
    if S == 16:
        assert len(sched) == {'ab2': 16, 'ab3': 19, 'ab4': 24}[method]
    f32 = lambda v: float(np.float32(v))
    own = ode.ode_schedule(start, S)
    read_later = lambda n: N > P - 1 and n < N - 1             # a later multistep step reads g_n: the store may be dropped otherwise, and is
    at = 0
    for n in range(N):
        if n < P - 1:
            step = sched[at:at + ns]
            at += ns
            assert [tuple(e)[:6] for e in step] == [tuple(e)[:6] for e in own[n * ns:(n + 1) * ns]], 'a start-up step is the start-up rule\'s own'
            assert [e.store for e in step] == [n % 3 if read_later(n) else -1] + [-1] * (ns - 1), 'the stage-0 derivative goes to slot n mod 3'
            assert all(e.hr == () and e.hw == () for e in step)
            continue
        e = sched[at]
        at += 1
        dt = float(ts[n + 1] - ts[n])
        assert e.t == float(ts[n]), 'a multistep evaluation sits on the grid point itself'
        assert e.q == 0 and e.last and e.wa == () and len(e.w) == 1 and e.wb == e.w
        assert e.store == (n % 3 if read_later(n) else -1)
        assert list(e.hr) == [(n - j) % 3 for j in range(P - 1, 0, -1)], 'the slots of g_{n-P+1} .. g_{n-1}, oldest first'
        for got, b in zip([*e.hw, e.w[0]], [*(beta[j] for j in range(P - 1, 0, -1)), beta[0]]):
            assert got == f32(got) and got != 0. and abs(got - dt * float(b)) <= 2. ** -24 * abs(dt * float(b)) * (1 + 1e-9)
    assert at == len(sched)
    # every slot a multistep step reads was written by the step it stands for, and by no step since
    owner = {}
    for e, n in zip(sched, [n for n in range(N) for _ in range(ns if n < P - 1 else 1)]):
        for j, s in zip(range(P - 1, 0, -1), e.hr):
            assert owner.get(s) == n - j, (method, S, n, j)
        if e.store >= 0:
            owner[e.store] = n                               # (after the reads: the launch reads before it writes)
    # the tableau rules' lists carry the defaults
    assert all(e.store == -1 and e.hr == () and e.hw == () for e in own)


@pytest.mark.parametrize('S', GRIDS)
@pytest.mark.parametrize('method', AB.METHODS)
def test_control_block_rows(method, S):
    sched = ode.ode_schedule(method, S)
    ctl = ode.ode_control(method, S)
    base = ode.ode_control(AB.MULTISTEP[method][1], S)
    assert base.rows.shape[0] == 8 and ode.ode_control('midpoint', S).rows.shape[0] == 1, 'the existing blocks keep their shape'
    assert ctl.rows.shape == (15, len(sched)) and ctl.rows.dtype == np.float32 and ctl.times == tuple(e.t for e in sched)
    for n, e in enumerate(sched):
        col = ctl.rows[:, n]
        assert ctl.modes[n] == (2 if e.last else 1) and col[0] == e.q
        assert list(col[1:4]) == [*e.wa, *[0.] * (3 - len(e.wa))] and list(col[4:8]) == [*e.wb, *[0.] * (4 - len(e.wb))]
        assert col[8] == e.store and list(col[9:12]) == [*e.hr, *[0] * (3 - len(e.hr))] and list(col[12:15]) == [*e.hw, *[0.] * (3 - len(e.hw))]
        if e.hr:
            assert ctl.modes[n] == 2 and col[0] == 0 and col[4] == e.w[0] != 0, 'a multistep evaluation: mode 2 at stage 0, its weight of g in update weight 0'
    P = AB.MULTISTEP[method][0]
    if S - 1 <= P - 1:
        assert np.array_equal(ctl.rows[:8], base.rows) and np.array_equal(ctl.modes, base.modes) and ctl.times == base.times
        assert (ctl.rows[8] == -1).all() and not ctl.rows[9:].any(), 'a short grid is the start-up rule with no history traffic'


# ---------------------------------------------------------------------------------------------- 3. / 4. the yardstick
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', AB.METHODS)
def test_ab_solve_converges_at_the_order_of_its_method(method, H):
    """grids (17, 33, 65, 129): on the tableau test's coarser ones the few start-up steps still dominate ab4's error"""
    P = AB.MULTISTEP[method][0]
    y0, c, cu = solve_fields(ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5)
    f = solve_field(c[0], cu[0], H)
    fine = RK.rk_solve('rk4', f, y0[0], torch.linspace(0, 1, 2049, dtype=F64))
    errs = [float((AB.ab_solve(method, f, y0[0], torch.linspace(0, 1, n, dtype=F64)) - fine).abs().max()) for n in (17, 33, 65, 129)]
    rates = [math.log2(a / b) for a, b in zip(errs, errs[1:])]
    print(f'{method} H {H}: errors {["%.3e" % e for e in errs]}, log2 ratios {["%.2f" % r for r in rates]} (order {P})')
    assert all(abs(r - P) <= 0.35 for r in rates), (method, rates)


@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', AB.METHODS)
def test_ab_solve_on_a_short_grid_is_the_start_up_rule_to_the_bit(method, H):
    P, start, _ = AB.MULTISTEP[method]
    y0, c, cu = solve_fields(ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5)
    f = solve_field(c[1], cu[1], H)
    for S in range(2, P + 1):                                # N = S - 1 <= P - 1
        ts = torch.linspace(0, 1, S, dtype=F64)
        assert torch.equal(AB.ab_solve(method, f, y0[1], ts), RK.rk_solve(start, f, y0[1], ts)), (method, S)
    ts = torch.linspace(0, 1, P + 2, dtype=F64)
    assert not torch.equal(AB.ab_solve(method, f, y0[1], ts), RK.rk_solve(start, f, y0[1], ts)), 'one step further the multistep rule has taken over'


def test_ab_solve_calls_the_field_once_per_multistep_step():
    y0, c, cu = solve_fields(ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5)
    inner = solve_field(c[0], cu[0], 1)
    for method in AB.METHODS:
        calls = []
        AB.ab_solve(method, lambda t, y: (calls.append(float(t)), inner(t, y))[1], y0[0], torch.linspace(0, 1, 16, dtype=F64))
        assert len(calls) == AB.forwards(method, 16) == {'ab2': 16, 'ab3': 19, 'ab4': 24}[method]


# ---------------------------------------------------------------------------------------------- 5. constructor
def _model(**kw):
    from transfusion_pytorch_amd import Transfusion
    return Transfusion(num_text_tokens=32, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=64, depth=2), **kw)


@pytest.mark.parametrize('method', AB.METHODS)
def test_constructor_takes_the_multistep_methods(method):
    m = _model(odeint_kwargs=dict(atol=1e-5, rtol=1e-5, method=method))
    assert m.ode_method == method and m.odeint_kwargs['method'] == method
    assert _model(odeint_kwargs=dict(method=method)).ode_method == method                  # atol / rtol: accepted, not needed
    assert _model(odeint_kwargs=dict(method=method, atol=1., rtol=0.)).ode_method == method
    assert m._clone_architecture().ode_method == method
    assert ode.check_odeint_kwargs(dict(method=method, rtol=1e-3)) == method


def test_constructor_still_refuses_the_adams_names_of_torchdiffeq():
    for bad in ('explicit_adams', 'implicit_adams', 'dopri5', 'rk4_classic', 'ab5', 'ab1'):
        with pytest.raises(NotImplementedError, match='euler, midpoint, heun2, heun3, rk4') as ei:
            _model(odeint_kwargs=dict(method=bad))
        assert 'ab2, ab3, ab4' in str(ei.value), 'the refusal points to the multistep rules that do exist'
    for method in AB.METHODS:
        with pytest.raises(NotImplementedError, match='euler, midpoint, heun2, heun3, rk4'):
            _model(odeint_kwargs=dict(method=method, options=dict(step_size=0.1)))
        with pytest.raises(NotImplementedError, match='step_size'):
            _model(odeint_kwargs=dict(method=method, step_size=0.1))


# ---------------------------------------------------------------------------------------------- 6. ABI and host checks
def test_abi_and_version():
    for name in ('tfx_ode_ab_axpy', 'tfx_ode_ab_update'):
        assert name in capi.FUNCTIONS and hasattr(capi.lib(), name)
    assert capi.ENUMS['TFX_ODE_AB_HIST'] == 3 == ode.HIST_SLOTS
    assert len(capi.FUNCTIONS['tfx_ode_ab_update'][1]) == len(capi.FUNCTIONS['tfx_ode_rk_update'][1]) + 1, 'tfx_ode_rk_update with the ring'
    assert len(capi.FUNCTIONS['tfx_ode_ab_axpy'][1]) == 15
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'-odeab' in v and v.index(b'odeab') > v.index(b'oderk')


def test_host_argument_checks_return_before_any_launch():
    """every refused call below carries pointers no kernel could touch (small integers): a launch would fault, a host check returns its code"""
    lib = capi.lib()
    P = 64                                                   # a non-null pointer value that is never dereferenced on the host
    # tfx_ode_ab_axpy(y, h0, h1, h2, w0, w1, w2, wg, f_cond, f_uncond, cfg, g_out, out, n, stream)
    ax = lambda y=P, h=(P, P, P), w=(1., 1., 1.), fc=P, go=P, out=P, n=8: lib.tfx_ode_ab_axpy(y, *h, *w, 1., fc, None, 1., go, out, n, None)
    assert ax(n=0) == 0 and ax(n=-3) == 0
    assert ax(n=0, y=None, h=(None, None, None)) == 0, 'n <= 0 returns before the pointers are looked at'
    assert ax(y=None) == -1 and ax(fc=None) == -1 and ax(out=None) == -1
    for j in range(3):
        h = [P, P, P]; h[j] = None
        assert ax(h=tuple(h)) == -3, j
    assert ax(y=None, h=(None, P, P)) == -1, 'the missing state comes first'
    # tfx_ode_ab_update(y, k, hist, ctl, B, Lc, dmax, pred, H, Lq, dl, cfg, sel, rows0, stream)
    up = lambda y=P, k=P, hist=P, ctl=P, B=2, Lc=3, dmax=8, pred=P, H=1, Lq=4, dl=8: lib.tfx_ode_ab_update(y, k, hist, ctl, B, Lc, dmax, pred, H, Lq, dl, 1., None, None, None)
    assert up(B=0) == 0 and up(Lc=0) == 0 and up(dl=0) == 0
    for kw in (dict(y=None), dict(k=None), dict(hist=None), dict(ctl=None), dict(pred=None), dict(H=0), dict(H=3), dict(Lq=2), dict(dl=9)):
        assert up(**kw) == -1, kw
