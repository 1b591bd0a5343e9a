"""Fixed-grid Runge-Kutta solvers (`odeint_kwargs['method']` in euler / midpoint / heun2 / heun3 / rk4): everything that needs no GPU - the tableaus
against tests/_ode_rk_cases.py's own copy and the order conditions in exact rationals, the evaluation schedule, the fp64 yardstick `rk_solve` itself
(against the torchdiffeq stand-in for midpoint, and by its observed order of convergence), the constructor, the C ABI and its host-side checks."""
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

import _ode_rk_cases as RK                                                                  # noqa: E402
from _decode_loss_cases import F64, ODE_SHAPE, solve_field, solve_fields                   # noqa: E402
from oracle.shims.torchdiffeq import odeint                                                 # noqa: E402
from transfusion_pytorch_amd import capi, ode                                               # noqa: E402


# ---------------------------------------------------------------------------------------------- 1. tableaus
@pytest.mark.parametrize('method', RK.METHODS)
def test_tableaus_equal_the_restated_ones_and_have_exactly_their_order(method):
    order, c, A, b = RK.TABLEAUS[method]
    tab = ode.TABLEAUS[method]
    assert set(ode.TABLEAUS) == set(RK.TABLEAUS) and ode.METHODS == tuple(RK.METHODS)
    assert tab.order == order and list(tab.c) == c and [list(r) for r in tab.A] == A and list(tab.b) == b
    assert all(isinstance(v, Fr) for v in [*tab.c, *tab.b, *(a for r in tab.A for a in r)]), 'exact fractions'
    assert len(c) <= ode.MAX_STAGES == RK.MAX_STAGES and all(len(A[q]) == q for q in range(len(c)))
    for q in range(len(c)):
        assert sum(A[q], Fr(0)) == c[q], 'row sum'
    cond = RK.order_conditions(method)
    for p in range(1, order + 1):
        assert all(r == 0 for r in cond[p]), (method, p, cond[p])
    assert any(r != 0 for r in cond[order + 1]), f'{method} would be of order {order + 1}'


# ---------------------------------------------------------------------------------------------- 2. schedule
@pytest.mark.parametrize('S', [2, 3, 8, 16])
@pytest.mark.parametrize('method', RK.METHODS)
def test_schedule_shape_times_and_weights(method, S):
    _, c, A, b = RK.TABLEAUS[method]
    n = len(c)
    sched = ode.ode_schedule(method, S)
    ts = torch.linspace(0, 1, S)
    assert len(sched) == n * (S - 1)
    f32 = lambda v: float(np.float32(v))
    for k in range(S - 1):
        t0, dt = float(ts[k]), float(ts[k + 1] - ts[k])
        step = sched[k * n:(k + 1) * n]
        assert [e.q for e in step] == list(range(n)) and [e.last for e in step] == [False] * (n - 1) + [True]
        assert all(step[q].t <= step[q + 1].t for q in range(n - 1)), 'non-decreasing inside a step'
        for q, e in enumerate(step):
            if c[q] == 1:
                assert e.t == float(ts[k + 1]), 'a c = 1 stage sits on the grid point itself'
            else:
                assert e.t == t0 + float(c[q]) * dt
            assert len(e.wa) == q and len(e.w) == q + 1 and len(e.wb) == n
            # the weights are fp32 numbers within one rounding of dt a (dt itself is an fp32 number)
            for got, a in zip([*e.wa, *e.wb, *e.w], [*A[q], *b, *(b[:q + 1] if e.last else A[q + 1])]):
                assert got == f32(got) and abs(got - dt * float(a)) <= 2. ** -24 * abs(dt * float(a)) * (1 + 1e-9) and (got == 0.) == (a == 0)


@pytest.mark.parametrize('S', [2, 3, 4, 8, 16, 31])
def test_midpoint_schedule_is_the_list_the_midpoint_loops_build(S):
    ts = torch.linspace(0, 1, S)
    evals = []                                               # the list the midpoint kernels were written against; ode.ode_control / sampling._ode_solve read it off the schedule
    for k in range(S - 1):
        t0, dt = float(ts[k]), float(ts[k + 1] - ts[k])
        evals += [(t0, dt * 0.5, 1), (t0 + dt * 0.5, dt, 2)]
    sched = ode.ode_schedule('midpoint', S)
    assert [e.t for e in sched] == [e[0] for e in evals]
    assert np.array_equal(np.array([e.w[e.q] for e in sched], np.float32).view(np.int32), np.array([e[1] for e in evals], np.float32).view(np.int32))
    assert [2 if e.last else 1 for e in sched] == [e[2] for e in evals]
    assert all(e.w[0] == 0. for e in sched if e.last), 'b_0 = 0: the update adds the second derivative alone'


# ---------------------------------------------------------------------------------------------- 3. the yardstick
@pytest.mark.parametrize('H', [1, 2])
def test_rk_solve_midpoint_is_the_torchdiffeq_stand_in_to_the_bit(H):
    B, Lc, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5
    y0, c, cu = solve_fields(B, Lc, dl)
    ts = torch.linspace(0, 1, 8, dtype=F64)
    for i in range(B):
        f = solve_field(c[i], cu[i], H)
        assert torch.equal(RK.rk_solve('midpoint', f, y0[i], ts), odeint(f, y0[i], ts, method='midpoint')[-1])


@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', RK.METHODS)
def test_rk_solve_converges_at_the_order_of_its_method(method, H):
    p = RK.TABLEAUS[method][0]
    y0, c, cu = solve_fields(ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5)
    f = solve_field(c[0], cu[0], H)
    fine = RK.rk_solve('rk4', f, y0[0], torch.linspace(0, 1, 2049, dtype=F64))
    errs = [float((RK.rk_solve(method, f, y0[0], torch.linspace(0, 1, n, dtype=F64)) - fine).abs().max()) for n in (5, 9, 17, 33)]
    rates = [math.log2(a / b) for a, b in zip(errs, errs[1:])]
    print(f'{method} H {H}: errors {["%.3e" % e for e in errs]}, log2 ratios {["%.2f" % r for r in rates]} (order {p})')
    assert all(abs(r - p) <= 0.35 for r in rates), (method, rates)


# ---------------------------------------------------------------------------------------------- 4. constructor
def _model(**kw):
    from transfusion_pytorch_amd import Transfusion
    return Transfusion(num_text_tokens=32, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=64, depth=2), **kw)


@pytest.mark.parametrize('method', RK.METHODS)
def test_constructor_takes_the_five_methods(method):
    m = _model(odeint_kwargs=dict(atol=1e-5, rtol=1e-5, method=method))
    assert m.ode_method == method and m.odeint_kwargs['method'] == method
    assert _model(odeint_kwargs=dict(method=method)).ode_method == method                  # atol / rtol: accepted, not needed
    assert _model(odeint_kwargs=dict(method=method, atol=1., rtol=0.)).ode_method == method
    assert m._clone_architecture().ode_method == method


def test_constructor_defaults_to_midpoint_and_refuses_the_rest():
    assert _model().ode_method == 'midpoint' and _model(odeint_kwargs=dict(atol=1e-5)).ode_method == 'midpoint'
    for bad in ('dopri5', 'explicit_adams', 'rk4_classic'):
        with pytest.raises(NotImplementedError, match='euler, midpoint, heun2, heun3, rk4'):
            _model(odeint_kwargs=dict(method=bad))
    with pytest.raises(NotImplementedError, match='euler, midpoint, heun2, heun3, rk4'):
        _model(odeint_kwargs=dict(method='euler', options=dict(step_size=0.1)))
    with pytest.raises(NotImplementedError, match='step_size'):
        _model(odeint_kwargs=dict(step_size=0.1))


# ---------------------------------------------------------------------------------------------- 5. / 6. ABI and host checks
def test_abi_and_version():
    for name in ('tfx_ode_rk_axpy', 'tfx_ode_rk_stage', 'tfx_ode_rk_update'):
        assert name in capi.FUNCTIONS and hasattr(capi.lib(), name)
    assert capi.ENUMS['TFX_ODE_MAX_STAGES'] == 4 == ode.MAX_STAGES
    assert len(capi.FUNCTIONS['tfx_ode_rk_stage'][1]) == len(capi.FUNCTIONS['tfx_ode_stage'][1])
    assert len(capi.FUNCTIONS['tfx_ode_rk_update'][1]) == len(capi.FUNCTIONS['tfx_ode_update'][1])
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and all(tok in v for tok in (b'laser', b'muon', b'selfflow', b'adamgroups', b'oderk'))
    assert v.index(b'oderk') > v.index(b'adamgroups')


def test_host_argument_checks_return_before_any_launch():
    """every refused call below carries pointers no kernel could touch (small integers): a launch would fault, a host check returns its code"""
    lib = capi.lib()
    P = 64                                                   # a non-null pointer value that is never dereferenced on the host
    # tfx_ode_rk_axpy(y, k, k_stride, nk, w0..w3, f_cond, f_uncond, cfg, k_out, out, n, stream)
    ax = lambda y=P, k=P, ks=8, nk=1, fc=P, ko=P, out=P, n=8: lib.tfx_ode_rk_axpy(y, k, ks, nk, 1., 1., 1., 1., fc, None, 1., ko, out, n, None)
    assert ax(n=0) == 0 and ax(n=-3) == 0
    assert ax(y=None) == -1 and ax(fc=None) == -1 and ax(ko=None, out=None) == -1
    assert ax(nk=-1) == -2 and ax(nk=4) == -2
    assert ax(k=None) == -3 and ax(ks=7) == -3
    # tfx_ode_rk_stage(y, k, ctl, B, Lc, dmax, x, H, Lq, dl, rows0, stream)
    st = lambda y=P, k=P, ctl=P, B=2, Lc=3, dmax=8, x=P, H=1, Lq=4, dl=8: lib.tfx_ode_rk_stage(y, k, ctl, B, Lc, dmax, x, H, Lq, dl, None, None)
    assert st(B=0) == 0 and st(Lc=0) == 0 and st(dl=0) == 0
    for kw in (dict(y=None), dict(k=None), dict(ctl=None), dict(x=None), dict(H=0), dict(H=3), dict(Lq=2), dict(dl=9)):
        assert st(**kw) == -1, kw
    # tfx_ode_rk_update(y, k, ctl, B, Lc, dmax, pred, H, Lq, dl, cfg, sel, rows0, stream)
    up = lambda y=P, k=P, ctl=P, B=2, Lc=3, dmax=8, pred=P, H=1, Lq=4, dl=8: lib.tfx_ode_rk_update(y, k, ctl, B, Lc, dmax, pred, H, Lq, dl, 1., None, None, None)
    assert up(B=0) == 0 and up(Lc=0) == 0 and up(dl=0) == 0
    for kw in (dict(y=None), dict(k=None), dict(ctl=None), dict(pred=None), dict(H=0), dict(H=3), dict(Lq=2), dict(dl=9)):
        assert up(**kw) == -1, kw
