"""Fixed-grid explicit Runge-Kutta solvers of the sampling paths (`odeint_kwargs['method']`).

The reference hands `odeint_kwargs` to `torchdiffeq.odeint`; here the fixed-grid rules of that package are restated as Butcher tableaus in exact
fractions (PARITY UNPINNED: the package is not part of the reference checkout, no reference test runs any of them - like the midpoint rule,
SURVEY Appendix D).  The grid is `t = linspace(0, 1, modality_steps)` itself; one step from t0 to t1 = t0 + dt is

    k_q = f(t0 + c_q dt, y + dt sum_{j<q} a_qj k_j)       q = 0 .. stages - 1          (a stage with c_q == 1 is evaluated at t1 itself)
    y  <- y + dt sum_q b_q k_q

`rk4` is torchdiffeq's: the 3/8 rule, not the classic tableau.  The device side is tfx_ode_rk_stage / tfx_ode_rk_update / tfx_ode_rk_axpy
(include/tfx.h); `midpoint` keeps its own kernels (tfx_ode_stage / tfx_ode_update / tfx_ode_axpy).
"""
from __future__ import annotations

import functools
from collections import namedtuple
from fractions import Fraction as Fr

import numpy as np
import torch

MAX_STAGES = 4                                               # == TFX_ODE_MAX_STAGES (include/tfx.h)

Tableau = namedtuple('Tableau', 'order c A b')               # A[q] = (a_q0 .. a_q,q-1): the weights of k_0 .. k_{q-1} in the input of stage q

TABLEAUS = {
    'euler':    Tableau(1, (Fr(0),), ((),), (Fr(1),)),
    'midpoint': Tableau(2, (Fr(0), Fr(1, 2)), ((), (Fr(1, 2),)), (Fr(0), Fr(1))),
    'heun2':    Tableau(2, (Fr(0), Fr(1)), ((), (Fr(1),)), (Fr(1, 2), Fr(1, 2))),
    'heun3':    Tableau(3, (Fr(0), Fr(1, 3), Fr(2, 3)), ((), (Fr(1, 3),), (Fr(0), Fr(2, 3))), (Fr(1, 4), Fr(0), Fr(3, 4))),
    'rk4':      Tableau(4, (Fr(0), Fr(1, 3), Fr(2, 3), Fr(1)), ((), (Fr(1, 3),), (Fr(-1, 3), Fr(1)), (Fr(1), Fr(-1), Fr(1))),
                        (Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8))),
}
METHODS = tuple(TABLEAUS)
_IGNORED_KEYS = ('atol', 'rtol')                             # tolerances of the adaptive solvers: a fixed-grid solver does not use them


def check_odeint_kwargs(odeint_kwargs) -> str:
    """the solver name of a constructor's `odeint_kwargs`; anything the fixed-grid solvers here cannot honour raises NotImplementedError"""
    kw = dict(odeint_kwargs or {})
    method = kw.pop('method', 'midpoint')
    if method not in TABLEAUS:
        raise NotImplementedError(f'odeint method {method!r} is not implemented: the fixed-grid solvers are {", ".join(METHODS)}')
    extra = [k for k in kw if k not in _IGNORED_KEYS]
    if extra:
        raise NotImplementedError(f'odeint_kwargs {extra} are not implemented: `method` (one of {", ".join(METHODS)}) is honoured, '
                                  f'`atol` / `rtol` are accepted and unused by fixed-grid solvers')
    return method


# one evaluation of the velocity field:
#   t     its time (a Python float)                        q, last   stage index inside its step / whether the step ends with it
#   wa    q weights dt a_qj: the evaluation's INPUT is y + sum_{j<q} wa_j k_j
#   w     q + 1 weights of what FOLLOWS it: y + sum_{j<=q} w_j k_j is the next stage's input (dt a_{q+1,j}), or, after the last stage, the new
#         state (dt b_j)
#   wb    `stages` weights dt b_j of the step's update
# (weights as Python floats that hold the fp32 values the kernels get)
Eval = namedtuple('Eval', 't q last wa w wb')


def _f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


def ode_schedule(method: str, modality_steps: int):
    """the flat evaluation list of one solve over `modality_steps` grid points: stages x (modality_steps - 1) entries, in the order the decode loops
    walk them.  For `midpoint` the times and the coefficients `w[q]` are the numbers the midpoint loops form themselves (t0, t0 + dt / 2; dt / 2, dt)."""
    return list(_schedule(method, int(modality_steps)))


@functools.lru_cache(maxsize=64)                             # (exact fractions, one fp32 rounding per weight: ~1 ms at 16 grid points, paid once)
def _schedule(method, modality_steps):
    tab = TABLEAUS[method]
    ts = torch.linspace(0, 1, modality_steps)
    n = len(tab.c)
    out = []
    for k in range(modality_steps - 1):
        t0, t1, dt = float(ts[k]), float(ts[k + 1]), float(ts[k + 1] - ts[k])
        scale = lambda row: tuple(_f32(Fr(dt) * a) for a in row)
        wb = scale(tab.b)
        for q in range(n):
            last = q == n - 1
            t = t1 if tab.c[q] == 1 else t0 + float(tab.c[q]) * dt
            out.append(Eval(t, q, last, scale(tab.A[q]), wb[:q + 1] if last else scale(tab.A[q + 1]), wb))
    return tuple(out)


# what the continuous decode loop uploads per evaluation (the solver control block of a mixed step, one column per evaluation):
#   times   the evaluation times (a tuple of Python floats)  modes   fp32: 1 = a stage, 2 = the evaluation that ends its step
#   rows    fp32 [1, n] for `midpoint` - the coefficient of tfx_ode_update; [8, n] for the tableau rules - the stage index, the 3 weights of the
#           evaluation's input, the 4 weights of the step's update (tfx_ode_rk_stage / tfx_ode_rk_update)
Control = namedtuple('Control', 'times modes rows')


@functools.lru_cache(maxsize=64)                             # (shared between calls: the arrays are read-only)
def ode_control(method: str, modality_steps: int) -> Control:
    sched = ode_schedule(method, modality_steps)
    modes = np.array([2 if e.last else 1 for e in sched], np.float32)
    if method == 'midpoint':
        rows = np.array([[e.w[e.q] for e in sched]], np.float32)
    else:
        rows = np.zeros((8, len(sched)), np.float32)
        for n, e in enumerate(sched):
            rows[0, n] = e.q; rows[1:1 + e.q, n] = e.wa; rows[4:4 + len(e.wb), n] = e.wb
    modes.flags.writeable = rows.flags.writeable = False
    return Control(tuple(e.t for e in sched), modes, rows)
