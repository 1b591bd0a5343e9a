"""Fixed-grid explicit Runge-Kutta solvers of the sampling paths (`odeint_kwargs['method']`).

The reference hands `odeint_kwargs` to `torchdiffeq.odeint`; here the fixed-grid rules of that package are restated as Butcher tableaus in exact
fractions (PARITY UNPINNED: the package is not part of the reference checkout, no reference test runs any of them - like the midpoint rule,
SURVEY Appendix D).  The grid is `t = linspace(0, 1, modality_steps)` itself; one step from t0 to t1 = t0 + dt is

    k_q = f(t0 + c_q dt, y + dt sum_{j<q} a_qj k_j)       q = 0 .. stages - 1          (a stage with c_q == 1 is evaluated at t1 itself)
    y  <- y + dt sum_q b_q k_q

`rk4` is torchdiffeq's: the 3/8 rule, not the classic tableau.  The device side is tfx_ode_rk_stage / tfx_ode_rk_update / tfx_ode_rk_axpy
(include/tfx.h); `midpoint` keeps its own kernels (tfx_ode_stage / tfx_ode_update / tfx_ode_axpy).

Adams-Bashforth multistep rules on the same grid (`ab2`, `ab3`, `ab4`; PARITY UNPINNED as well - they are NOT torchdiffeq's `explicit_adams`, whose order
ramp and constants cannot be checked without the package, so that name keeps raising).  With g_n = f(t_n, y_n) and P the order:

    n <  P - 1:   one step of the start-up rule (heun2 / heun3 / rk4: the rule of the same order, so the global order stays P), bit for bit what that
                  method does; its stage-0 derivative g_n is also kept in history slot n mod HIST_SLOTS
    n >= P - 1:   ONE evaluation at (t_n, y_n):  y_{n+1} = y_n + sum_j fp32(dt_n beta_j) g_{n-j}, history terms oldest first, the g_n term last;
                  g_n -> slot n mod HIST_SLOTS (for ab4 the slot of g_{n-3}, which the same launch reads first)

That is stages(start) min(P - 1, N) + max(0, N - (P - 1)) evaluations for N = modality_steps - 1 steps: 16 / 19 / 24 at 16 grid points against
midpoint's 30.  With N <= P - 1 the solve IS the start-up rule's.  A store no later step reads (the last step's, every store of such a short grid) is
dropped.  The device side is tfx_ode_rk_stage + tfx_ode_ab_update (state machine) and tfx_ode_rk_axpy / tfx_ode_ab_axpy (dense).
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

HIST_SLOTS = 3                                               # == TFX_ODE_AB_HIST (include/tfx.h): g_{n-1} .. g_{n-3}

Multistep = namedtuple('Multistep', 'order start beta')      # beta[j]: the weight of g_{n-j}; start: the tableau rule of the first order - 1 steps

MULTISTEP = {
    'ab2': Multistep(2, 'heun2', (Fr(3, 2), Fr(-1, 2))),
    'ab3': Multistep(3, 'heun3', (Fr(23, 12), Fr(-16, 12), Fr(5, 12))),
    'ab4': Multistep(4, 'rk4', (Fr(55, 24), Fr(-59, 24), Fr(37, 24), Fr(-9, 24))),
}
MULTISTEP_METHODS = tuple(MULTISTEP)
_IGNORED_KEYS = ('atol', 'rtol')                             # tolerances of the adaptive solvers: a fixed-grid solver does not use them


def check_odeint_kwargs(odeint_kwargs) -> str:
    """the solver name of a constructor's `odeint_kwargs`; anything the fixed-grid solvers here cannot honour raises NotImplementedError"""
    kw = dict(odeint_kwargs or {})
    method = kw.pop('method', 'midpoint')
    if method not in TABLEAUS and method not in MULTISTEP:
        raise NotImplementedError(f'odeint method {method!r} is not implemented: the fixed-grid solvers are {", ".join(METHODS)} and the '
                                  f'Adams-Bashforth rules {", ".join(MULTISTEP_METHODS)} (which are not the explicit_adams / implicit_adams of torchdiffeq)')
    extra = [k for k in kw if k not in _IGNORED_KEYS]
    if extra:
        raise NotImplementedError(f'odeint_kwargs {extra} are not implemented: `method` (one of {", ".join(METHODS)}, '
                                  f'{", ".join(MULTISTEP_METHODS)}) is honoured, `atol` / `rtol` are accepted and unused by fixed-grid solvers')
    return method


# one evaluation of the velocity field:
#   t     its time (a Python float)                        q, last   stage index inside its step / whether the step ends with it
#   wa    q weights dt a_qj: the evaluation's INPUT is y + sum_{j<q} wa_j k_j
#   w     q + 1 weights of what FOLLOWS it: y + sum_{j<=q} w_j k_j is the next stage's input (dt a_{q+1,j}), or, after the last stage, the new
#         state (dt b_j)
#   wb    `stages` weights dt b_j of the step's update
# the multistep rules add (defaults = a tableau rule's evaluation):
#   store the history slot that receives this evaluation's derivative g, -1 = none
#   hr    the history slots a multistep evaluation reads, oldest first;   hw   their weights dt beta_j (its weight of g itself is w[0] == wb[0])
# (weights as Python floats that hold the fp32 values the kernels get)
Eval = namedtuple('Eval', 't q last wa w wb store hr hw', defaults=(-1, (), ()))


def _f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


def ode_schedule(method: str, modality_steps: int):
    """the flat evaluation list of one solve over `modality_steps` grid points: stages x (modality_steps - 1) entries, in the order the decode loops
    walk them.  For `midpoint` the times and the coefficients `w[q]` are the numbers the midpoint loops form themselves (t0, t0 + dt / 2; dt / 2, dt).
    A multistep rule's list is its start-up rule's for the first order - 1 steps, then one entry per step."""
    return list((_multistep_schedule if method in MULTISTEP else _schedule)(method, int(modality_steps)))


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


@functools.lru_cache(maxsize=64)
def _multistep_schedule(method, modality_steps):
    ms = MULTISTEP[method]
    ts = torch.linspace(0, 1, modality_steps)
    start, stages = _schedule(ms.start, modality_steps), len(TABLEAUS[ms.start].c)
    N, P = modality_steps - 1, ms.order
    out = []
    for n in range(N):
        store = n % HIST_SLOTS if N > P - 1 and n < N - 1 else -1          # a later multistep step reads it
        if n < P - 1:
            out += [e._replace(store=store if e.q == 0 else -1) for e in start[n * stages:(n + 1) * stages]]
            continue
        dt = float(ts[n + 1] - ts[n])
        wg = (_f32(Fr(dt) * ms.beta[0]),)
        older = range(P - 1, 0, -1)
        out.append(Eval(float(ts[n]), 0, True, (), wg, wg, store, tuple((n - j) % HIST_SLOTS for j in older), tuple(_f32(Fr(dt) * ms.beta[j]) for j in older)))
    return tuple(out)


# what the continuous decode loop uploads per evaluation (the solver control block of a mixed step, one column per evaluation):
#   times   the evaluation times (a tuple of Python floats)  modes   fp32: 1 = a stage, 2 = the evaluation that ends its step
#   rows    fp32 [1, n] for `midpoint` - the coefficient of tfx_ode_update; [8, n] for the tableau rules - the stage index, the 3 weights of the
#           evaluation's input, the 4 weights of the step's update (tfx_ode_rk_stage / tfx_ode_rk_update); [15, n] for the multistep rules - those 8,
#           the slot that receives g (-1 = none), the 3 slots read, their 3 weights (tfx_ode_ab_update; a multistep evaluation is mode 2 at stage 0)
Control = namedtuple('Control', 'times modes rows')


@functools.lru_cache(maxsize=64)                             # (shared between calls: the arrays are read-only)
def ode_control(method: str, modality_steps: int) -> Control:
    sched = ode_schedule(method, modality_steps)
    modes = np.array([2 if e.last else 1 for e in sched], np.float32)
    if method == 'midpoint':
        rows = np.array([[e.w[e.q] for e in sched]], np.float32)
    else:
        rows = np.zeros((15 if method in MULTISTEP else 8, len(sched)), np.float32)
        for n, e in enumerate(sched):
            rows[0, n] = e.q; rows[1:1 + e.q, n] = e.wa; rows[4:4 + len(e.wb), n] = e.wb
            if method in MULTISTEP:
                rows[8, n] = e.store; rows[9:9 + len(e.hr), n] = e.hr; rows[12:12 + len(e.hw), n] = e.hw
    modes.flags.writeable = rows.flags.writeable = False
    return Control(tuple(e.t for e in sched), modes, rows)
