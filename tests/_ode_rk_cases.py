"""References and case tables of the fixed-grid Runge-Kutta solver tests (not collected: no test_ prefix; imports neither GPU code nor the package).

Everything here is written from the statement of the rules (the issue's table, include/tfx.h's contract), NOT from transfusion_pytorch_amd/ode.py or the
kernels: its own copy of the tableaus as exact fractions, the order conditions of rooted trees through order 4 (and the bushy tree of order 5), an fp64
solver `rk_solve`, and an fp64 restatement of one tfx_ode_rk_stage + tfx_ode_rk_update call with the rounding bounds of each output.

  step from t0 to t1 = t0 + dt:   k_q = f(t0 + c_q dt, y + dt sum_{j<q} a_qj k_j)   (c_q == 1: evaluated at t1 itself);   y <- y + dt sum_q b_q k_q
"""
import math
from fractions import Fraction as Fr

import torch

from _decode_loss_cases import SOLVE_OFFSETS

F64 = torch.float64
MAX_STAGES = 4
U24 = 2. ** -24

# name -> (order, c, A, b); A[q] = weights of k_0 .. k_{q-1} in the input of stage q.  rk4 is torchdiffeq's: the 3/8 rule
TABLEAUS = {
    'euler':    (1, [Fr(0)], [[]], [Fr(1)]),
    'midpoint': (2, [Fr(0), Fr(1, 2)], [[], [Fr(1, 2)]], [Fr(0), Fr(1)]),
    'heun2':    (2, [Fr(0), Fr(1)], [[], [Fr(1)]], [Fr(1, 2), Fr(1, 2)]),
    'heun3':    (3, [Fr(0), Fr(1, 3), Fr(2, 3)], [[], [Fr(1, 3)], [Fr(0), Fr(2, 3)]], [Fr(1, 4), Fr(0), Fr(3, 4)]),
    'rk4':      (4, [Fr(0), Fr(1, 3), Fr(2, 3), Fr(1)], [[], [Fr(1, 3)], [Fr(-1, 3), Fr(1)], [Fr(1), Fr(-1), Fr(1)]], [Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8)]),
}
METHODS = list(TABLEAUS)
NEW_METHODS = [m for m in METHODS if m != 'midpoint']


def stages(method):
    return len(TABLEAUS[method][1])


def order_conditions(method):
    """{order: [lhs - rhs of every rooted-tree condition of that order]} in exact rationals, orders 1 .. 4 complete, order 5 the bushy tree only (a
    method of order 5 would have to meet it: failing it is enough to show the order is below 5)"""
    _, c, A, b = TABLEAUS[method]
    n = len(c)
    a = [[A[i][j] if j < len(A[i]) else Fr(0) for j in range(n)] for i in range(n)]
    S = lambda f: sum((f(i) for i in range(n)), Fr(0))
    ac = [sum((a[i][j] * c[j] for j in range(n)), Fr(0)) for i in range(n)]
    ac2 = [sum((a[i][j] * c[j] ** 2 for j in range(n)), Fr(0)) for i in range(n)]
    aac = [sum((a[i][j] * ac[j] for j in range(n)), Fr(0)) for i in range(n)]
    return {
        1: [S(lambda i: b[i]) - 1],
        2: [S(lambda i: b[i] * c[i]) - Fr(1, 2)],
        3: [S(lambda i: b[i] * c[i] ** 2) - Fr(1, 3), S(lambda i: b[i] * ac[i]) - Fr(1, 6)],
        4: [S(lambda i: b[i] * c[i] ** 3) - Fr(1, 4), S(lambda i: b[i] * c[i] * ac[i]) - Fr(1, 8), S(lambda i: b[i] * ac2[i]) - Fr(1, 12),
            S(lambda i: b[i] * aac[i]) - Fr(1, 24)],
        5: [S(lambda i: b[i] * c[i] ** 4) - Fr(1, 5)],
    }


def rk_solve(method, f, y0, ts):
    """the state at ts[-1] of the fixed-grid solve in the dtype of y0 / ts (fp64 in the yardsticks).  Terms with a zero weight are left out, sums run
    from y with j ascending - for `midpoint` this is the arithmetic of oracle/shims/torchdiffeq to the bit."""
    _, c, A, b = TABLEAUS[method]
    y = y0
    for i in range(len(ts) - 1):
        t0, t1 = ts[i], ts[i + 1]
        dt = t1 - t0
        k = []
        for q in range(len(c)):
            x = y
            for j in range(q):
                if A[q][j] != 0:
                    x = x + k[j] * (dt * float(A[q][j]))
            k.append(f(t1 if c[q] == 1 else t0 + dt * float(c[q]), x))
        for j in range(len(c)):
            if b[j] != 0:
                y = y + (dt * float(b[j])) * k[j]
    return y


def rk_evals(method, S):
    """the evaluation list of a solve over S grid points on an fp64 grid (the grid `rk_solve` walks is the same numbers): per evaluation a dict with
    its time t, stage index q, `last`, the fp32 weights wa (3: input of this stage), wb (4: the step's update) and w (q + 1: what the dense form adds
    after this evaluation - the next stage's input, or the update)"""
    _, c, A, b = TABLEAUS[method]
    ts = torch.linspace(0, 1, S, dtype=F64)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    pad = lambda row, n: [f32(dt * float(a)) for a in row] + [0.] * (n - len(row))
    evals = []
    for k in range(S - 1):
        t0, t1 = float(ts[k]), float(ts[k + 1])
        dt = t1 - t0
        for q in range(len(c)):
            last = q == len(c) - 1
            evals.append(dict(t=t1 if c[q] == 1 else t0 + dt * float(c[q]), q=q, last=last, wa=pad(A[q], 3), wb=pad(b, 4),
                              w=pad(b[:q + 1] if last else A[q + 1], q + 1)))
    return ts, evals


def rk_schedule(step, evals, offsets=SOLVE_OFFSETS):
    """per sample at global step `step`: (mode, evaluation or None, time) - mode 0 before its solve starts, 3 once it has finished (re-encoded at t = 1);
    the tuple layout of _decode_loss_cases.solve_schedule, so that solve_pred / solve_rows0 take it"""
    out = []
    for off in offsets:
        k = step - off
        if k < 0:
            out.append((0, None, 0.))
        elif k >= len(evals):
            out.append((3, None, 1.))
        else:
            out.append((2 if evals[k]['last'] else 1, evals[k], evals[k]['t']))
    return out


def rk_ctl(sched):
    """the [9][B] control block of a step"""
    ctl = torch.zeros(9, len(sched), dtype=torch.float32)
    for i, (mode, ev, _) in enumerate(sched):
        ctl[0, i] = mode
        if ev is not None:
            ctl[1, i] = ev['q']
            ctl[2:5, i] = torch.tensor(ev['wa']); ctl[5:9, i] = torch.tensor(ev['wb'])
    return ctl


def rk_reference(y, k, ctl, pred, H, Lq, dl, cfg, sel=None, rows0=None, n_rows=None):
    """one tfx_ode_rk_stage + tfx_ode_rk_update call in fp64 from the header's contract.  y: [B, Lc, dmax]; k: [3, B, Lc, dmax]; ctl: [9, B] (its fp32
    numbers are the weights on both sides); pred: [rows, dl]; rows0 / sel as in _decode_loss_cases.ode_reference.  Only the elements the contract allows
    to be read enter the sums (so NaN sentinels elsewhere cannot leak into the reference).
    Returns a dict: x, x_w, x_bound (staged rows; the bound is 0 where no term was added: bit-equal), y, y_w, y_bound, k, k_w, k_bound."""
    B, Lc, dmax = y.shape
    n_rows = H * B * Lq if n_rows is None else n_rows
    y64, k64, p = y.to(F64), k.to(F64), pred.to(F64)
    out = dict(x=torch.full((n_rows, dl), float('nan'), dtype=F64), x_w=torch.zeros(n_rows, dl, dtype=torch.bool), x_bound=torch.zeros(n_rows, dl, dtype=F64),
               y=y64.clone(), y_w=torch.zeros(B, Lc, dmax, dtype=torch.bool), y_bound=torch.zeros(B, Lc, dmax, dtype=F64),
               k=k64.clone(), k_w=torch.zeros(3, B, Lc, dmax, dtype=torch.bool), k_bound=torch.zeros(3, B, Lc, dmax, dtype=F64))
    row0 = lambda h, i: int(rows0[h * B + i]) if rows0 is not None else (h * B + i) * Lq
    for i in range(B):
        mode, q = int(ctl[0, i]), int(ctl[1, i])
        wa, wb = [float(v) for v in ctl[2:5, i]], [float(v) for v in ctl[5:9, i]]
        if mode == 0:
            continue
        yi = y64[i, :, :dl]
        # ---- stage
        x, mag, n = yi.clone(), yi.abs(), 0
        if mode != 3:
            for j in range(q):
                if wa[j] != 0.:
                    x = x + wa[j] * k64[j, i, :, :dl]; mag = mag + (wa[j] * k64[j, i, :, :dl]).abs(); n += 1
        for h in range(H):
            r0 = row0(h, i)
            if r0 >= 0:
                out['x'][r0:r0 + Lc] = x; out['x_w'][r0:r0 + Lc] = True
                out['x_bound'][r0:r0 + Lc] = (n + 1) * U24 * mag if n else 0.
        # ---- update
        if mode not in (1, 2) or (sel is not None and float(sel[i]) == 0.):
            continue
        rs = [row0(h, i) for h in range(H)]
        if min(rs) < 0:
            continue
        g = p[rs[0]:rs[0] + Lc]
        fb = g.abs()
        if H == 2:
            u = p[rs[1]:rs[1] + Lc]
            fb = u.abs() + abs(cfg) * (g.abs() + u.abs())
            g = u + cfg * (g - u)
        if mode == 1:
            out['k'][q, i, :, :dl] = g; out['k_w'][q, i, :, :dl] = True
            out['k_bound'][q, i, :, :dl] = 3 * U24 * fb if H == 2 else 0.
        else:
            acc, mag, n = yi.clone(), yi.abs(), 0
            for j in range(q):
                if wb[j] != 0.:
                    acc = acc + wb[j] * k64[j, i, :, :dl]; mag = mag + (wb[j] * k64[j, i, :, :dl]).abs(); n += 1
            out['y'][i, :, :dl] = acc + wb[q] * g; out['y_w'][i, :, :dl] = True
            out['y_bound'][i, :, :dl] = (n + 4) * U24 * (mag + abs(wb[q]) * fb)
    return out


def solve_bound(method, S, scale):
    """rounding bound of a whole fp32 solve through the kernels against fp64 `rk_solve`: stages (S - 1) updates of at most stages + 7 fp32 roundings
    each, amplified by at most e^0.9 (the toy fields contract: |df/dy| <= 0.5 + cfg 0.2 = 0.9 over unit time), times max|y| + max|c|"""
    n = stages(method)
    return n * (S - 1) * (n + 7) * U24 * math.exp(0.9) * scale
