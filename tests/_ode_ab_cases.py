"""References and case tables of the Adams-Bashforth multistep solver tests (not collected: no test_ prefix; imports neither GPU code nor the package).

Written from the statement of the rules (include/tfx.h's contract, the README), NOT from transfusion_pytorch_amd/ode.py or the kernels: its own copy of the
coefficients as exact fractions, an fp64 solver `ab_solve`, the evaluation list of a solve, and an fp64 restatement of one tfx_ode_rk_stage +
tfx_ode_ab_update call with the rounding bounds of each output.  The start-up steps lean on tests/_ode_rk_cases.py, which the tableau tests pin.

  grid t_0 .. t_{S-1}, N = S - 1 steps, g_n = f(t_n, y_n), P the order:
    n <  P - 1:   one step of the start-up rule (the tableau rule of the same order);  g_n -> history slot n mod 3
    n >= P - 1:   y_{n+1} = y_n + sum_j (dt_n beta_j) g_{n-j}: from y, history terms oldest first (j = P - 1 .. 1), the g_n term last;  g_n -> slot n mod 3
"""
import math
from fractions import Fraction as Fr

import torch

import _ode_rk_cases as RK
from _decode_loss_cases import SOLVE_OFFSETS

F64 = torch.float64
U24 = RK.U24
HIST_SLOTS = 3

# name -> (order P, start-up rule, beta_0 .. beta_{P-1}: the weights of g_n, g_{n-1}, ...)
MULTISTEP = {
    'ab2': (2, 'heun2', [Fr(3, 2), Fr(-1, 2)]),
    'ab3': (3, 'heun3', [Fr(23, 12), Fr(-16, 12), Fr(5, 12)]),
    'ab4': (4, 'rk4', [Fr(55, 24), Fr(-59, 24), Fr(37, 24), Fr(-9, 24)]),
}
METHODS = list(MULTISTEP)


def forwards(method, S):
    """evaluations of one solve over S grid points: stages(start) min(P - 1, N) + max(0, N - (P - 1))"""
    P, start, _ = MULTISTEP[method]
    N = S - 1
    return RK.stages(start) * min(P - 1, N) + max(0, N - (P - 1))


def _start_step(method, f, y, t0, t1):
    """one step of the tableau rule `method`, the arithmetic of RK.rk_solve line by line; returns (the new state, k_0 = f(t0, y))"""
    _, c, A, b = RK.TABLEAUS[method]
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
    return y, k[0]


def ab_solve(method, f, y0, ts):
    """the state at ts[-1] of the multistep solve in the dtype of y0 / ts (fp64 in the yardsticks); one call of f per multistep step"""
    P, start, beta = MULTISTEP[method]
    y, g = y0, {}
    for n in range(len(ts) - 1):
        t0, t1 = ts[n], ts[n + 1]
        if n < P - 1:
            y, g[n] = _start_step(start, f, y, t0, t1)
            continue
        dt = t1 - t0
        g[n] = f(t0, y)
        acc = y
        for j in range(P - 1, 0, -1):
            acc = acc + (dt * float(beta[j])) * g[n - j]
        y = acc + (dt * float(beta[0])) * g[n]
        g.pop(n - (P - 1), None)
    return y


def ab_evals(method, S):
    """the evaluation list of a solve over S grid points on an fp64 grid: RK.rk_evals' dicts (t, q, last, wa, wb, w) with three more entries - `store`
    (the slot that receives g, -1 = none: here every step's stage 0 stores, n mod 3), `hr` (3 slots read, oldest first, zero-padded) and `hw` (their fp32
    weights, 0 = not read).  A multistep evaluation is q = 0, last, with its weight of g in wb[0]."""
    P, start, beta = MULTISTEP[method]
    ts, start_evals = RK.rk_evals(start, S)
    ns = RK.stages(start)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    evals = []
    for n in range(S - 1):
        if n < P - 1:
            for e in start_evals[n * ns:(n + 1) * ns]:
                evals.append(dict(e, step=n, store=n % HIST_SLOTS if e['q'] == 0 else -1, hr=[0, 0, 0], hw=[0., 0., 0.]))
            continue
        dt = float(ts[n + 1]) - float(ts[n])
        older = list(range(P - 1, 0, -1))
        wg = f32(dt * float(beta[0]))
        evals.append(dict(t=float(ts[n]), q=0, last=True, wa=[0.] * 3, wb=[wg, 0., 0., 0.], w=[wg], step=n, store=n % HIST_SLOTS,
                          hr=[(n - j) % HIST_SLOTS for j in older] + [0] * (3 - len(older)), hw=[f32(dt * float(beta[j])) for j in older] + [0.] * (3 - len(older))))
    return ts, evals


ab_schedule = RK.rk_schedule                                 # per sample at a global step: (mode, evaluation or None, time)


def ab_ctl(sched):
    """the [16][B] control block of a step: rows 0..8 as RK.rk_ctl, row 9 the slot that receives g, rows 10..12 the slots read, rows 13..15 their weights"""
    ctl = torch.zeros(16, len(sched), dtype=torch.float32)
    ctl[:9] = RK.rk_ctl(sched)
    ctl[9] = -1.
    for i, (_, ev, _) in enumerate(sched):
        if ev is not None:
            ctl[9, i] = ev['store']
            ctl[10:13, i] = torch.tensor(ev['hr'], dtype=torch.float32); ctl[13:16, i] = torch.tensor(ev['hw'])
    return ctl


def ab_reference(y, k, hist, ctl, pred, H, Lq, dl, cfg, sel=None, rows0=None, n_rows=None):
    """one tfx_ode_rk_stage + tfx_ode_ab_update call in fp64 from the header's contract.  y: [B, Lc, dmax]; k, hist: [3, B, Lc, dmax]; ctl: [16, B];
    the rest as RK.rk_reference, whose dict is returned with y / y_w / y_bound of the mode 2 samples redone with the history terms and h / h_w / h_bound
    (the ring) added.  Only what the contract allows to be read enters a sum: a slot whose weight is 0 may hold a NaN."""
    B, Lc, dmax = y.shape
    out = RK.rk_reference(y, k, ctl[:9], pred, H, Lq, dl, cfg, sel=sel, rows0=rows0, n_rows=n_rows)
    y64, k64, h64, p = y.to(F64), k.to(F64), hist.to(F64), pred.to(F64)
    out.update(h=h64.clone(), h_w=torch.zeros(3, B, Lc, dmax, dtype=torch.bool), h_bound=torch.zeros(3, B, Lc, dmax, dtype=F64))
    row0 = lambda h, i: int(rows0[h * B + i]) if rows0 is not None else (h * B + i) * Lq
    for i in range(B):
        mode, q = int(ctl[0, i]), int(ctl[1, i])
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
        store = float(ctl[9, i])
        if store >= 0:
            s = min(int(store), 2)
            out['h'][s, i, :, :dl] = g; out['h_w'][s, i, :, :dl] = True
            out['h_bound'][s, i, :, :dl] = 3 * U24 * fb if H == 2 else 0.
        if mode == 2:
            wb = [float(v) for v in ctl[5:9, i]]
            acc = y64[i, :, :dl].clone()
            mag, n = acc.abs(), 0
            for j in range(q):
                if wb[j] != 0.:
                    acc = acc + wb[j] * k64[j, i, :, :dl]; mag = mag + (wb[j] * k64[j, i, :, :dl]).abs(); n += 1
            for j in range(3):
                w, s = float(ctl[13 + j, i]), min(max(int(ctl[10 + j, i]), 0), 2)
                if w != 0.:
                    acc = acc + w * h64[s, i, :, :dl]; mag = mag + (w * h64[s, i, :, :dl]).abs(); n += 1
            out['y'][i, :, :dl] = acc + wb[q] * g
            out['y_bound'][i, :, :dl] = (n + 4) * U24 * (mag + abs(wb[q]) * fb)
    return out


def solve_bound(method, S, scale):
    """Rounding bound of a whole fp32 solve through the kernels against fp64 `ab_solve`, built as RK.solve_bound is:

        evaluations  x  roundings per update  x  2^-24  x  amplification  x  scale          scale = max|y| + max|c| (the size of a term)

    * roundings per update: an update sums at most P derivative terms; each costs one fmaf rounding and carries the 3 roundings of its guided
      derivative (history entries are stored guided derivatives), and 4 more are allowed as in the per-call bound (terms + 4): 4 P + 4.  A start-up
      stage of the same order has no more terms than that.
    * amplification: the toy fields have |df/dy| <= L = 0.5 + cfg 0.2 = 0.9.  An error e in the states and in the stored derivatives (L e each) enters
      y_{n+1} = y_n + dt sum_j beta_j g_{n-j} as at most e (1 + dt L sum_j |beta_j|) - the Lipschitz bound is multiplied by sum|beta_j| because the
      beta alternate in sign and the terms need not cancel - so over unit time by at most exp(L sum|beta_j|).  A start-up step of a tableau rule at
      dt L <= 0.13 amplifies by less than exp(2 dt L) (rk4: b sums to 1, its stage inputs grow a perturbation by at most 1.42), which the same factor
      covers since sum|beta_j| >= 2 for every rule here.
    The factor is exp(1.8) / exp(3.3) / exp(6.0) for ab2 / ab3 / ab4: a bound on rounding, not a test of the coefficients - those are pinned element
    by element."""
    P, _, beta = MULTISTEP[method]
    return forwards(method, S) * (4 * P + 4) * U24 * math.exp(0.9 * float(sum(abs(b) for b in beta))) * scale
