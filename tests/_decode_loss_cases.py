"""References and case tables of the decode-side and loss kernel tests (not collected: no test_ prefix; imports neither GPU code nor the library).

Everything here is fp64 torch on CPU tensors, written from the semantics stated in include/tfx.h and the reference lines it cites - not from the kernels:

  draw_reference / u_for     tfx_sample_tokens(_range): sample_text_token + min_p_filter (T:591-605), generate_text_only's text-only draw (T:2695-2698)
  ode_reference              tfx_ode_stage + tfx_ode_update: the fixed-grid midpoint solver as a per-sample state machine (T:2468-2525)
  mse_reference              tfx_mse_fwd_bwd: flow / velocity / reconstruction losses (T:3359-3362, MP:177-200) with model_output_clean (MP:100-126)

tests/test_decode_loss_refs_cpu.py pins these references to something other than the kernels (torchdiffeq's odeint, the reference's three sampling
steps restated, the header's closed-form gradient); tests/test_decode_loss_kernels_gpu.py holds the kernels against them.
"""
import math

import torch

F64 = torch.float64

# ---------------------------------------------------------------------------------------------- case tables
SAMPLE_SHAPES = [(1, 70, 70, 72), (5, 390, 256, 392), (7, 390, 64, 448), (6, 390, 65, 392), (4, 300, 1, 304), (9, 392, 390, 392)]   # (B, V, V_draw, ld)
SAMPLE_MODES = [(1.0, 0.1), (0.7, 0.3), (2.0, 0.0)]                                                                                 # (temperature, min_p)
# per shape: (seed of its B rows, seed of the 64 rows of the u -> 1 edge).  The first seeds from 0 / 1000 at which, in every mode, no column's
# exp((l - l_max) / T) lies within a relative 1e-3 of min_p and every row keeps its targets (the tests assert both before they call)
SAMPLE_SEEDS = {(1, 70, 70, 72): (0, 1002), (5, 390, 256, 392): (4, 1003), (7, 390, 64, 448): (2, 1003), (6, 390, 65, 392): (0, 1002),
                (4, 300, 1, 304): (0, 1353), (9, 392, 390, 392): (11, 1003)}
ODE_SHAPE = dict(B=5, Lc=7, Lq=9, dmax=12)
ODE_MODES = [1, 2, 0, 3, 1]
ODE_COEF = [0.25, -0.5, 0.75, 0.125, 1.5]
MSE_SHAPES = [(37, 5, 8, 64), (300, 48, 48, 64), (8200, 16, 16, 64)]                 # (R, dl, ld_pred, ld_d); the last: R ld_d > 2048 x 256 threads
CLEAN_EPS = 0.05
CE_SHAPES = [(3, 512, 512, 512), (1000, 390, 392, 448), (777, 513, 516, 516), (4100, 390, 392, 392), (1, 70, 72, 72)]   # (T, V, ld, ld_d)


# ---------------------------------------------------------------------------------------------- sampling
def draw_reference(logits, V, V_draw, T, min_p):
    """(keep, q) over the columns [0, V_draw): p = softmax(logits[:, :V] / T) over ALL V columns; a column survives when p >= min_p max(p) and it
    lies inside the draw range; q = the survivors' probabilities (unnormalised: they sum to the surviving mass), 0 elsewhere."""
    p = (logits[:, :V].to(F64) / T).softmax(-1)
    col = torch.arange(V)
    keep = (p >= min_p * p.amax(-1, keepdim=True)) & (col < V_draw)[None]
    q = torch.where(keep, p, torch.zeros_like(p))
    return keep[:, :V_draw], q[:, :V_draw]


def u_for(q, k):
    """the uniform that lands in the middle of survivor k's cell of the inverse CDF (index order): (cdf[k - 1] + q[k] / 2) / total, formed in fp64 and
    rounded to fp32.  q: [B, V_draw] fp64; k: [B] long."""
    cdf = q.cumsum(-1)
    qk = q.gather(1, k[:, None])[:, 0]
    below = cdf.gather(1, k[:, None])[:, 0] - qk
    return ((below + qk / 2) / cdf[:, -1]).to(torch.float32)


def sample_logits(B, V, V_draw, ld, seed):
    """fp32 logits [B, ld]: 3 N(0, 1) in the V valid columns, 1e9 in the pad columns (they must never be looked at).  With V_draw < V the columns
    outside the draw range are capped 0.5 below the best text logit, and every second row then gets its global maximum at a column >= V_draw, 0.3
    above the best text logit: the min-p threshold hangs on a column outside the draw range while text survivors remain (exp(-0.3 / T) >= 0.65 is
    far above every min_p used)."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, ld, generator=g) * 3.
    lg[:, V:] = 1e9
    if V_draw < V:
        for r in range(B):
            top = lg[r, :V_draw].max()
            lg[r, V_draw:V] = torch.minimum(lg[r, V_draw:V], top - 0.5)
            if r % 2 == 0:
                lg[r, V_draw + int(torch.randint(0, V - V_draw, (1,), generator=g))] = top + 0.3
    return lg


def min_p_margin(logits, V, T, min_p):
    """smallest relative distance of any column's exp((l - l_max) / T) from the min-p threshold (fp64): the filter of a test row must not hang on a rounding"""
    if min_p == 0.:
        return math.inf
    l = logits[:, :V].to(F64)
    r = ((l - l.amax(-1, keepdim=True)) / T).exp()
    return float(((r - min_p).abs() / min_p).min())


def draw_targets(keep, q, min_cell=1e-3):
    """per row the survivors worth aiming at: the first, the last, the one that follows the longest run of filtered columns, the ones nearest columns 63
    and 64 (the kernel scans 64 columns per trip) - those whose cell holds at least `min_cell` of the row's surviving mass, without repeats."""
    out = []
    for r in range(keep.shape[0]):
        idx = keep[r].nonzero().flatten()
        if idx.numel() == 0:
            out.append([]); continue
        cand = [int(idx[0]), int(idx[-1])]
        prev = torch.cat([torch.tensor([-1]), idx[:-1]])
        cand.append(int(idx[int((idx - prev).argmax())]))
        for col in (63, 64):
            cand.append(int(idx[int((idx - col).abs().argmin())]))
        tot = float(q[r].sum())
        seen = []
        for k in cand:
            if k not in seen and float(q[r, k]) >= min_cell * tot:
                seen.append(k)
        out.append(seen)
    return out


# ---------------------------------------------------------------------------------------------- ODE state machine
def ode_reference(y, ym, ctl, pred, H, Lq, dl, cfg, sel=None, rows0=None, n_rows=None):
    """tfx_ode_stage followed by tfx_ode_update (include/tfx.h), as plain loops over (sample i, row j, column c).

    y, ym: [B, Lc, dmax]; ctl: [2, B] = (mode, coefficient a) per sample; rows0: None or a list of H B first rows (negative = that half carries no
    block); sel: None or B numbers (0 = skip the sample in the update).  `pred` is a [rows, dl] tensor, a callable x -> pred (the whole-solve
    drivers: the field is evaluated on the staged rows), or None (stage only).
    Returns x, y', ym' (fp64) and boolean masks x_w, y_w, ym_w of the elements the calls may write."""
    B, Lc, dmax = y.shape
    n_rows = H * B * Lq if n_rows is None else n_rows
    y, ym = y.to(F64).clone(), ym.to(F64).clone()
    x = torch.full((n_rows, dl), float('nan'), dtype=F64)
    x_w = torch.zeros(n_rows, dl, dtype=torch.bool)
    y_w, ym_w = torch.zeros(B, Lc, dmax, dtype=torch.bool), torch.zeros(B, Lc, dmax, dtype=torch.bool)
    mode = [int(ctl[0][i]) for i in range(B)]
    coef = [float(ctl[1][i]) for i in range(B)]

    def row0(h, i):
        return int(rows0[h * B + i]) if rows0 is not None else (h * B + i) * Lq

    for i in range(B):                                      # stage: the evaluation input of every sample that is inside a modality
        if mode[i] == 0:
            continue
        src = ym if mode[i] == 2 else y
        for h in range(H):
            r0 = row0(h, i)
            if r0 < 0:
                continue
            for j in range(Lc):
                for c in range(dl):
                    x[r0 + j, c] = src[i, j, c]; x_w[r0 + j, c] = True
    if pred is None:
        return x, y, ym, x_w, y_w, ym_w
    p = (pred(x) if callable(pred) else pred).to(F64)
    for i in range(B):                                      # update: first evaluation -> midpoint, second -> the step's end
        if mode[i] not in (1, 2) or (sel is not None and float(sel[i]) == 0.):
            continue
        rs = [row0(h, i) for h in range(H)]
        if min(rs) < 0:
            continue
        for j in range(Lc):
            for c in range(dl):
                f = p[rs[0] + j, c]
                if H == 2:
                    u = p[rs[1] + j, c]
                    f = u + cfg * (f - u)
                v = y[i, j, c] + coef[i] * f
                if mode[i] == 1:
                    ym[i, j, c] = v; ym_w[i, j, c] = True
                else:
                    y[i, j, c] = v; y_w[i, j, c] = True
    return x, y, ym, x_w, y_w, ym_w


def ode_evals(S):
    """the (time, coefficient, mode) list of a solve over S grid points, as sampling.py's continuous decode loop builds it - on an fp64 grid, so that
    the grid torchdiffeq walks is the same numbers"""
    ts = torch.linspace(0, 1, S, dtype=F64)
    evals = []
    for k in range(S - 1):
        t0, dt = float(ts[k]), float(ts[k + 1] - ts[k])
        evals += [(t0, dt * 0.5, 1), (t0 + dt * 0.5, dt, 2)]
    return ts, evals


SOLVE_S = 8
SOLVE_OFFSETS = [0, 1, 2, 3, 5]                            # sample i starts its solve at global step SOLVE_OFFSETS[i]: idle before, finished after
CFG_SCALE = 3.


def solve_fields(B, Lc, dl, seed=0):
    g = torch.Generator().manual_seed(seed)
    y0 = torch.randn(B, Lc, dl, generator=g, dtype=F64)
    c = torch.randn(B, Lc, dl, generator=g, dtype=F64)
    cu = torch.randn(B, Lc, dl, generator=g, dtype=F64)
    return y0, c, cu


def solve_schedule(step, evals, offsets=SOLVE_OFFSETS):
    """per sample at global step `step`: (mode, coefficient, time) - mode 0 before its solve starts, 3 once it has finished (re-encoded at t = 1)"""
    out = []
    for off in offsets:
        k = step - off
        if k < 0:
            out.append((0, 0., 0.))
        elif k >= len(evals):
            out.append((3, 0., 1.))
        else:
            t, a, m = evals[k]
            out.append((m, a, t))
    return out


def solve_steps(evals, offsets=SOLVE_OFFSETS):
    return max(offsets) + len(evals) + 1                    # the last sample's last evaluation, then one step in which it is finished too


def solve_rows0(B, H, Lc, sched, seed):
    """a compacted row table for one step: only the samples with a block this step get rows, in shuffled order; everyone else -1.  Returns (rows0, rows)"""
    g = torch.Generator().manual_seed(seed)
    live = [(h, i) for h in range(H) for i in range(B) if sched[i][0] != 0]
    order = torch.randperm(len(live), generator=g).tolist()
    rows0 = [-1] * (H * B)
    for slot, k in enumerate(order):
        h, i = live[k]
        rows0[h * B + i] = slot * Lc
    return rows0, max(len(live), 1) * Lc


def solve_pred(x, sched, c, cu, H, Lq, rows0):
    """the toy fields on the staged rows: f(t, y) = cos(3 t) c - 0.5 y in the conditional half, fu(t, y) = cos(3 t) c' - 0.3 y in the null-text half.
    x: [rows, dl] of any dtype / device; c, cu: [B, Lc, dl] on x's device.  Rows no block owns keep whatever they hold."""
    B, Lc, dl = c.shape
    pred = x.clone()
    for h in range(H):
        for i in range(B):
            r0 = rows0[h * B + i] if rows0 is not None else (h * B + i) * Lq
            if r0 < 0 or sched[i][0] == 0:
                continue
            ct = math.cos(3. * sched[i][2])
            k, d = (c, 0.5) if h == 0 else (cu, 0.3)
            pred[r0:r0 + Lc] = (ct * k[i] - d * x[r0:r0 + Lc].to(k.dtype)).to(x.dtype)
    return pred


def solve_field(c, cu, H, cfg=CFG_SCALE):
    """the same field as a torchdiffeq `func` for ONE sample (c, cu: [Lc, dl])"""
    def f(t, y):
        ct = math.cos(3. * float(t))
        fc = ct * c - 0.5 * y
        if H == 1:
            return fc
        fu = ct * cu - 0.3 * y
        return fu + cfg * (fc - fu)
    return f


# ---------------------------------------------------------------------------------------------- MSE modes
def mse_reference(pred, flow, noise, t_row, grad_scale, clean_eps=None, recon_w=None, recon_mode=0, old=None):
    """(sum of the weighted squared error, d pred) of tfx_mse_fwd_bwd, fp64, the gradient by autograd.

    pred, flow, noise: [R, dl] (flow = clean - noise, so clean = noise + flow and noised = t clean + (1 - t) noise); t_row: [R] the row's time.
      plain               loss = sum (pred - flow)^2                                              (T:3359-3362; the velocity target T:3394-3418 alike)
      recon_w, mode 0     loss = sum_r w_r sum_c (noised - (noise + pred (1 - t)))^2             (interleaved forward, T:2840-2853)
      recon_w, mode 1     loss = sum_r w_r sum_c (clean - (noise + pred (1 - t)))^2              (forward_modality, MP:177-200)
      clean_eps           `pred` is what tfx_output_to_flow made of a model output: out -> (out - noised) / max(1 - t, clean_eps) (MP:100-126); the
                          gradient is taken with respect to that OUTPUT (here: the output that gives exactly `pred`)
    The gradient is that of (grad_scale / 2) loss (grad_scale = 2 weight / (R dl)); with `old` (accumulate) the result is old + gradient."""
    pred, flow, noise, t = pred.to(F64), flow.to(F64), noise.to(F64), t_row.to(F64)[:, None]
    clean = noise + flow
    noised = t * clean + (1 - t) * noise
    if clean_eps is not None:
        den = (1 - t).clamp(min=clean_eps)
        leaf = (pred * den + noised).detach().requires_grad_(True)
        p = (leaf - noised) / den
    else:
        leaf = pred.detach().clone().requires_grad_(True)
        p = leaf
    if recon_w is None:
        loss = ((p - (clean - noise)) ** 2).sum()
    else:
        target = noised if recon_mode == 0 else clean
        loss = (recon_w.to(F64)[:, None] * (target - (noise + p * (1 - t))) ** 2).sum()
    (g,) = torch.autograd.grad(0.5 * grad_scale * loss, leaf)
    if old is not None:
        g = old.to(F64) + g
    return loss.detach(), g


def mse_closed_form(pred, flow, t_row, grad_scale, clean_eps=None, recon_w=None, recon_mode=0):
    """the gradient as include/tfx.h states it: grad_scale w (1 - t) r with r = (1 - t) pred - c flow (c = t for recon_mode 0, 1 for recon_mode 1; plain:
    grad_scale (pred - flow)), times 1 / max(1 - t, clean_eps) in clean mode"""
    pred, flow, t = pred.to(F64), flow.to(F64), t_row.to(F64)[:, None]
    if recon_w is None:
        g = grad_scale * (pred - flow)
    else:
        r = (1 - t) * pred - (t if recon_mode == 0 else 1.) * flow
        g = grad_scale * recon_w.to(F64)[:, None] * (1 - t) * r
    if clean_eps is not None:
        g = g / (1 - t).clamp(min=clean_eps)
    return g


def mse_inputs(R, dl, seed=0):
    """fp32 pred / flow / noise [R, dl], instance times (0, 1 and 1 - CLEAN_EPS / 2 among them: the clamp of the clean mode is active), a row -> instance
    map that uses every instance, and per-row reconstruction weights with zero rows"""
    g = torch.Generator().manual_seed(seed)
    pred, flow, noise = (torch.randn(R, dl, generator=g) for _ in range(3))
    times = torch.cat([torch.tensor([0., 1., 1. - CLEAN_EPS / 2]), torch.rand(4, generator=g)])
    row_inst = (torch.arange(R) % times.numel()).to(torch.int32)
    w = torch.rand(R, generator=g) / 3.
    w[::5] = 0.
    return pred, flow, noise, times, row_inst, w


MSE_MODES = {                                                # name -> (clean, recon_mode or None)
    'plain': (False, None), 'clean': (True, None), 'recon0': (False, 0), 'recon1': (False, 1), 'recon0_clean': (True, 0), 'recon1_clean': (True, 1),
}
