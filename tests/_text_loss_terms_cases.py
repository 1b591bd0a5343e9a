"""Cases of the cross entropy with a z-loss and label smoothing (csrc/tokenwise.hip tfx_ce_reg_fwd_bwd / tfx_ce_reg_fwd / tfx_ce_reg_bwd, include/tfx.h
tfx_ce_reg_args): the float64 restatement and the per-element bounds (not collected: no test_ prefix; imports no GPU code at module level).  Shapes, inputs, the
plain restatement and the plain bounds are those of tests/_text_head_cases.py: its six shapes are the smallest at which these kernels can go wrong (the narrow
fast path, the widest narrow row, the wide path with a ragged fifth trip, a 32 k row, the second trip of each capped grid), pad columns hold 1e4, ignored rows NaN.
Shared by tests/test_text_loss_terms_cpu.py and tests/test_text_loss_terms_gpu.py.

Semantics (tfx.h), per valid row with the launch's V columns, lse = log sum_c exp l_c, p_c = exp(l_c - lse), z >= 0, 0 <= e < 1:
    r        = (1 - e) (lse - l_y) + e (lse - (1/V) sum_c l_c) + z lse^2
    d r / d l_c = p_c (1 + 2 z lse) - (1 - e) [c == y] - e / V
The weights of the restatement are the fp32 values the kernels receive (z, e rounded to fp32 once, then exact in float64); 1 / V is exact.

SETTINGS.  (z, e) = (1e-2, 0), (0, 0.1), (1e-2, 0.1).  z is that large on purpose: at 1e-4 the factor 1 + 2 z lse stays inside the bf16 rounding of d logits and
no row would notice a missing term (test_text_loss_terms_cpu.py asserts that the settings used ARE noticed, under the bounds below).

Bounds, in the style of _text_head_cases.py (u = 2^-24, E(n, M) = (n + 8) u M, tol_bf16 = 2^-8 |y| + 2 E; tol_lse and the error of p are that module's):
  ce = lse - l_y           e_ce = tol_lse + u |ce|                                                   (one subtraction)
  sq = lse^2               e_sq = 2 |lse| tol_lse + tol_lse^2 + u sq                                 (the error of lse through the square, one product)
  sl = sum_c l_c           V terms, in any order that keeps the depth of the kernels' sums: a term passes through at most D additions - ceil(V / 64) in a lane
                           (the strided pass of tfx_ce_reg_fwd_bwd, one column per lane and trip; every other kernel walks fewer), 2 for the pairs inside a
                           16-byte chunk, 6 in the wave, 4 in the LDS combine - and each addition rounds a partial sum no larger than sum_c |l_c|:
                               e_sl = (ceil(V / 64) + 12) u sum_c |l_c|
                           (the order-free figure E(V, sum |l_c|) = (V + 8) u sum |l_c| also holds, but at V = 32003 it is 62 times this one and lets smoothing
                           alone vanish inside the bound of the three-row case's loss sum: test_bounds_cannot_hide_a_dead_term).  Formed only when e > 0.
  mu = sl fp32(1 / V)      e_mu = e_sl / V + 2 u |mu|                                                (the rounding of 1 / V, one product)
  t  = lse - mu            e_t  = tol_lse + e_mu + u |t|                                             (the first of the two extra subtractions)
  r_s = (1 - e) ce + e t   e_rs = (1 - e) e_ce + e e_t + 3 u ((1 - e) |ce| + e |t|)                   (the rounding of 1 - e, two products, one sum: at most three roundings
                           on the way of either term).  With e = 0 the kernels take r_s = ce: e_rs = e_ce.
  r  = r_s + z sq          e_r  = e_rs + z e_sq + 2 u (|r_s| + z sq)                                 (one product, one sum)
  acc[0]                   sum of r over the valid rows onto the value the buffer held, any order: E(n_valid + 1, |init| + sum_t M_t) + sum_t e_r,
                           M_t = (1 - e) (|lse| + |l_y|) + e (|lse| + |mu|) + z sq >= |r_t|.  acc[1]: exact.
  aux[0]                   the plain sum: _text_head_cases.bounds' figure for acc[0], on aux's own initial value.
  aux[1]                   sum of sq: E(n_valid + 1, |init| + sum_t sq) + sum_t e_sq.
  d logits                 y = (p k - (1 - e) [c == y] - e / V) s,  k = 1 + 2 z lse:
                             p    e_p = p (tol_lse + (2.5 |l_c - lse| + 3) u)                         (as _text_head_cases: the argument's error, the exponential's)
                             k    e_k = 2 z tol_lse + u (2 z |lse| + |k|)                             (2 z is exact; one product, one sum: tol_lse enters a second time)
                             p k  e_p k + p e_k + u p k
                             the constants: u (1 - e) [c == y] for 1 - e, 2 u e / V for e fp32(1 / V)
                             the two extra subtractions: each one rounding of a partial result no larger than p k + (1 - e) [c == y] + e / V
                             s = fp32(grad_scale) fp32(*scale_dev) and the product with it: 2 u |y / s|
                               E_d = |s| (e_p k + p e_k + u p k + u (1 - e) [c == y] + 2 u e / V + 2 u (p k + (1 - e) [c == y] + e / V) + 2 u |y / s|) + 2^-126
                           tol = tol_bf16(y, E_d).  Pad columns and ignored rows: exactly zero.
The same bounds hold tfx_ce_reg_fwd_bwd (one maximum, no rescale, a shorter sum per lane): fewer operations of the same kinds.  Nothing here was fitted to what a
kernel returns."""
import math
from types import SimpleNamespace

import torch

from _text_head_cases import ACC_INIT, CASES, FUSED_CASES, WIDE_LD, bounds, case_id, ce_ref, inputs  # noqa: F401
from _gemm_cases import U32, tol_bf16

SETTINGS = ((1e-2, 0.0), (0.0, 0.1), (1e-2, 0.1))      # (z, e) of the kernel tests
AUX_INIT = (0.75, 3.0)                                 # what `aux` holds before a launch: the kernels add


def setting_id(s):
    return 'z{:g}_e{:g}'.format(*s)


def f32(v):
    """the fp32 value a kernel receives for the Python float v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32).double())


def reg_ref(logits, labels, V, z, e, scale=1.0):
    """the float64 restatement: ce_ref's fields (lse, p, onehot, valid, x, picked ...) plus, per row, ce / sq / mu / t / rs / row (zero where ignored), the
    three sums `loss` (regularised), `ce_sum`, `sq_sum`, the count, and d logits [T, V] `d` at `scale`"""
    z, e = f32(z), f32(e)
    b = ce_ref(logits, labels, V)
    valid = b.valid
    zero = torch.zeros_like(b.m)
    lse = b.m + b.S.log()                                   # (b.lse is zeroed on ignored rows; their x is zero, so this is finite everywhere)
    ce = lse - b.picked
    sq = lse * lse
    mu = b.x.sum(dim=1) / V
    t = lse - mu
    rs = (1 - e) * ce + e * t
    row = rs + z * sq
    k = 1 + 2 * z * lse
    d = (b.p * k[:, None] - (1 - e) * b.onehot - e / V) * scale
    d = torch.where(valid[:, None], d, torch.zeros_like(d))
    w = lambda v: torch.where(valid, v, zero)
    return SimpleNamespace(lse=b.lse, lse_all=lse, p=b.p, onehot=b.onehot, valid=valid, x=b.x, picked=b.picked, m=b.m, S=b.S, plain=b, z=z, e=e, V=V,
                           ce=w(ce), sq=w(sq), mu=w(mu), t=w(t), rs=w(rs), row=w(row), k=k, d=d, count=valid.sum().double(),
                           loss=w(row).sum(), ce_sum=w(ce).sum(), sq_sum=w(sq).sum())


def reg_bounds(r, scale=1.0, acc0=ACC_INIT[0], aux0=AUX_INIT):
    """(tol_lse [T], tol of acc[0], tol of aux[0], tol of aux[1], tol of d logits [T, V]) for the reference `r` of reg_ref, by the docstring's derivation"""
    V, z, e, u = r.V, r.z, r.e, U32
    tol_lse, tol_ce_sum, _ = bounds(r.plain, V, 1.0, aux0[0])
    valid, zero = r.valid, torch.zeros_like(r.m)
    w = lambda v: torch.where(valid, v, zero)
    lse = r.lse_all
    e_ce = tol_lse + u * r.ce.abs()
    e_sq = 2 * lse.abs() * tol_lse + tol_lse ** 2 + u * r.sq
    if e > 0:
        e_sl = (math.ceil(V / 64) + 12) * u * r.x.abs().sum(dim=1)
        e_mu = e_sl / V + 2 * u * r.mu.abs()
        e_t = tol_lse + e_mu + u * r.t.abs()
        e_rs = (1 - e) * e_ce + e * e_t + 3 * u * ((1 - e) * r.ce.abs() + e * r.t.abs())
    else:
        e_rs = e_ce
    e_r = e_rs + z * e_sq + 2 * u * (r.rs.abs() + z * r.sq)
    n_valid = int(valid.sum())
    M = (1 - e) * (lse.abs() + r.picked.abs()) + e * (lse.abs() + r.mu.abs()) + z * r.sq
    tol_loss = (n_valid + 1 + 8) * u * (abs(acc0) + w(M).sum()) + w(e_r).sum()
    tol_sq_sum = (n_valid + 1 + 8) * u * (abs(aux0[1]) + w(r.sq).sum()) + w(e_sq).sum()
    # ---- d logits
    arg = (r.x - lse[:, None]).abs()
    e_p = r.p * (tol_lse[:, None] + (2.5 * arg + 3) * u)
    k = r.k.abs()[:, None]
    e_k = (2 * z * tol_lse + u * (2 * z * lse.abs() + r.k.abs()))[:, None]
    pk = r.p * k
    oh = (1 - e) * r.onehot
    ev = e / V
    y_over_s = (r.p * r.k[:, None] - oh - ev).abs()
    E_d = abs(scale) * (e_p * k + r.p * e_k + u * pk + u * oh + 2 * u * ev + 2 * u * (pk + oh + ev) + 2 * u * y_over_s) + 2.0 ** -126
    tol_d = tol_bf16(r.d, E_d)
    tol_d = torch.where(valid[:, None], tol_d, torch.zeros_like(tol_d))
    return tol_lse, tol_loss, tol_ce_sum, tol_sq_sum, tol_d
