"""Cases of the per-token losses (Transfusion.set_token_losses_(), include/tfx.h tfx_ce_rows_args / tfx_mse_rows_args): the float64 restatements
and the bounds of the row values (not collected: no test_ prefix; imports no GPU code at module level).  Shared by tests/test_token_losses_cpu.py,
tests/test_token_losses_kernels_gpu.py and tests/test_token_losses_gpu.py.  Shapes, inputs, settings and weight patterns are those of
tests/_text_head_cases.py, tests/_text_loss_terms_cases.py and tests/_loss_weight_cases.py.

Semantics.  tfx_ce_rows_fwd is tfx_ce_w_fwd plus one output: a row that counts (label >= 0 and w != 0) stores row_loss = w r, the number it adds to acc[0],
    r = (1 - e) (lse - l_y) + e (lse - (1/V) sum_c l_c) + z lse^2,
and an ignored row stores 0 without being read.  tfx_mse_rows_fwd adds w_r sum_c err^2 to row_sse[r] and to acc[0], and reads no row of weight 0.

Bounds (u = 2^-24).
  row_loss   _text_loss_terms_cases.py derives, from tol_lse, the error e_r of the row term r through its operations: the subtraction lse - l_y
             (e_ce = tol_lse + u |ce|), with smoothing the row mean, the second subtraction and the mix (e_rs), the square of lse (e_sq) and the z term
             (e_r = e_rs + z e_sq + 2 u (|r_s| + z sq)).  The stored value is the ONE product w r on top of that - w is an input, exact - so
                 tol_row = w e_r + u w |r|.
             With z = e = 0 and w = 1 this is tol_lse + 2 u |lse - l_y|.  Ignored rows: exactly zero.
  row_sse    w sum of dl squares.  One square: the subtraction rounds once (u |err|), so err^2 carries 2 u err^2 + u^2 err^2, its own product u err^2:
             (3 u + u^2) err^2 <= 4 u err^2.  The sum of dl non-negative terms in any order: (dl + 8) u sum err^2 (every partial sum is at most the total; 8: the
             slack the project's E(n, M) keeps).  The row reaches memory through at most ld_d / 64 atomic additions of partial sums (one more rounding chain of
             that length) and one product with w per term, which the row's common factor bounds by u w sum err^2:
                 tol_sse = w (4 + dl + 8 + ld_d / 64 + 1) u sum_c err^2.
Nothing here was fitted to what a kernel returns."""
import math

import torch

import _loss_weight_cases as C
import _text_loss_terms_cases as R
from _gemm_cases import U32

SETTINGS, PATTERNS = C.SETTINGS, C.PATTERNS
F64 = torch.float64


def row_term(logits, labels, V, z=0., e=0.):
    """the float64 restatement of the row term, written from the formula alone: [T] values, 0 where the label is < 0"""
    x = logits[:, :V].to(F64)
    lab = labels.long()
    valid = lab >= 0
    x = torch.where(valid[:, None], x, torch.zeros_like(x))
    lse = torch.logsumexp(x, dim=1)
    ly = x.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    z, e = R.f32(z), R.f32(e)
    r = (1 - e) * (lse - ly) + e * (lse - x.mean(dim=1)) + z * lse * lse
    return torch.where(valid, r, torch.zeros_like(r))


def row_sse(pred, flow, w):
    """float64: w_r sum_c (pred - flow)^2 per row"""
    return w.to(F64) * ((pred.to(F64) - flow.to(F64)) ** 2).sum(dim=1)


def row_loss_bounds(r):
    """(tol_lse [T], tol_row [T]) for the reference `r` of _loss_weight_cases.ce_w_ref, by the docstring (the terms are _text_loss_terms_cases.reg_bounds')"""
    u, z, e, V = U32, r.z, r.e, r.V
    tol_lse = R.bounds(r.plain, V, 1.0, R.AUX_INIT[0])[0]
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
    return tol_lse, r.w * e_r + u * r.w * r.row.abs()


def row_sse_bound(pred, flow, w, ld_d):
    dl = pred.shape[1]
    sse = ((pred.to(F64) - flow.to(F64)) ** 2).sum(dim=1)
    return w.to(F64) * (4 + dl + 8 + ld_d // 64 + 1) * U32 * sse


# ---------------------------------------------------------------------------------------------- the flow index
def flow_index_batch(seed=0):
    """a batch with two modality types and a sample without modalities, and BY HAND the (sample, instance number within the sample) of every latent row per type:
    sample 0 = [M0 (2, 3), text, M1 (4,)], sample 1 = [text], sample 2 = [M1 (2,), M1 (3,), text, M0 (1, 2)]"""
    g = torch.Generator().manual_seed(seed)
    t = lambda n: torch.randint(0, 256, (n,), generator=g)
    m = lambda ty, *ax: (ty, torch.randn(*ax, C.DIM_LATENTS[ty], generator=g))
    mods = [[m(0, 2, 3), t(2), m(1, 4)], [t(5)], [m(1, 2), m(1, 3), t(1), m(0, 1, 2)]]
    want = {0: [(0, 0)] * 6 + [(2, 2)] * 2, 1: [(0, 1)] * 4 + [(2, 0)] * 2 + [(2, 1)] * 3}
    return mods, want
