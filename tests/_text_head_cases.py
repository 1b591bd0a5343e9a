"""Cases of the chunked cross entropy (csrc/tokenwise.hip tfx_ce_fwd / tfx_ce_bwd, include/tfx.h tfx_ce_chunk_args): inputs, the float64 restatement and the
per-element bounds (not collected: no test_ prefix; imports no GPU code at module level).  Shared by tests/test_text_head_cpu.py (the restatement against
torch.nn.functional.cross_entropy and its autograd gradient) and tests/test_text_head_gpu.py (the kernels through the C ABI).

Inputs of a case (T, V, ld), `inputs`: fp32 logits [T, ld] whose pad columns V .. ld - 1 hold +1e4 (a kernel that read one would see it in every row
statistic) and whose ignored rows hold NaN (an ignored row is not read); labels with
  row 0    a logit of +80 in column V - 3 among values near -80 (the online maximum jumps by 160 late in the row), label in column 0
  row 1    a constant row, label in column V - 1
  rows t >= 3 with t % 5 == 3 (and row 2 of a three-row case) ignored (-1), every other row N(0, 3^2) logits with a random label.

Bounds, derived from the operation count as tests/_tokenwise_cases.py derives them (u = 2^-24, E(n, M) = (n + 8) u M, tol_bf16 = 2^-8 |y| + 2 E):
  S = sum_c exp(l_c - m)   Term c enters a running sum through one exponential of argument l_c - m' (m' the running maximum then, |argument| <= d_c = m - l_c)
                           and is rescaled by exp(m' - m'') whenever the maximum moves, the jumps adding up to at most d_c; __expf(x) is within (1.5 |x| + 3) u
                           relative (the figure _tokenwise_cases.py uses), so the term carries at most (3 d_c + 4 (K + 2)) u from its exponentials - K = the chunks
                           one lane walks, ceil(V / 256) for the narrow kernel (the wide one walks fewer), + 2 for the wave and the LDS combine - and one rounding
                           for every addition above it: 4 K in the lane, 6 + 4 in the combines.  Weighted by the term's share p_c = exp(-d_c) / S:
                               rel_S = (3 sum_c p_c d_c + 8 K + 18) u                       (sum p d is computed in float64 per row)
  lse = m + log S          tol_lse = rel_S + 4 u (|log S| + |m| + |lse|): __logf is v_log_f32 times ln 2 (two roundings of |log S|), the sum one of |lse|.
  acc[0]                   sum over the valid rows of lse_t - l[label_t] onto the value the buffer held: E(n_valid + 1, |init| + sum |lse_t| + |l[label_t]|) + sum tol_lse_t,
                           any order (per-block partial sums, then fp32 atomics).  acc[1]: exact.
  dlogits                  y = (p - [c == label]) s,  p = exp(l_c - lse): the argument is off by tol_lse + u |l_c - lse|, the exponential by (1.5 |l_c - lse| + 3) u,
                           the difference and the product with s = fp32(grad_scale) fp32(*scale_dev) by three roundings:
                               E_d = |s| (p (tol_lse + (2.5 |l_c - lse| + 3) u) + 3 u |p - [c == label]|) + 2^-126        (the last term: fp32 flushes below it)
                           tol = tol_bf16(y, E_d).  Pad columns and ignored rows: exactly zero.
The same bound holds tfx_ce_fwd_bwd (one maximum, no rescale, at most 16 additions per lane at the widths compared): fewer operations of the same kinds.

`dlogits` has one width for its row stride and for the columns a launch zeroes (ld_d), so nothing can lie between two rows: the band behind ld_d is what follows
the LAST row - the buffers of tests/_gemm_cases.py `guarded` with no column padding: GUARD rows in front and behind, which hold the 8 columns behind the last
row and the whole row after T.  `lse` is guarded the same way."""
import math
from types import SimpleNamespace

import torch

from _gemm_cases import BF, GUARD, U16, U32, tol_bf16  # noqa: F401

CAP_ROWS_NARROW = 4096            # rows one trip of the capped narrow grid covers: CE_CAP_NARROW = 1024 blocks of four rows (csrc/tokenwise.hip)
CAP_ROWS_WIDE = 2048              # ... and of the wide grid: CE_CAP_WIDE blocks of one row
WIDE_LD = 1024                    # CE_WIDE_LD: wider rows take a block each
CASES = ((5, 395, 448),           # the shipped vocabulary, fewer rows than two blocks hold
         (67, 1000, 1024),        # V % 8 == 0, V < ld; the widest narrow row
         (33, 4099, 4160),        # odd V, the wide path: a block walks the row in four full trips and a fifth of one ragged chunk
         (3, 32003, 32064),       # a real tokenizer's width, three rows
         (CAP_ROWS_NARROW + 5, 395, 448),      # a second trip of the capped grid at the narrowest width, ragged (T % 4 == 1): 7.3 MB of logits
         (CAP_ROWS_WIDE + 3, 1030, 1032))      # ... and of the wide grid at its narrowest width, V % 4 == 2: 8.5 MB
FUSED_CASES = CASES[:2]           # also against tfx_ce_fwd_bwd
PAD_VALUE = 1e4
ACC_INIT = (1.5, 2.0)             # what `acc` holds before a launch: the kernels add


def case_id(c):
    return 'T{}_V{}_ld{}'.format(*c)


def inputs(T, V, ld, device='cpu'):
    """(logits fp32 [T, ld], labels int32 [T]) of a case, deterministic"""
    g = torch.Generator(device='cpu').manual_seed(7919 * T + 31 * V + ld)
    lg = torch.randn(T, ld, generator=g) * 3.0
    lab = torch.randint(0, V, (T,), generator=g, dtype=torch.int64).to(torch.int32)
    lg[0] = -80.0 + 0.5 * torch.randn(ld, generator=g)
    lg[0, V - 3] = 80.0
    lab[0] = 0
    lg[1] = 1.25
    lab[1] = V - 1
    ign = torch.zeros(T, dtype=torch.bool)
    ign[3::5] = True
    if T == 3:
        ign[2] = True
    lab[ign] = -1
    lg[ign] = float('nan')
    lg[:, V:] = PAD_VALUE
    return lg.to(device), lab.to(device)


def ce_ref(logits, labels, V, scale=1.0):
    """the float64 restatement: per-row lse (0 for ignored rows), sum of lse - l[label] over the valid rows, their count, d logits [T, V] (zero rows where ignored),
    and the softmax p (for the bounds)"""
    x = logits[:, :V].double()
    valid = labels >= 0
    x = torch.where(valid[:, None], x, torch.zeros_like(x))
    m = x.max(dim=1).values
    S = (x - m[:, None]).exp().sum(dim=1)
    lse = m + S.log()
    lab = labels.long().clamp(min=0)
    picked = x.gather(1, lab[:, None])[:, 0]
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    p = (x - lse[:, None]).exp()
    onehot = torch.zeros_like(p).scatter_(1, lab[:, None], 1.0)
    d = torch.where(valid[:, None], (p - onehot) * scale, torch.zeros_like(p))
    lse = torch.where(valid, lse, torch.zeros_like(lse))
    return SimpleNamespace(lse=lse, loss=loss, count=valid.sum().double(), d=d, p=p, onehot=onehot, valid=valid, m=m, S=S, x=x, picked=picked)


def bounds(r, V, scale=1.0, acc0=ACC_INIT[0]):
    """(tol_lse [T], tol of acc[0], tol of d logits [T, V]) for the reference `r` of ce_ref"""
    K = math.ceil(V / 256)
    dist = r.m[:, None] - r.x
    share = (-dist).exp() / r.S[:, None]
    rel_S = (3 * (share * dist).sum(dim=1) + 8 * K + 18) * U32
    tol_lse = rel_S + 4 * U32 * (r.S.log().abs() + r.m.abs() + r.lse.abs())
    tol_lse = torch.where(r.valid, tol_lse, torch.zeros_like(tol_lse))
    n_valid = int(r.valid.sum())
    mag = abs(acc0) + torch.where(r.valid, r.lse.abs() + r.picked.abs(), torch.zeros_like(r.lse)).sum()
    tol_loss = (n_valid + 1 + 8) * U32 * mag + tol_lse.sum()
    arg = (r.x - r.lse[:, None]).abs()
    E_d = abs(scale) * (r.p * (tol_lse[:, None] + (2.5 * arg + 3) * U32) + 3 * U32 * (r.p - r.onehot).abs()) + 2.0 ** -126
    tol_d = tol_bf16(r.d, E_d)
    tol_d = torch.where(r.valid[:, None], tol_d, torch.zeros_like(tol_d))
    return tol_lse, tol_loss, tol_d
