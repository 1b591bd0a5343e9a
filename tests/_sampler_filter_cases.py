"""Reference and case tables of the filtered text draw, tfx_sample_tokens_filtered (not collected: no test_ prefix; imports neither GPU code nor the
library).  fp64 torch on CPU tensors, written from the semantics stated in include/tfx.h - not from the kernel.  The top-k and top-p filters are not
the reference's (it has min-p only): they are pinned to that text, not to a golden.

tests/test_sampler_filters_cpu.py holds `filter_reference` to an independent restatement (topk, descending sort + cumsum) and the table to its
margins; tests/test_sampler_filters_gpu.py holds the kernel to `filter_reference`.
"""
import functools
import math

import torch

from _decode_loss_cases import F64, SAMPLE_SHAPES, draw_targets, min_p_margin, sample_logits

NARROW_MAX = 1024                                            # include/tfx.h: TFX_SAMPLE_NARROW_MAX, the last width of the one-wave-per-row form
# (B, V, V_draw, ld): the existing shapes; one column; one wave trip exactly; a row of many trips (block-per-row form); one column on either side
# of the width-class boundary, the wide one with a draw range that ends inside the row
FILTER_SHAPES = SAMPLE_SHAPES + [(3, 1, 1, 8), (2, 64, 64, 64), (3, 4100, 4100, 4104), (2, NARROW_MAX, NARROW_MAX, NARROW_MAX),
                                 (2, NARROW_MAX + 1, 1000, NARROW_MAX + 8)]
FILTER_MODES = [(1.0, 0., 0, 0.9), (1.0, 0., 0, 0.3), (0.7, 0., 40, 0.5), (2.0, 0., 5, 1.0), (1.0, 0.1, 20, 0.9), (0.7, 0.3, 3, 0.95),
                (1.0, 0., 1, 1.0), (1.0, 0., 10 ** 6, 1.0)]                                             # (temperature, min_p, top_k, top_p)
NUCLEUS_MARGIN, MIN_P_MARGIN, TOP_K_MARGIN = 1e-4, 1e-3, 1e-6
# NUCLEUS_MARGIN is derived, not measured.  The kernel's M and G sums carry at most (ceil(V_draw / (64 W)) + 6 + W - 1) 2^-24 relative (header: each
# thread's columns in index order, a 6-step wave tree, the W wave totals in order; W = 1 up to 1024 columns, 16 beyond): 1.3e-6 at 1024, 1.5e-6 at
# 4100 columns.  r itself carries the hardware exponential's error, about 2e-6 at |argument| <= 20.  1e-4 is more than 25 x their sum.

# per shape, per mode of FILTER_MODES: the first seed from 0 at which all B rows of sample_logits meet the three margins (`margins_ok`; the tests assert
# them before they call the kernel).  Found by `python tests/_sampler_filter_cases.py`; None = no seed in 0..39, the pair is dropped (none is, today).
FILTER_SEEDS = {
    (1, 70, 70, 72): (0, 0, 0, 0, 0, 0, 0, 0),
    (5, 390, 256, 392): (0, 0, 0, 0, 1, 0, 0, 0),
    (7, 390, 64, 448): (0, 0, 0, 0, 0, 0, 0, 0),
    (6, 390, 65, 392): (0, 0, 0, 0, 0, 0, 0, 0),
    (4, 300, 1, 304): (0, 0, 0, 0, 0, 0, 0, 0),
    (9, 392, 390, 392): (0, 0, 0, 0, 0, 0, 0, 0),
    (3, 1, 1, 8): (0, 0, 0, 0, 0, 0, 0, 0),
    (2, 64, 64, 64): (0, 0, 0, 0, 0, 0, 0, 0),
    (3, 4100, 4100, 4104): (4, 0, 0, 0, 0, 0, 0, 0),
    (2, 1024, 1024, 1024): (0, 0, 0, 0, 0, 0, 0, 0),
    (2, 1025, 1000, 1032): (0, 0, 0, 0, 0, 0, 0, 0),
}


def _kth_largest(lc, top_k):
    return lc.sort(-1, descending=True).values[:, top_k - 1:top_k]


def filter_reference(logits, V, V_draw, T, top_k, top_p, min_p):
    """(keep, q) over the columns [0, V_draw), by the definition in include/tfx.h: r_c = exp((l_c - l_max) / T) with l_max over ALL V columns;
    top-k: l_c >= the k-th largest candidate logit (0 = off, >= V_draw keeps all); top-p over the top-k survivors S: G(r_c) < top_p M with M = sum
    of r over S and G(x) = sum of r over S above x (>= 1 = off); min-p: r_c >= min_p.  keep = the intersection; q = the survivors' r (unnormalised:
    the rows sum to the surviving mass), 0 elsewhere."""
    l = logits[:, :V].to(F64)
    r = ((l - l.amax(-1, keepdim=True)) / T).exp()[:, :V_draw]
    lc = l[:, :V_draw]
    S = torch.ones_like(lc, dtype=torch.bool)
    if 0 < top_k < V_draw:
        S = lc >= _kth_largest(lc, top_k)
    keep = S & (r >= min_p)
    if top_p < 1.:
        keep &= _mass_above(r, S) < top_p * torch.where(S, r, torch.zeros_like(r)).sum(-1, keepdim=True)
    return keep, torch.where(keep, r, torch.zeros_like(r))


def _mass_above(r, S):
    """G(r_c) for every column: the sum of r over the members of S that are strictly above r_c (ascending sort, suffix sums, the first index past the
    values equal to r_c)"""
    v = torch.where(S, r, torch.zeros_like(r)).sort(-1).values
    suf = torch.cat([v.flip(-1).cumsum(-1).flip(-1), torch.zeros_like(v[:, :1])], -1)
    return suf.gather(1, torch.searchsorted(v, r.contiguous(), right=True))


def nucleus_margin(logits, V, V_draw, T, top_k, top_p):
    """min over the top-k survivors of |G(r_c) - top_p M| / M: no column's membership in the nucleus may hang on a rounding of the two sums"""
    if top_p >= 1.:
        return math.inf
    l = logits[:, :V].to(F64)
    r = ((l - l.amax(-1, keepdim=True)) / T).exp()[:, :V_draw]
    lc = l[:, :V_draw]
    S = lc >= _kth_largest(lc, top_k) if 0 < top_k < V_draw else torch.ones_like(lc, dtype=torch.bool)
    M = torch.where(S, r, torch.zeros_like(r)).sum(-1, keepdim=True)
    d = (_mass_above(r, S) - top_p * M).abs() / M
    return float(d[S].min())


def top_k_margin(logits, V_draw, top_k):
    """smallest relative distance from the k-th largest candidate logit of any candidate that is not exactly tied with it"""
    if not 0 < top_k < V_draw:
        return math.inf
    lc = logits[:, :V_draw].to(F64)
    kth = _kth_largest(lc, top_k)
    d = ((lc - kth).abs() / kth.abs().clamp(min=1e-30))[lc != kth]
    return float(d.min()) if d.numel() else math.inf


def margins_ok(lg, V, Vd, T, mp, k, p):
    return (nucleus_margin(lg, V, Vd, T, k, p) >= NUCLEUS_MARGIN and min_p_margin(lg, V, T, mp) >= MIN_P_MARGIN
            and top_k_margin(lg, Vd, k) >= TOP_K_MARGIN)


def aim_targets(keep, q, min_cell=1e-3):
    """per row every target of draw_targets, then the heaviest survivor if its cell holds `min_cell` of the surviving mass and it is not among them:
    with hundreds of survivors (top_k past the row's width) the first, the last and the columns near 63 / 64 may all be lighter than that"""
    out = draw_targets(keep, q, min_cell)
    for r, t in enumerate(out):
        if keep[r].any():
            h = int(q[r].argmax())
            if h not in t and float(q[r, h]) >= min_cell * float(q[r].sum()):
                t.append(h)
    return out


def cases():
    """every (shape, mode, seed) of the table"""
    return [(s, m, FILTER_SEEDS[s][i]) for s in FILTER_SHAPES for i, m in enumerate(FILTER_MODES) if FILTER_SEEDS[s][i] is not None]


@functools.lru_cache(maxsize=None)
def case(shape, mode, seed):
    """(logits, keep, q) of one table entry - computed once, shared by the tests, never written to"""
    B, V, Vd, ld = shape
    T, mp, k, p = mode
    lg = sample_logits(B, V, Vd, ld, seed)
    keep, q = filter_reference(lg, V, Vd, T, k, p, mp)
    return lg, keep, q


# hand-made tie rows: (logits, temperature, top_k, top_p, the columns kept).  Ties at the k-th place all survive; ties at the nucleus boundary are
# all kept: r = 1, .5, .5, .25, .25, M = 2.5, top_p M = 1.5 - G = 0, 1, 1 for columns 0-2 (kept), 2 for columns 3-4 (dropped)
TIE_ROWS = [([5., 4., 4., 4., 1., 0., -1., 3.], 1.0, 2, 1.0, [0, 1, 2, 3]),
            ([math.log(4.), math.log(2.), math.log(2.), 0., 0.], 1.0, 0, 0.6, [0, 1, 2])]


if __name__ == '__main__':                                  # the seed search
    for s in FILTER_SHAPES:
        B, V, Vd, ld = s
        found = []
        for T, mp, k, p in FILTER_MODES:
            found.append(next((sd for sd in range(40) if margins_ok(sample_logits(B, V, Vd, ld, sd), V, Vd, T, mp, k, p)), None))
        print(f'    {s}: {tuple(found)},')
