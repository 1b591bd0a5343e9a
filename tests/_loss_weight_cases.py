"""Cases of the per-token loss weights (Transfusion.forward(loss_weights=...), include/tfx.h tfx_ce_w_args / tfx_ce_w_chunk_args / tfx_mse_w_args): the float64
restatements, the weight patterns, the bounds and the hand-written weight layouts (not collected: no test_ prefix; imports no GPU code at module level).  Shared
by tests/test_loss_weights_cpu.py, tests/test_loss_weights_kernels_gpu.py and tests/test_loss_weights_gpu.py.

Semantics.  A row with label < 0 or weight 0 is ignored; any other row adds w times what tfx_ce_reg_* adds - acc[0] += w r, acc[1] += w, aux[0] += w (lse - l_y),
aux[1] += w lse^2 - and its gradient is (d r / d l_c) s with s = grad_scale w [scale_dev].  The squared error: acc[0] += sum_r w_r sum_c err^2,
d pred = grad_scale w_r err (clean factor).

Bounds (u = 2^-24; everything else is tests/_text_loss_terms_cases.py's derivation, per row):
  d logits   the `_reg` bound is linear in |s| (E_d = |s| (...) + 2^-126, tol_bf16 = 2^-8 |y| + 2 E_d), so the bound at scale s w is w times the bound at scale s;
             the one operation more, the product grad_scale w, is one rounding of s: u |y| on top.
  acc[0]     sum of n terms w_t r_t onto the initial value, any order: (n + 1 + 8) u (|init| + sum w_t M_t) + sum w_t e_r,t + u sum w_t |r_t|   (the error of
             every r_t scaled by its weight, one rounding for the product w r, the rounding chain of the sum over magnitudes M_t >= |r_t|)
  acc[1]     sum of the n weights: (n + 1 + 8) u (|init| + sum w); exact - the count - when every weight is 0 or 1 (integers below 2^24)
  aux[0/1]   the same with (ce, e_ce, |lse| + |l_y|) and (sq, e_sq, sq)
  mse        tests/test_decode_loss_kernels_gpu.py::test_mse_modes' figures on the weighted reference: acc grows by the float64 sum to 1e-5 relative, d pred
             within 2^-8 |ref| + 2^-22 (|g| + |old|)
Nothing here was fitted to what a kernel returns."""
import math

import torch

import _text_loss_terms_cases as R
from _gemm_cases import U32

SETTINGS = ((0.0, 0.0),) + R.SETTINGS
PATTERNS = ('ones', 'binary', 'uniform', 'zeros')


def weights(T, pattern, seed=0):
    """[T] fp32 weights: all ones | 0 / 1 at random | uniform on [0, 2] with about a quarter exact zeros | all zero"""
    g = torch.Generator().manual_seed(1000 + seed)
    if pattern == 'ones':
        return torch.ones(T)
    if pattern == 'zeros':
        return torch.zeros(T)
    if pattern == 'binary':
        return (torch.rand(T, generator=g) < 0.6).float()
    w = 2. * torch.rand(T, generator=g)
    w[torch.rand(T, generator=g) < 0.25] = 0.
    return w


def ce_w_ref(logits, labels, w, V, z=0., e=0., scale=1.0):
    """float64 restatement: reg_ref of the rows that count (label >= 0 and w != 0; the others as if their label were -1) with, per row, the weight applied:
    fields of reg_ref plus `w` [T] (0 on ignored rows), the sums loss = sum w r, wsum = sum w, ce_sum = sum w ce, sq_sum = sum w lse^2, and d = w d_reg"""
    w = w.to(logits.device, torch.float64)
    lab = torch.where(w == 0, torch.full_like(labels, -1), labels)
    r = R.reg_ref(logits, lab, V, z, e, scale)
    r.w = torch.where(r.valid, w, torch.zeros_like(w))
    r.d_reg, r.d = r.d, r.d * r.w[:, None]
    r.loss, r.wsum, r.ce_sum, r.sq_sum = (r.w * r.row).sum(), r.w.sum(), (r.w * r.ce).sum(), (r.w * r.sq).sum()
    return r


def ce_w_bounds(r, scale=1.0, acc0=R.ACC_INIT, aux0=R.AUX_INIT):
    """(tol_lse [T], tol acc[0], tol acc[1], tol aux[0], tol aux[1], tol d logits [T, V]) for the reference `r` of ce_w_ref, by the docstring"""
    u, z, e, V = U32, r.z, r.e, r.V
    r.d, keep = r.d_reg, r.d
    tol_lse, _, _, _, tol_d = R.reg_bounds(r, scale)
    r.d = keep
    tol_d = tol_d * r.w[:, None] + u * r.d.abs()
    lse, w = r.lse_all, r.w
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
    M = (1 - e) * (lse.abs() + r.picked.abs()) + e * (lse.abs() + r.mu.abs()) + z * r.sq
    n = int((w != 0).sum())
    chain = (n + 1 + 8) * u

    def total(init, mag, err, val):
        return chain * (abs(init) + (w * mag).sum()) + (w * err).sum() + u * (w * val.abs()).sum()
    return (tol_lse, total(acc0[0], M, e_r, r.row), chain * (abs(acc0[1]) + w.sum()), total(aux0[0], lse.abs() + r.picked.abs(), e_ce, r.ce),
            total(aux0[1], r.sq, e_sq, r.sq), tol_d)


def mse_w_ref(pred, flow, w, grad_scale, t_row=None, clean_eps=None, old=None):
    """(sum_r w_r sum_c (pred - flow)^2, d pred) in float64: d pred = grad_scale w_r (pred - flow) [/ max(1 - t, clean_eps)] [+ old]"""
    F = torch.float64
    err = pred.to(F) - flow.to(F)
    wc = w.to(F)[:, None]
    g = grad_scale * wc * err
    if clean_eps is not None:
        g = g / (1 - t_row.to(F)[:, None]).clamp(min=clean_eps)
    return (wc * err ** 2).sum(), g if old is None else old.to(F) + g


# ---------------------------------------------------------------------------------------------- the weight layout
# Every sample is written with its parts as (kind, length) and the expected weights of its row written out BY HAND, token by token:
#   s = [sos], e = [eos], text tokens as their weight, a modality instance of axial shape (2, 3) as  M , , , S  followed by six latent slots and E
#   ([meta] '2' ',' '3' [som] ... [eom]: the shape string "2,3" is three characters), (4,) as  M , S  four slots E.
# `T(n)` is a text part of n tokens, `M0(2, 3)` / `M1(4)` instances of type 0 (dim_latent 3) / type 1 (dim_latent 5).
def layout_samples():
    """name -> (parts, weights, expected row) with parts as ('t', n) | ('m', type, axial), weights as forward() takes them with 1-D weights given as lists"""
    a, b, c = 0.5, 2.0, 0.25
    return {
        # [sos] t t t [eos]: per-token weights; [eos] takes the tensor's last element
        'text_only': ([('t', 3)], [[0.0, a, b]], [0, 0.0, a, b, b]),
        # [sos] M '2' ',' '3' S x6 E t t [eos]: "image -> caption" - the instance and its inserted tokens off, the caption on
        'modality_first': ([('m', 0, (2, 3)), ('t', 2)], [0.0, 1.0], [0] + [0.0] * 5 + [0.0] * 6 + [0.0] + [1.0, 1.0] + [1.0]),
        # [sos] t t M '4' S x4 E [eos]: "prompt -> image" - [eos] takes the instance's scalar weight
        'modality_last': ([('t', 2), ('m', 1, (4,))], [0.0, b], [0] + [0.0, 0.0] + [b] * 3 + [b] * 4 + [b] + [b]),
        # two types and a text between them; None = 1
        'two_types': ([('m', 0, (2, 3)), ('t', 2), ('m', 1, (4,))], [a, [c, 0.0], None],
                      [0] + [a] * 5 + [a] * 6 + [a] + [c, 0.0] + [1.0] * 3 + [1.0] * 4 + [1.0] + [1.0]),
        # two adjacent instances, then text with a scalar weight
        'adjacent': ([('m', 1, (4,)), ('m', 0, (2, 3)), ('t', 1)], [b, 0.0, c], [0] + [b] * 3 + [b] * 4 + [b] + [0.0] * 5 + [0.0] * 6 + [0.0] + [c] + [c]),
        # no weights for the sample: ones everywhere but [sos]
        'none': ([('t', 2), ('m', 1, (4,))], None, [0] + [1.0] * 2 + [1.0] * 8 + [1.0]),
    }


DIM_LATENTS = (3, 5)
PACK_KW = dict(num_modalities=2, dim_latents=DIM_LATENTS, sos_id=300, eos_id=301, meta_id=302, som_ids=[500, 501], eom_ids=[502, 503])


def layout_batch(names, seed=0):
    """(modalities, loss_weights, expected (b, n_full) grid, expected instance weights in scan order) of the named samples as one batch"""
    S = layout_samples()
    g = torch.Generator().manual_seed(seed)
    mods, lw, rows, w_inst = [], [], [], []
    for nm in names:
        parts, ws, row = S[nm]
        mods.append([torch.randint(0, 256, (p[1],), generator=g) if p[0] == 't' else (p[1], torch.randn(*p[2], DIM_LATENTS[p[1]], generator=g)) for p in parts])
        lw.append(None if ws is None else [torch.tensor(w) if isinstance(w, list) else w for w in ws])
        for k, p in enumerate(parts):
            if p[0] == 'm':
                w_inst.append(1.0 if ws is None or ws[k] is None else float(ws[k]))
        rows.append(row)
    n = max(len(r) for r in rows)
    grid = torch.tensor([r + [0.0] * (n - len(r)) for r in rows], dtype=torch.float32)
    return mods, lw, grid, torch.tensor(w_inst, dtype=torch.float32)
