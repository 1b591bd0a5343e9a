"""LoRA kernel cases: float64 restatements, per-element bounds and guard bands (not collected: no test_ prefix; imports no GPU code at module level).

Shared by tests/test_lora_cpu.py (the restatements against torch autograd) and tests/test_lora_kernels_gpu.py (tfx_lora_merge / _down / _grad through the C ABI).
GUARD, the fill patterns, e32 / tol_f32 / tol_bf16 and the guarded / padded buffers are those of tests/_gemm_cases.py.

The restatements (what include/tfx.h promises, in float64 from the exact operand values):
  merge64(W, B, A, s)        W + s B A
  down64(Q, R)               Q R^T                      U = X A^T (R = A),  dU = dY B (R = B^T)
  grad64(P, Q, alpha, r)     alpha P[:, :r]^T Q         dB^T = s U^T dY,    dA = s dU^T X
With W_eff = W + s B A and dW = dY^T X:  dA = s B^T dW = s (dY B)^T X,  dB = s dW A^T = s (dY^T (X A^T)) - test_lora_cpu checks this against autograd.

Bounds, derived, not tuned (u16 = 2^-8, u32 = 2^-24; e32(n, S) = 2 (n + 2) u32 S as in _gemm_cases):
  merge    r fused multiply-adds and the closing s * acc + w in fp32, S = |W| + |s| sum_j |B||A|:                     tol = e32(r, S)
  down     K exact bf16 products summed in fp32, one rounding to bf16:                                                 tol = u16 |y| + 2 e32(K, S)
  grad     M exact products summed in fp32 in any order (MFMA chains per run, the runs in ascending order), the multiplication by alpha and the
           addition to G: M + 2 roundings in all, S = |alpha| sum_m |p||q| + |G_initial|:                              tol = e32(M, S)
  down -> grad (the composed pair, P never seen by the test): P = bf16(P_exact + d), |d| <= e32(K, S_down), so P is off by at most
           dP = u16 |P_exact| + 2 e32(K, S_down) and G by |alpha| sum_m dP |q|, next to the product's own e32(M, S):   tol = |alpha| dP^T |Q| + e32(M, S)
"""
from types import SimpleNamespace

import torch

from _gemm_cases import BF, GUARD, PAD, U16, e32, guarded, padded, tol_bf16, tol_f32   # noqa: F401

GRAD_M = (70, 192, 1000)          # + the smallest M with three row runs (found with tfx_lora_grad_plan in the test)
GRAD_K = (64, 200, 520)
RANKS = (1, 8, 24, 64)
MERGE_N = (8, 130)
MERGE_K = (64, 200)


def r_pad_of(r):
    return 32 if r <= 32 else 64


def merge64(W, B, A, s):
    return W.double() + s * (B.double() @ A.double())


def down64(Q, R):
    return Q.double() @ R.double().T


def grad64(P, Q, alpha, r):
    return alpha * (P.double()[:, :r].T @ Q.double())


def _gen(*key):
    return torch.Generator(device='cpu').manual_seed(9000 + sum((i + 1) * 131 * int(k) for i, k in enumerate(key)))


def build_merge(N, K, r, s, device='cpu', zero_b=False):
    g = _gen(N, K, r, 1)
    W = torch.randn(N, K, generator=g)
    W[0, 0] = -0.0                                            # a negative zero keeps its sign bit when nothing is added
    A = torch.randn(max(r, 1), K, generator=g) * K ** -0.5
    B = torch.zeros(N, max(r, 1)) if zero_b else torch.randn(N, max(r, 1), generator=g)
    Wb, Wv = padded(W.to(device)); Ab, Av = padded(A.to(device)); Bb, Bv = padded(B.to(device))
    obuf, ov = guarded(N, K, torch.float32, device)
    kw = dict(W=Wv, ldw=K + GUARD, B=Bv, ldb=max(r, 1) + GUARD, A=Av, lda=K + GUARD, Weff=ov, ldo=K + GUARD, N=N, K=K, r=r, s=s)
    ref = merge64(Wv, Bv[:, :r], Av[:r], s)
    S = Wv.double().abs() + abs(s) * (Bv[:, :r].double().abs() @ Av[:r].double().abs())
    return SimpleNamespace(kw=kw, buf=obuf, view=ov, before=obuf.clone(), ref=ref, tol=tol_f32(e32(r, S)), W=Wv, keep=[Wb, Ab, Bb])


def build_down(M, K, r, device='cpu'):
    g = _gen(M, K, r, 2)
    rp = r_pad_of(r)
    Q = torch.randn(M, K, generator=g).to(BF)
    R = torch.zeros(rp, K)
    R[:r] = torch.randn(r, K, generator=g) * K ** -0.5
    Qb, Qv = padded(Q.to(device)); Rb, Rv = padded(R.to(BF).to(device))
    pbuf, pv = guarded(M, rp, BF, device)
    kw = dict(Q=Qv, ldq=K + GUARD, R=Rv, ldr=K + GUARD, P=pv, ldp=rp + GUARD, M=M, K=K, r_pad=rp)
    ref = down64(Qv, Rv)
    S = Qv.double().abs() @ Rv.double().abs().T
    return SimpleNamespace(kw=kw, buf=pbuf, view=pv, before=pbuf.clone(), ref=ref, tol=tol_bf16(ref, e32(K, S)), E=e32(K, S), Q=Qv, R=Rv, keep=[Qb, Rb])


def build_grad(M, K, r, alpha=1.0, accumulate=0, device='cpu', mapped=False, P=None):
    """mapped: the transposed, column-mapped store of dB - G is [K_out, r] (g_row_stride 1, g_col_stride r + GUARD), colmap a permutation with drops.
    P: a [M, r_pad] bf16 operand made elsewhere (the composed test) instead of the drawn one."""
    g = _gen(M, K, r, 3 + int(mapped))
    rp = r_pad_of(r)
    if P is None:
        P = (torch.randn(M, rp, generator=g) * 0.5).to(BF).to(device)     # columns r .. r_pad - 1 are NOT zero here: rows j >= r of G must stay unwritten
    Q = (torch.randn(M, K, generator=g) * 0.5).to(BF)
    Pb, Pv = padded(P); Qb, Qv = padded(Q.to(device))
    prod = grad64(Pv, Qv, alpha, r)
    Sp = abs(alpha) * (Pv.double()[:, :r].abs().T @ Qv.double().abs())
    keep = [Pb, Qb]
    if not mapped:
        gbuf, gv = guarded(r, K, torch.float32, device)
        gv.copy_(torch.randn(r, K, generator=g).to(device))
        init = gv.double().clone()
        kw = dict(G=gv, g_row_stride=K + GUARD, g_col_stride=1)
        written = torch.zeros(gbuf.shape, dtype=torch.bool, device=device)
        written[GUARD:GUARD + r, :K] = True
        pick = lambda buf: buf[GUARD:GUARD + r, :K]
        ref, S = prod, Sp
    else:
        Kout = K + 5
        cm = torch.randperm(Kout, generator=g)[:K]
        cm[::7] = -1
        cmd = cm.to(torch.int32).to(device)
        keep.append(cmd)
        gbuf, gv = guarded(Kout, r, torch.float32, device)
        gv.copy_(torch.randn(Kout, r, generator=g).to(device))
        init_full = gv.double().clone()
        kept = (cm >= 0).to(device)
        dst = cm.to(device)[kept]
        kw = dict(G=gv, g_row_stride=1, g_col_stride=r + GUARD, colmap=cmd)
        written = torch.zeros(gbuf.shape, dtype=torch.bool, device=device)
        written[dst + GUARD, :r] = True
        written[:, r:] = False
        pick = lambda buf: buf[GUARD:GUARD + Kout, :r][dst].T            # [r, kept columns]
        init = init_full[dst].T
        ref, S = prod[:, kept], Sp[:, kept]
    if accumulate:
        ref = ref + init; S = S + init.abs()
    kw.update(P=Pv, ldp=rp + GUARD, Q=Qv, ldq=K + GUARD, M=M, K=K, r=r, r_pad=rp, accumulate=accumulate, alpha=alpha)
    return SimpleNamespace(kw=kw, buf=gbuf, before=gbuf.clone(), written=written, pick=pick, ref=ref, S=S, tol=tol_f32(e32(M, S)), P=Pv, Q=Qv, keep=keep)
