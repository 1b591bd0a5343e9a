"""Attention kernels (csrc/attention.hip, decode_attn_rows_k of csrc/decode.hip): the soft-cap contract in float64, per-element bounds for every output of
tfx_attn_fwd / tfx_attn_bwd / tfx_decode_attn, the probe inputs that place scores on purpose, and an fp32 / bf16 CPU emulation with a fault list
(not collected: no test_ prefix; imports no GPU code at module level).

Shared by tests/test_attention_bounds_cpu.py (the emulation of a correct kernel stays under every bound in two summation orders, every listed fault breaks one,
and the report says per fault what the per-row / whole-tensor tolerances of tests/_attn_cases.py and tests/test_kernels_gpu.py do with it on the catalogue's
own inputs) and tests/test_attention_softcap_gpu.py.
U16 = 2^-8, U32 = 2^-24, assert_elementwise, assert_untouched and guarded are those of tests/_gemm_cases.py.

Operands.  The convention of _attn_cases.exact_input_reference(): every kernel is judged from ITS OWN inputs, in float64 - the forward from its bf16 q~, k~, v
and gate logits; the prep kernel from dout and the forward kernel's bf16 `out`; the dK/dV and dQ kernels from q~, k~, v and the prep kernel's bf16 do_eff and
fp32 delta.  The backward kernels read the forward's fp32 lse where the reference has its own: the measured difference |lse_kernel - lse_ref| of the row enters
their bound as a relative error of P (it is an operand error, not theirs), so the backward bounds hold whatever the forward did.

The soft-cap contract (include/tfx.h, tfx_qk_norm_rope_args.sc_plan; attention.hip softcap16).  x = s / cap.
  plan_ref()   B = 1.02 ns^2 q_scale max|1 + gq| max|1 + gk|.  The mode is a comparison of the fp32 B the kernel stores (B / cap <= 0.2: mode 0, <= 0.35:
               mode 1, else 2), so B is formed in fp32 in the header's order - products only, no contraction, correctly rounded division: bit for bit - and
               everything else in float64 from that B.  Mode 0: tanh x ~ a1 x + a3 x^3 with the x^5 Taylor term (2/15) x^5 economised on [-b, b], b = B / cap:
               T5(y) = 16 y^5 - 20 y^3 + 5 y  =>  x^5 ~ (5/4) b^2 x^3 - (5/16) b^4 x, so a1 = 1 - b^4 / 24, a3 = -1/3 + b^2 / 6.  Mode 1: the x^7 term
               -(17/315) x^7 economised with T7: x^7 ~ (7/4) b^2 x^5 - (7/8) b^4 x^3 + (7/64) b^6 x.  Derivative coefficients: a1, 3 a3, 5 a5 exactly.
               Slots: {mode, L a1, L a3 / cap^2, L a5 / cap^4, a1, 3 a3 / cap^2, 5 a5 / cap^4, B}, L = log2 e.  Mode 2 (and no gains: B = +inf) holds the Taylor
               cubic.  A slot is a sum of at most three terms, each a chain of at most 14 fp32 roundings (b^2 carries 3, its cube 11, 1 / cap^2 two, L and
               the rational constants one each): slot_tol = 16 u32 (sum of the magnitudes of the slot's terms).  B and the mode are exact.
  forms()      what a kernel may apply to a score, each with the interval it may be applied on:
                 plan modes 0 / 1     the plan's polynomial, |s| <= B (nothing else; a visible score outside is a contract violation and raises)
                 no plan, 'wave'      Taylor cubic |x| <= 0.12, quintic <= 0.28, degree 9 <= 0.45, the exact exp2 / rcp form anywhere.  Which one a score gets
                                      depends on the largest |score| of its wave, so every form whose interval holds |x| is legal and none above its
                                      threshold: the bound is a function of the score alone
                 no plan, 'row'       (the forward against a KV cache, softcap16<true>) degree 9 <= 0.45 or exact, by the row's own maximum
                 'rows'               (decode_attn_rows_k) exact, with or without a plan
               Thresholds are compared in fp32 on the fp32 score: legal means |s| - e_s <= fl32(fl32(thr) cap), e_s the score's accumulation error below.
  eps_fwd(x)   max over the legal forms of |form(x) - tanh x| + the form's fp32 evaluation: 6 u32 |x| for a polynomial (Horner with folded coefficients, each
               rounded once), 12 u32 for the exact form (th = 1 - 2 r, r = rcp(1 + exp2(2 L x)): r is within 5 u32 + ln2 |arg| u32 relative, r |arg| <= 0.53, one
               more rounding of th).  Evaluated at the element's own x in float64, nothing tabulated.
  eps_bwd(x)   modes 0 / 1: |a1 + 3 a3 x^2 + 5 a5 x^4 - (1 - tanh^2 x)| + 6 u32.  Mode 2: the kernels form 1 - (s2 / cap2)^2 from THEIR capped score: max over the
               legal forms f of |f^2 - tanh^2| + 2 |f| round(f) + 3 u32.

Bounds, derived, not tuned.  acc(n) = 2 (n + 2) u32 for a sum of n products or terms in fp32 in any order (e32 of _gemm_cases.py; a lone product of two bf16
values has 16 significant bits and is exact: acc(n <= 1) = 0).  h16(y) = 2^(floor(log2 |y|) - 8) is the half-ulp of y's bf16 binade, <= u16 |y| and as small as
u16 |y| / 2: a bf16 rounding is charged h16 of the largest value it can have been applied to, a bf16 output y gets tol = E + h16(|y| + E) (so the general shape
tol = u16 |y| + c u16 M + (n + c') u32 M' below is an upper envelope of what is asserted).  M sums magnitudes, so a reference near zero keeps an absolute term
and no element is excluded.
  scores       s_ij from bf16 q~, k~: e_s = acc(nz_ij) sum_d |q_id k_jd|, nz the number of non-zero products.  |tanh''| <= 0.77, so the capped score moves by
               e_s (1 - t^2) + e_s^2 / (2 cap) nats, t = tanh x.
  exp          P~_ij = exp2(s2) against the FIXED reference 0: relative error rho_ij = cap eps_fwd + [score term] + (cap |t| + 3) u32 (s2 rounded once: |s2| ln2 u32
               = cap |t| u32; v_exp_f32 at 1 ulp = 2 u32; one for the product with cap2).
  lse          the row sum of m visible terms, all positive: relative R_i = sum_j p_ij rho_ij + acc(m) (d lse / d s_j = p_j: the score errors enter p-weighted,
               never more than cap eps_fwd of the row's worst key).  lse = log2(sum) ln2 with v_log_f32 at 1 ulp: tol = R_i + 4 u32 |lse| + 4 u32, in nats.
  out          g sum_j bf16(P~_ij) v_jd / sum: E = g [(1 + R') sum_j p_ij (rho_ij + h16(P~ (1 + rho)) / P~) |v_jd| + (acc(m) + R') M_id], M_id = sum_j p_ij |v_jd|,
               R' = R_i + A_SIG + 3 u32 (the reciprocal, the product with g, A_SIG = (|z| + 5) u32 of _tokenwise_cases.py for sigmoid); c = 2: P and the store.
               The rows kernel keeps P in fp32 (no h16 term) and accumulates with fma.  p_ij moves by rho_ij + R_i: the 2 cap eps of the score error.
  do_eff       bf16(dout g): E = |dout g| (A_SIG + 2 u32).      delta = sum_d dout og (fp32, 64 terms): acc(64) sum |dout og|.
  dgate        bf16(delta (1 - g)): E = tol_delta (1 - g) + sum |dout og| (g A_SIG + 2 u32).
  dS           P_ij (dP_ij - delta_i) tanh'_ij.  P = exp2(s2 - lse2) carries pi_ij = rho_ij + |lse_kernel - lse_ref| + (2 |lse| + |cap t - lse| + 2) u32;
               dP = do_eff . v: e_dP = acc(nz) sum |do_eff v|, one rounding of the difference; tanh' carries eta_ij = eps_bwd + 0.77 e_s / cap.
               E_dS = p [(1 + pi) (|D| + e_D) (tanh' + eta) (1 + 3 u32) - |D| tanh'] - the product of the three perturbed factors, nothing dropped - and the
               bf16 packing adds h16(|dS| + E_dS): W_ij = E_dS + h16.
  dq, dk       sum_j bf16(dS_ij) k~_jd (sum_i ... q~_id): E = sum W |k| + acc(n_terms) sum (|dS| + W) |k|; c = 2: dS and the store.
  dv           sum_i bf16(P_ij) do_eff_id: E = sum_i (p pi + h16(p (1 + pi))) |do_eff| + acc(n_terms) sum p |do_eff|.
  LASER        the same bounds with the extra factor.  out = g log(O), O = P v' > 0: every term is positive, M = O, and the relative error relO of O (the `out`
               formula without g) becomes absolute: E = g [relO / (1 - relO) + 4 u32 |log O| + 4 u32] + |out| (A_SIG + 2 u32).  do_eff = bf16(dout g exp(-L)),
               L = og / g from the kernel's own og: E = |do_eff| [A_SIG + (A_SIG + 3 u32) |L| + (1.5 |L| + 3) u32 + 3 u32] (rcp(g), the product, __expf as in
               _tokenwise_cases.py, two products).  delta = g sum_d dout: (acc(64) + A_SIG + u32) g sum |dout|.  dS, dq, dk unchanged with v' for v.  dv: the
               dK/dV kernel STORES d v' in bf16 (E1 = E + h16) and tfx_laser_v_bwd multiplies by F = exp(c th) (1 - th^2), th = tanh(v / c), from the raw v:
               E = E1 F + (|d v'| + E1) F relF, relF = (5 c |th| + 4) u32 + (8 th^2 + 2) u32 / (1 - th^2) + 2 u32 (tanhf, expf at 2 ulp); c = 3 roundings.
  fused QK-norm backward (nr_*): the bound through the norm's nested row sums and the atomically accumulated gain gradients is not derived yet;
               that path stays on ROW_TOL_NR of _attn_cases.py and has no per-element bound here.

Worst error / bound of the fp32 CPU emulation per output, in both summation orders: tests/test_attention_bounds_cpu.py prints them and asserts that every
bf16 output reaches at least 0.1 of its bound.  The bf16 outputs sit at the rounding term; lse reaches its bound where a polynomial branch is applied at the end
of its interval (the Taylor quintic at 0.28: 7.1e-6 x cap); delta is an fp32 sum of 64 signed terms against the worst case of the sum of their magnitudes and
stays far below.  The MI355X figures per test are in profiles/attn_bounds.txt.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from _attn_cases import B_OVER_CAP, CAP, CASES, LASER_C, build_inputs, heads, layout_maps, norm_qk
from _gemm_cases import U16, U32  # noqa: F401

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
BF = torch.bfloat16
F64 = torch.float64
TAYLOR = (1., -1. / 3., 2. / 15., -17. / 315., 62. / 2835.)
THRESH = (0.12, 0.28, 0.45)               # Taylor cubic / quintic / degree 9 (attention.hip make_softcap_legacy)
PLAN_THRESH = (0.2, 0.35)                 # plan mode 0 / 1 (tfx.h)
B_MARGIN = 1.02
TANH_D2_MAX = 0.77                        # max |d^2 tanh / dx^2| = 4 / (3 sqrt 3) = 0.7698
f32 = np.float32


def acc(n):
    """relative error of an fp32 sum of n terms against the sum of their magnitudes"""
    n = torch.as_tensor(n, dtype=F64)
    return torch.where(n <= 1, torch.zeros_like(n), 2 * (n + 2) * U32)


def h16(y):
    """half-ulp of the bf16 binade of |y| (0 at 0)"""
    y = y.abs()
    return torch.where(y > 0, torch.exp2(torch.floor(torch.log2(y.clamp_min(1e-300))) - 8), torch.zeros_like(y))


def fl32_thr(thr, cap):
    """the kernel's fp32 threshold fl(fl(thr) cap)"""
    return float(f32(thr) * f32(cap))


# ---------------------------------------------------------------------------------------------- the plan
def _plan_B32(gq, gk, norm_scale, q_scale, fault=None):
    mq = np.abs(f32(1) + gq.detach().cpu().numpy().astype(f32)).max()
    mk = np.abs(f32(1) + gk.detach().cpu().numpy().astype(f32)).max()
    ns = f32(norm_scale) if norm_scale > 0 else f32(8)
    lead = f32(1) if fault == 'B_without_1.02' else f32(1.02)
    return lead * ns * ns * f32(q_scale) * mq * mk


def _plan_from_B(B, cap, fault=None):
    """(mode, (a1, a3, a5), (d1, d3, d5) in x units, slots, slot_mag) in float64 from the fp32 B"""
    ic2 = 1. / (cap * cap)
    a, mag = [1., -1. / 3., 0.], [1., 1. / 3., 0.]
    mode = 2
    if math.isfinite(B):
        bx32 = f32(B) / f32(cap)
        b2 = (float(B) / cap) ** 2
        sg = -1. if fault == 'a3_economisation_sign' else 1.
        if bx32 <= f32(0.2):
            mode = 0
            a, mag = [1. - b2 * b2 / 24., -1. / 3. + sg * b2 / 6., 0.], [1. + b2 * b2 / 24., 1. / 3. + b2 / 6., 0.]
        elif bx32 <= f32(0.35):
            c7 = 17. / 315.
            mode = 1
            a = [1. - c7 * (7. / 64.) * b2 ** 3, -1. / 3. + sg * c7 * (7. / 8.) * b2 * b2, 2. / 15. - c7 * (7. / 4.) * b2]
            mag = [1. + c7 * (7. / 64.) * b2 ** 3, 1. / 3. + c7 * (7. / 8.) * b2 * b2, 2. / 15. + c7 * (7. / 4.) * b2]
            if fault == 'taylor_in_mode_1':
                a = [1., -1. / 3., 2. / 15.]
    d = [a[0], (1. if fault == 'd3_without_3' else 3.) * a[1], (1. if fault == 'd5_without_5' else 5.) * a[2]]
    slots = [float(mode), LOG2E * a[0], LOG2E * a[1] * ic2, LOG2E * a[2] * ic2 * ic2, d[0], d[1] * ic2, d[2] * ic2 * ic2, float(B)]
    smag = [0., LOG2E * mag[0], LOG2E * mag[1] * ic2, LOG2E * mag[2] * ic2 * ic2, mag[0], 3 * mag[1] * ic2, 5 * mag[2] * ic2 * ic2, 0.]
    return mode, a, d, slots, smag


def _plan(B, cap, fault=None):
    mode, a, d, slots, smag = _plan_from_B(B, cap, fault)
    return SimpleNamespace(mode=mode, B=B, bx=B / cap, a=tuple(a), d=tuple(d), cap=cap, slots=torch.tensor(slots, dtype=F64),
                           slot_tol=16 * U32 * torch.tensor(smag, dtype=F64))


def plan_ref(gq, gk, norm_scale, q_scale, cap, fault=None):
    """the header's rule (module docstring).  gq / gk: fp32 tensors (64,), or None: no RMS normalisation - mode 2 with B = +inf.
    `fault`: the CPU emulation's fault list only."""
    return _plan(float('inf') if gq is None or gk is None else float(_plan_B32(gq, gk, norm_scale, q_scale, fault)), cap, fault)


def plan_at(bx, cap=CAP, fault=None):
    """the plan of a layer whose stored B is fl32(bx cap) (the probes: any B a gain pair can produce)"""
    return _plan(float(f32(bx * cap)), cap, fault)


def gains_for(bx, cap=CAP, dh=64, step=0):
    """gains whose plan has B / cap next to `bx`: the largest g = gq[c] = gk[c] with fl32 B / cap <= bx (step 0), or `step` fp32 steps of g further
    (+1: the first g above).  norm_scale = dh^0.5, q_scale = dh^-0.5.  Returns (gq, gk, norm_scale, q_scale)."""
    ns, qs = dh ** 0.5, dh ** -0.5
    g = f32(math.sqrt(bx * cap / (1.02 * ns * ns * qs)) - 1.)

    def over(gv):
        t = torch.full((64,), float(gv), dtype=torch.float32)
        return f32(_plan_B32(t, t, ns, qs)) / f32(cap) > f32(bx)
    while over(g):
        g = np.nextafter(g, f32(-np.inf))
    while not over(np.nextafter(g, f32(np.inf))):
        g = np.nextafter(g, f32(np.inf))
    for _ in range(abs(step)):
        g = np.nextafter(g, f32(np.inf if step > 0 else -np.inf))
    gen = torch.Generator().manual_seed(int(bx * 1000) + step)
    gq = (1 + float(g)) * (0.5 + 0.45 * torch.rand(64, generator=gen)) - 1              # |1 + gain| stays below the largest one's
    gk = (1 + float(g)) * (0.5 + 0.45 * torch.rand(64, generator=gen)) - 1
    gq[7] = float(g); gk[11] = float(g)
    return gq, gk, ns, qs


# ---------------------------------------------------------------------------------------------- the forms
def _poly(a, x):
    u = x * x
    r = torch.zeros_like(x)
    for c in reversed(a):
        r = r * u + c
    return r * x


def _dpoly(a, x):
    u = x * x
    r = torch.zeros_like(x)
    for i in reversed(range(len(a))):
        r = r * u + (2 * i + 1) * a[i]
    return r


def forms(cap, plan=None, path='wave'):
    """[(name, largest |s| the form may be applied on, polynomial coefficients in x or None = the exact form)]"""
    if path == 'rows':
        return [('exact', float('inf'), None)]
    if plan is not None and plan.mode <= 1:
        return [('plan cubic' if plan.mode == 0 else 'plan quintic', plan.B, plan.a[:2 + plan.mode])]
    ex, t9 = ('exact', float('inf'), None), ('taylor 9', fl32_thr(THRESH[2], cap), TAYLOR)
    if path == 'row':
        return [t9, ex]
    return [('taylor cubic', fl32_thr(THRESH[0], cap), TAYLOR[:2]), ('taylor quintic', fl32_thr(THRESH[1], cap), TAYLOR[:3]), t9, ex]


def _form_eval(a, x):
    """(value, fp32 evaluation error) of one form in tanh units"""
    if a is None:
        return torch.tanh(x), torch.full_like(x, 12 * U32)
    return _poly(a, x), 6 * U32 * x.abs()


def eps_fwd(s, e_s, cap, plan=None, path='wave'):
    """largest |form(x) - tanh x| + evaluation error over the forms legal at each score (tanh units); +inf where no form is legal (outside a plan's B)"""
    x, t = s / cap, torch.tanh(s / cap)
    eps = torch.full_like(s, float('-inf'))
    for _, smax, a in forms(cap, plan, path):
        f, r = _form_eval(a, x)
        eps = torch.where(s.abs() - e_s <= smax, torch.maximum(eps, (f - t).abs() + r), eps)
    return torch.where(torch.isinf(eps), torch.full_like(eps, float('inf')), eps)


def eps_bwd(s, e_s, cap, plan=None):
    """the same for the derivative factor 1 - tanh^2 (the backward kernels: 'wave' forms)"""
    x = s / cap
    t = torch.tanh(x)
    if plan is not None and plan.mode <= 1:
        ok = s.abs() - e_s <= plan.B
        return torch.where(ok, (_dpoly([plan.a[0], plan.a[1], plan.a[2]], x) - (1 - t * t)).abs() + 6 * U32, torch.full_like(s, float('inf')))
    eps = torch.zeros_like(s)
    for _, smax, a in forms(cap, None, 'wave'):
        f, r = _form_eval(a, x)
        eps = torch.where(s.abs() - e_s <= smax, torch.maximum(eps, (f * f - t * t).abs() + 2 * f.abs() * r + r * r + 3 * U32), eps)
    return eps


# ---------------------------------------------------------------------------------------------- references and bounds
def problem(q, k, v, gate, kv_end, dout=None, cap=CAP, plan=None, path='wave', name='', v_raw=None):
    """one launch: q (b, h, n, 64), k / v (b, h, nk, 64), gate logits (b, h, n), dout like q - the bf16 VALUES the kernels read, any float dtype; kv_end (b, n).
    v_raw: LASER - `v` is the bf16 v' = exp(c tanh(v_raw / c)) the attention kernels read, v_raw the values tfx_laser_v_bwd reads"""
    return SimpleNamespace(q=q.to(BF).double(), k=k.to(BF).double(), v=v.to(BF).double(), gate=gate.to(BF).double(), kv_end=kv_end.long(),
                           dout=None if dout is None else dout.to(BF).double(), cap=cap, plan=plan, path=path, name=name,
                           b=q.shape[0], h=q.shape[1], n=q.shape[2], nk=k.shape[2], laser=v_raw is not None,
                           v_raw=None if v_raw is None else v_raw.to(BF).double())


def _a_sig(z):
    return (z.abs() + 5) * U32


def _scores(P, path):
    q, k, cap = P.q, P.k, P.cap
    s = torch.einsum('bhid,bhjd->bhij', q, k)
    S = torch.einsum('bhid,bhjd->bhij', q.abs(), k.abs())
    nz = torch.einsum('bhid,bhjd->bhij', (q != 0).double(), (k != 0).double())
    e_s = acc(nz) * S
    t = torch.tanh(s / cap)
    vis = (torch.arange(P.nk, device=q.device)[None, None, :] < P.kv_end[:, :, None])[:, None]
    eps = eps_fwd(s, e_s, cap, P.plan, path)
    if bool((torch.isinf(eps) & vis).any()):
        raise ValueError(f'{P.name}: a visible score lies outside the plan\'s bound B = {P.plan.B}: the inputs break the contract of sc_plan')
    eps = torch.where(vis, eps, torch.zeros_like(eps))
    score = e_s * (1 - t * t) + 0.5 * e_s * e_s / cap
    rho = cap * eps + score + (cap * t.abs() + 3) * U32
    z = (cap * t).masked_fill(~vis, float('-inf'))
    lse = torch.logsumexp(z, dim=-1)
    p = torch.exp(z - lse[..., None])
    return SimpleNamespace(s=s, e_s=e_s, t=t, vis=vis, rho=rho, z=z, lse=lse, p=p, m=P.kv_end[:, None, :].double().expand_as(lse))


def forward_bounds(P):
    """{'out': (ref, tol), 'lse': (ref, tol)} in float64, (b, h, n, 64) / (b, h, n)"""
    c = _scores(P, P.path)
    R = (c.p * c.rho).sum(-1) + acc(c.m)
    lse_tol = R + 4 * U32 * c.lse.abs() + 4 * U32
    sg = torch.sigmoid(P.gate)
    Rp = R + _a_sig(P.gate) + 3 * U32
    Rp = Rp / (1 - Rp)
    if P.path == 'rows':
        w = c.p * c.rho
    else:                                                             # P~ = exp(z) against the fixed reference 0, packed to bf16
        E = torch.exp(c.z)
        w = c.p * (c.rho + h16(E * (1 + c.rho)) / E.clamp_min(1e-300))
    M = torch.einsum('bhij,bhjd->bhid', c.p, P.v.abs())
    num = torch.einsum('bhij,bhjd->bhid', w, P.v.abs())
    O = torch.einsum('bhij,bhjd->bhid', c.p, P.v)
    if P.laser:                                                       # og = g log(O / sum), O = P v' > 0: M = O, the relative error of O becomes absolute
        Rl = (R + 3 * U32)[..., None]
        relO = ((1 + Rl) * num + (acc(c.m)[..., None] + Rl) * O) / O
        ref = sg[..., None] * torch.log(O)
        Eo = sg[..., None] * (relO / (1 - relO) + 4 * U32 * torch.log(O).abs() + 4 * U32) + ref.abs() * (_a_sig(P.gate) + 2 * U32)[..., None]
        return {'out': (ref, Eo + h16(ref.abs() + Eo)), 'lse': (c.lse, lse_tol)}
    ref = O * sg[..., None]
    Eo = sg[..., None] * ((1 + Rp[..., None]) * num + (acc(c.m) + Rp)[..., None] * M)
    return {'out': (ref, Eo + h16(ref.abs() + Eo)), 'lse': (c.lse, lse_tol)}


def backward_bounds(P, got):
    """{'do_eff', 'delta', 'dgate', 'dq', 'dk', 'dv': (ref, tol)} from the kernels' own out, lse, do_eff and delta in `got` ((b, h, n, ...) tensors)"""
    cap = P.cap
    sg = torch.sigmoid(P.gate)
    a_sig = _a_sig(P.gate)
    og, dout = got['out'].double(), P.dout
    r = {}
    dl_ref, Md = (dout * og).sum(-1), (dout * og).abs().sum(-1)
    dl_tol = acc(64) * Md
    if P.laser:
        L = og / sg[..., None]
        ref = dout * sg[..., None] * torch.exp(-L)
        E = ref.abs() * (a_sig[..., None] + (a_sig[..., None] + 3 * U32) * L.abs() + (1.5 * L.abs() + 3) * U32 + 3 * U32)
        r['do_eff'] = (ref, E + h16(ref.abs() + E))
        r['delta'] = (dout.sum(-1) * sg, (acc(64) + a_sig + U32) * dout.abs().sum(-1) * sg)
    else:
        ref = dout * sg[..., None]
        E = ref.abs() * (a_sig + 2 * U32)[..., None]
        r['do_eff'] = (ref, E + h16(ref.abs() + E))
        r['delta'] = (dl_ref, dl_tol)
    ref = dl_ref * (1 - sg)
    E = dl_tol * (1 - sg) + Md * (sg * a_sig + 2 * U32)
    r['dgate'] = (ref, E + h16(ref.abs() + E))

    c = _scores(P, 'wave')
    de, dl = got['do_eff'].double(), got['delta'].double()
    lse_k = got['lse'].double()
    pi = c.rho + ((lse_k - c.lse).abs() + (2 * c.lse.abs() + 2) * U32)[..., None] + torch.where(c.vis, (c.z - c.lse[..., None]).abs(), torch.zeros_like(c.s)) * U32
    pi = torch.where(c.vis, pi, torch.zeros_like(pi))
    dP = torch.einsum('bhid,bhjd->bhij', de, P.v)
    MdP = torch.einsum('bhid,bhjd->bhij', de.abs(), P.v.abs())
    nzv = torch.einsum('bhid,bhjd->bhij', (de != 0).double(), (P.v != 0).double())
    D = dP - dl[..., None]
    eD = acc(nzv) * MdP + U32 * D.abs()
    dth = 1 - c.t * c.t
    eta = eps_bwd(c.s, c.e_s, cap, P.plan) + TANH_D2_MAX * c.e_s / cap
    eta = torch.where(c.vis, eta, torch.zeros_like(eta))
    dS = c.p * D * dth
    E_dS = c.p * ((1 + pi) * (D.abs() + eD) * (dth + eta) * (1 + 3 * U32) - D.abs() * dth)
    W = E_dS + h16(dS.abs() + E_dS)
    A = dS.abs() + W
    cnt = c.vis.double().sum(-2).expand(P.b, P.h, P.nk)                              # rows that see key j
    for name, eq, other, nterm in (('dq', 'bhij,bhjd->bhid', P.k, c.m), ('dk', 'bhij,bhid->bhjd', P.q, cnt)):
        ref = torch.einsum(eq, dS, other)
        E = torch.einsum(eq, W, other.abs()) + acc(nterm)[..., None] * torch.einsum(eq, A, other.abs())
        r[name] = (ref, E + h16(ref.abs() + E))
    Wp = c.p * pi + h16(c.p * (1 + pi))
    ref = torch.einsum('bhij,bhid->bhjd', c.p, de)
    E = torch.einsum('bhij,bhid->bhjd', Wp, de.abs()) + acc(cnt)[..., None] * torch.einsum('bhij,bhid->bhjd', c.p + Wp, de.abs())
    if P.laser:                                                       # d v' is stored in bf16, then tfx_laser_v_bwd: dv = bf16(d v' F), F = exp(c th) (1 - th^2)
        th = torch.tanh(P.v_raw / LASER_C)
        F = torch.exp(LASER_C * th) * (1 - th * th)
        relF = (5 * LASER_C * th.abs() + 4) * U32 + (8 * th * th + 2) * U32 / (1 - th * th) + 2 * U32
        E1 = E + h16(ref.abs() + E)
        ref, E = ref * F, E1 * F + (ref.abs() + E1) * F * relF
    r['dv'] = (ref, E + h16(ref.abs() + E))
    return r


def ratios(got, bounds):
    """{name: (worst error / bound, number of elements over it, index of the worst)}; a non-finite element counts as inf"""
    out = {}
    for name, (ref, tol) in bounds.items():
        g = got[name].double()
        err = (g - ref).abs()
        ratio = torch.where(torch.isfinite(g), err / tol.clamp_min(1e-300), torch.full_like(err, float('inf')))
        ratio = torch.where(torch.isfinite(g) & (err == 0), torch.zeros_like(ratio), ratio)
        i = int(ratio.argmax())
        out[name] = (float(ratio.flatten()[i]), int((ratio > 1).sum()), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape))))
    return out


# ---------------------------------------------------------------------------------------------- probe inputs
def two_col(target):
    """(q0, q1) bf16 values with q0 + q1 exact in fp32 and as close to `target` as two bf16 columns get (2^-16 relative)"""
    t = torch.as_tensor(target, dtype=F64)
    q0 = t.to(BF).double()
    q1 = (t - q0).to(BF).double()
    return q0, q1


def _step_bf16(x, up):
    """the neighbouring bf16 value of the (bf16-valued) float64 scalar x"""
    if x == 0:
        return (1. if up else -1.) * 2. ** -60
    b = torch.tensor(x, dtype=BF).view(torch.int16).item()
    b += 1 if (x > 0) == up else -1
    return float(torch.tensor(b, dtype=torch.int16).view(BF))


def at_threshold(thr_s, above):
    """the two-column score next to the fp32 threshold thr_s: the largest q0 + q1 <= thr_s, or the smallest above it.  The grid of two bf16 columns has a
    spacing of about 2^-17 relative here (asserted: within 2^-15), i.e. on the order of 100 fp32 ulps - not the fp32 neighbours of the threshold: a kernel
    threshold that is off by less than that moves lse by less than 1e-9 nats and is invisible to any bound of this file"""
    q0, q1 = (float(v) for v in two_col(thr_s))
    while q0 + q1 > thr_s:
        q1 = _step_bf16(q1, False)
    while q0 + _step_bf16(q1, True) <= thr_s:
        q1 = _step_bf16(q1, True)
    if above:
        q1 = _step_bf16(q1, True)
    assert (q0 + q1 > thr_s) == above and abs(q0 + q1 - thr_s) <= 2. ** -15 * thr_s
    return q0 + q1


def wave_scores(lo, hi, cap, n=32, inner=()):
    """|scores| of one 32-row wave: both end points on the two-column grid (lo just above its threshold unless 0, hi at or just below), `inner` extra
    values, the rest spread over [lo, hi]; signs are applied by the caller"""
    v = [at_threshold(hi, False)] * 2 + ([at_threshold(lo, True)] * 2 if lo > 0 else [0., 2. ** -20]) + list(inner)
    v += torch.linspace(lo, hi, n - len(v) + 2, dtype=F64)[1:-1].tolist()
    return v[:n]


def noplan_scores(cap):
    """192 scores in six waves of 32 rows: cubic, quintic and degree-9 intervals with their end points, a wave of small scores that one row pushes to the
    exact form, the saturated range up to 3 cap, and a wave that mixes every range below 0.45 cap"""
    t = [fl32_thr(x, cap) for x in THRESH]
    small = [0.01 * cap, 0.05 * cap, 0.1 * cap]
    w = [wave_scores(0., t[0], cap), wave_scores(t[0], t[1], cap, inner=small), wave_scores(t[1], t[2], cap, inner=small + [0.2 * cap]),
         wave_scores(0., t[1], cap, inner=[at_threshold(t[2], True)]),
         wave_scores(t[2], 3 * cap, cap, inner=[0.5 * cap, 0.7 * cap, cap, 1.5 * cap, 2 * cap, 0.02 * cap, 0.2 * cap, 0.4 * cap]),
         wave_scores(0., t[2], cap)]
    return [x for ww in w for x in ww]


def plan_scores(B, cap):
    """192 scores inside [0, B]: every wave holds the end point B itself, 16 rows of the second and fifth reach >= 0.95 B"""
    w = []
    for i in range(6):
        inner = torch.linspace(0.95 * B, B, 18, dtype=F64)[1:-1].tolist() if i in (1, 4) else []
        w.append(wave_scores(0., B, cap, inner=inner))
    return [x for ww in w for x in ww]


def _signed(scores, flip):
    s = torch.tensor(scores, dtype=F64)
    sign = torch.where(torch.arange(len(scores)) % 2 == 0, 1., -1.).double()
    return s * sign * (-1. if flip else 1.)


PROBE_LAYOUT = (((), ((20, 30), (100, 49)), ((0, 192),)))      # pure causal; blocks across the 32-key boundaries 32 and 128; the whole sample one block


def fwd_probe(plan=None, path='wave', cap=CAP, seed=0, n_kv=0):
    """the forward function probe: within one (sample, head) every key row is the vector (1, 1, 0, ...) (head 1: its negative), q_i = (q0, q1, 0, ...):
    row i has ONE score s_i = q0 + q1, exact in fp32, for all its keys; v is constant along the keys, so out = sigmoid(gate) v and lse = cap tanh(s_i / cap)
    + ln(m_i).  n_kv > 0: the keys are a cache of n_kv rows per sample and kv_end is drawn over [1, n_kv]."""
    g = torch.Generator().manual_seed(100 + seed)
    scores = plan_scores(plan.B, cap) if plan is not None and plan.mode <= 1 else noplan_scores(cap)
    n, b, h = len(scores), len(PROBE_LAYOUT), 2
    q = torch.zeros(b, h, n, 64, dtype=F64)
    for s_ in range(b):
        order = torch.arange(n) if s_ != 1 else torch.arange(n).reshape(6, 32).flip(0).reshape(-1)      # sample 1: the waves in reverse order
        for hh in range(h):
            sc = _signed(scores, flip=(s_ + hh) % 2 == 1)[order]
            q[s_, hh, :, 0], q[s_, hh, :, 1] = two_col(sc)
    assert bool((q.to(BF).double() == q).all())
    nk = n_kv or n
    k = torch.zeros(b, h, nk, 64, dtype=F64)
    k[:, 0, :, :2] = 1.
    k[:, 1, :, :2] = -1.
    v = torch.randn(b, h, 1, 64, generator=g, dtype=F64).expand(b, h, nk, 64).contiguous() * 2
    gate = torch.randn(b, h, n, generator=g, dtype=F64) * 2
    if n_kv:
        kv_end = torch.randint(1, n_kv + 1, (b, n), generator=g)
        kv_end[:, ::7] = n_kv
        kv_end[:, 3::11] = 1
    else:
        kv_end = layout_maps(n, PROBE_LAYOUT)[0]
    return problem(q, k, v, gate, kv_end, cap=cap, plan=plan, path=path, name=f'fwd probe plan={None if plan is None else plan.mode} {path}')


def closed_form_lse(P):
    """cap tanh(s_i / cap) + ln(m_i) of the forward probe"""
    s = (P.q[..., :2] * P.k[:, :, :1, :2]).sum(-1)
    return P.cap * torch.tanh(s / P.cap) + torch.log(P.kv_end[:, None, :].double())


def deriv_probe(plan=None, cap=CAP, seed=0):
    """the derivative probe: even keys (group A) are (1, 1, 0, ...) with v = +w e_5, odd keys (group B) the zero vector with v = -w e_5; dout = do e_5,
    q_i = (q0, q1, 0, ...).  dq_i[0] = tanh'(s_i) 2 g do w P_A P_B up to the roundings of `out` inside delta: every term of the sum over the keys has the
    same sign, the derivative factor scales the element one to one.  Returns (problem, q_start (b, n))."""
    g = torch.Generator().manual_seed(200 + seed)
    scores = plan_scores(plan.B, cap) if plan is not None and plan.mode <= 1 else noplan_scores(cap)
    n, b, h = len(scores), len(PROBE_LAYOUT), 2
    q = torch.zeros(b, h, n, 64, dtype=F64)
    for s_ in range(b):
        order = torch.arange(n) if s_ != 1 else torch.arange(n).reshape(6, 32).flip(0).reshape(-1)
        for hh in range(h):
            sc = _signed(scores, flip=(s_ + hh) % 2 == 1)[order]
            q[s_, hh, :, 0], q[s_, hh, :, 1] = two_col(sc)
    k = torch.zeros(b, h, n, 64, dtype=F64)
    k[:, 0, 0::2, :2] = 1.
    k[:, 1, 0::2, :2] = -1.
    v = torch.zeros(b, h, n, 64, dtype=F64)
    w = torch.tensor([1.5, 2.25, 3.0], dtype=F64)[:b]
    v[:, :, 0::2, 5] = w[:, None, None]
    v[:, :, 1::2, 5] = -w[:, None, None]
    dout = torch.zeros(b, h, n, 64, dtype=F64)
    dout[..., 5] = (torch.randn(b, h, n, generator=g, dtype=F64).abs() + 0.5).to(BF).double()
    gate = torch.randn(b, h, n, generator=g, dtype=F64)
    kv_end, q_start = layout_maps(n, PROBE_LAYOUT)
    P = problem(q, k, v, gate, kv_end, dout=dout, cap=cap, plan=plan, path='wave', name=f'derivative probe plan={None if plan is None else plan.mode}')
    return P, q_start


def catalogue_problem(name, mode, qk=None, inp=None, bx=None, vl=None, laser=False):
    """a case of _attn_cases.CATALOGUE as a problem.  On the CPU (qk None): q~ | k~ = bf16(norm_qk) of the bf16-rounded raw inputs; on the GPU: the
    kernel's own q~ | k~ and the inputs run_kernels() returned.  The plan is plan_ref of the case's gains.  bx (CPU only): every 1 + gain is scaled so that
    B / cap becomes bx instead of the catalogue's B_OVER_CAP[mode] - the same layout and sentinels under a tighter plan of the same mode.  laser: the LASER
    forms; vl (b, h, n, 64) = the v' tfx_laser_v_fwd wrote (CPU: bf16(exp(c tanh(v / c))) in fp32).  Returns (problem, q_start, inputs)."""
    case = CASES[name]
    b, h, n, HD = case.b, case.h, case.n, case.h * 64
    if inp is None:
        inp = build_inputs(case, mode)
        inp['qkvg'] = inp['qkvg'].to(BF).float()
        inp['dout'] = inp['dout'].to(BF).float()
        if bx is not None:
            r = math.sqrt(bx / B_OVER_CAP[mode])
            inp['gq'], inp['gk'] = (1 + inp['gq']) * r - 1, (1 + inp['gk']) * r - 1
    if qk is None:
        qk = norm_qk(inp['qkvg'][:, :2 * HD], h, inp['gq'], inp['gk'], inp['q_scale'], inp['norm_scale']).to(BF)
    dev = qk.device
    X = inp['qkvg'].to(dev)
    plan = None if mode is None else plan_ref(inp['gq'], inp['gk'], inp['norm_scale'], inp['q_scale'], CAP)
    assert plan is None or plan.mode == mode
    v = heads(X[:, 2 * HD:3 * HD], b, n, h)
    if laser and vl is None:
        vl = torch.exp(LASER_C * torch.tanh(v.float() / LASER_C)).to(BF)
    P = problem(heads(qk.float(), b, n, h), heads(qk[:, HD:].float(), b, n, h), vl if laser else v,
                X[:, 3 * HD:3 * HD + h].reshape(b, n, h).transpose(1, 2), inp['kv_end'].to(dev), dout=heads(inp['dout'].to(dev), b, n, h),
                plan=plan, name=f'{name} mode={mode}' + (f' B/cap={bx}' if bx else '') + (' laser' if laser else ''), v_raw=v if laser else None)
    return P, inp['q_start'], inp


# ---------------------------------------------------------------------------------------------- fp32 / bf16 emulation of the kernels' arithmetic
FAULTS = ('d3_without_3', 'd5_without_5', 'a3_economisation_sign', 'taylor_in_mode_1', 'mode2_derivative_without_log2e', 'thresholds_one_branch_up',
          'B_without_1.02')
ORDERS = ('blocked', 'units')
F32 = torch.float32


def _bf(x):
    return x.to(BF).float()


def _mm(a, bt, order, step):
    """a (.., i, c) x bt (.., j, c)^T in fp32: one blocked product, or the sum of the products of `step` columns at a time (the MFMA's k-steps / the 32-key units)"""
    if order == 'blocked':
        return a @ bt.transpose(-1, -2)
    r = None
    for c0 in range(0, a.shape[-1], step):
        t = a[..., c0:c0 + step] @ bt[..., c0:c0 + step].transpose(-1, -2)
        r = t if r is None else r + t
    return r


def _block_max(a, rows, cols):
    """max of |a| over aligned (rows x cols) blocks of the last two dims, broadcast back"""
    b, h, n, m = a.shape
    pn, pm = -n % rows, -m % cols
    x = torch.nn.functional.pad(a.abs(), (0, pm, 0, pn), value=0.)
    x = x.reshape(b, h, (n + pn) // rows, rows, (m + pm) // cols, cols).amax(dim=(3, 5), keepdim=True)
    return x.expand(b, h, (n + pn) // rows, rows, (m + pm) // cols, cols).reshape(b, h, n + pn, m + pm)[:, :, :n, :m]


def _softcap_f32(s, cap, slots, path, fault, transposed=False):
    """s2 = cap log2e tanh(s / cap) as softcap16 forms it in fp32 (slots: the fp32 plan or None).  The data-dependent form follows the largest |score| of
    the wave's 32 x 32 unit ('row': of the row's 32 keys of the unit)"""
    if slots is not None and slots[0] <= 1:
        u = s * s
        return s * (u * (u * slots[3] + slots[2]) + slots[1]) if slots[0] == 1 else s * (u * slots[2] + slots[1])
    c = torch.tensor(cap, dtype=F32)
    ic = 1 / c
    i2 = ic * ic
    L = torch.tensor(LOG2E, dtype=F32)
    kk = [L, -L * i2 * 0.33333334, L * i2 * i2 * 0.13333334, -L * i2 * i2 * i2 * 0.053968254, L * i2 * i2 * i2 * i2 * 0.021869488]
    thr = [float(f32(t) * f32(cap)) for t in THRESH]
    if fault == 'thresholds_one_branch_up':
        thr = [thr[1], thr[2], thr[2]]
    exact = (c * L) * (1 - 2 / (1 + torch.exp2(s * ic * (2 * L))))
    u = s * s
    p9 = s * (u * (u * (u * (u * kk[4] + kk[3]) + kk[2]) + kk[1]) + kk[0])
    if path == 'rows':
        return exact
    if path == 'row':
        return torch.where(_block_max(s, 1, 32) > thr[2], exact, p9)
    amax = _block_max(s, 32, 32)
    p3 = s * (u * kk[1] + kk[0])
    p5 = s * (u * (u * kk[2] + kk[1]) + kk[0])
    return torch.where(amax > thr[2], exact, torch.where(amax > thr[1], p9, torch.where(amax > thr[0], p5, p3)))


def emulate_plan(gq, gk, norm_scale, q_scale, cap, fault=None):
    """the eight fp32 slots softcap_plan_write stores (float64 values rounded to fp32: the kernel's few roundings are inside slot_tol)"""
    return plan_ref(gq, gk, norm_scale, q_scale, cap, fault).slots.float()


def emulate(P, order='blocked', fault=None, slots=None):
    """the kernels' arithmetic contract in fp32 / bf16 on the CPU: scores by fp32 accumulation, the soft-cap form softcap16 would pick, the fixed-reference
    softmax in the log2 domain, P and dS packed to bf16, fp32 accumulation, bf16 stores.  `slots`: the fp32 plan (default: P.plan's slots, with `fault`).
    Returns the outputs as (b, h, n, ...) fp32 tensors."""
    cap = P.cap
    if slots is None and P.plan is not None:
        pf = _plan_from_B(P.plan.B, cap, fault)
        slots = torch.tensor(pf[3], dtype=F64).float()
    if slots is not None and slots[0] > 1:
        slots = None
    fwd_slots = None if P.path == 'rows' else slots             # the rows kernel ignores the plan
    q, k, v, gate = P.q.float(), P.k.float(), P.v.float(), P.gate.float()
    vis = (torch.arange(P.nk)[None, None, :] < P.kv_end[:, :, None])[:, None]
    L = torch.tensor(LOG2E, dtype=F32)
    s = _mm(q, k, order, 16)
    s2 = _softcap_f32(s, cap, fwd_slots, P.path, fault)
    e = torch.where(vis, torch.exp2(s2), torch.zeros_like(s2))
    if order == 'blocked':
        ls = e.sum(-1)
    else:
        ls = torch.zeros_like(e[..., 0])
        for c0 in range(0, P.nk, 32):
            ls = ls + e[..., c0:c0 + 32].sum(-1)
    pb = e if P.path == 'rows' else _bf(e)
    o = _mm(pb, v.transpose(-1, -2), order, 32)
    g = 1 / (1 + torch.exp(-gate))
    got = {'out': _bf(g[..., None] * torch.log(o * (1 / ls)[..., None])) if P.laser else _bf(o * (g / ls)[..., None]), 'lse': torch.log2(ls) * LN2}
    if P.dout is None:
        return got
    dout = P.dout.float()

    def row_sum(x):
        return x.sum(-1) if order == 'blocked' else x.reshape(*x.shape[:-1], 8, 8).sum(-1).sum(-1)
    dg = row_sum(dout * got['out'])
    if P.laser:
        de, dl = _bf(dout * g[..., None] * torch.exp(-got['out'] * (1 / g)[..., None])), row_sum(dout) * g
    else:
        de, dl = _bf(dout * g[..., None]), dg
    got.update(do_eff=de, delta=dl, dgate=_bf(dg * (1 - g)))
    lse2 = got['lse'] * L
    cap2 = torch.tensor(cap, dtype=F32) * L
    if slots is not None:
        u = s * s
        dth = u * (u * slots[6] + slots[5]) + slots[4] if slots[0] == 1 else u * slots[5] + slots[4]
        arg = s * (u * (u * slots[3] + slots[2]) + slots[1]) - lse2[..., None] if slots[0] == 1 else s * (u * slots[2] + slots[1]) - lse2[..., None]
    else:
        s2b = _softcap_f32(s, cap, None, 'wave', fault)
        g2 = 1 / (cap * cap) if fault == 'mode2_derivative_without_log2e' else 1 / (cap2 * cap2)
        dth = 1 - s2b * s2b * g2
        arg = s2b - lse2[..., None]
    p = torch.where(vis, torch.exp2(arg), torch.zeros_like(arg))
    dP = _mm(de, v, order, 16)
    dS = _bf(p * ((dP - dl[..., None]) * dth))
    got['dq'] = _bf(_mm(dS, k.transpose(-1, -2), order, 32))
    got['dk'] = _bf(_mm(dS.transpose(-1, -2), q.transpose(-1, -2), order, 32))
    got['dv'] = _bf(_mm(_bf(p).transpose(-1, -2), de.transpose(-1, -2), order, 32))
    if P.laser:
        th = torch.tanh(P.v_raw.float() / LASER_C)
        got['dv'] = _bf(got['dv'] * torch.exp(LASER_C * th) * (1 - th * th))
    return got
