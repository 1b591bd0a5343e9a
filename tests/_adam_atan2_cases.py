"""Shared by tests/test_adam_atan2_cpu.py and tests/test_adam_atan2_gpu.py: the Adam-atan2 rule of `tfx_adam_atan2_step` (include/tfx.h) in fp64, a
per-element error bound for an fp32 evaluation of it derived from the operation count, an fp32 emulation of the kernel's arithmetic on the CPU, and a
list of injected faults the bound must catch.

The rule per element (fp32 in the kernel, every rounding spelled out there under `fp contract(off)`):
    g = g coef;  w = p keep;  g = fma(l2, w, g) if l2 != 0;  m = fma(b1, m, (1 - b1) g);  v = fma(b2, v, g ((1 - b2) g))
    y = m (1 / bc1);  x = sqrt(v) (b / sqrt(bc2));  theta = atan2f(y, x);  p = w - (lr a) theta
keep = 1 - lr wd for a decoupled group (else 1), l2 = wd for the L2 form (else 0); 1 / bc1, b / sqrt(bc2), lr a and keep are rounded ONCE to fp32 on the
host side of the launch.  `ref64` evaluates the same expressions in fp64 from the same fp32 inputs and the same fp32 hyperparameters, with `coef`
given (the clip's own rounding is not what is judged).

THE BOUND, u = 2^-24 (one fp32 rounding is at most u times the magnitude of the result; a result is at most the sum of the magnitudes of its terms).
The multiples are the COUNTED roundings, first order in u, nothing added:
    g coef          1 rounding                                              dg = u |g coef|
    w = p keep      keep rounded on the host (1), the product (1); none where keep = 1      dw = 2 u |w|
    fma(l2, w, g)   1 rounding of the sum, inherited dg and l2 dw           dg = dg + l2 dw + u (|l2 w| + |g coef|)
    m               omb1 = fl(1 - b1) (1), omb1 g (1), the fma (1 on each term): 3 on |(1 - b1) g|, 1 on |b1 m|, plus (1 - b1) dg
    v               omb2 (1), omb2 g (1), g (...) (1), the fma (1 on each term): 4 on |(1 - b2) g^2|, 1 on |b2 v|, plus 2 (1 - b2) |g| dg
    y               1 / bc1 rounded on the host (1), the product (1)        dy = dm / bc1 + 2 u |y|
    x               sqrtf is correctly rounded (1, and it halves v's relative error), b / sqrt(bc2) on the host (1), the product (1)
                                                                            dx = dv b / (2 sqrt(v bc2)) + 3 u x
    theta           d atan2 = (x dy - y dx) / (x^2 + y^2): the absolute form (m can cancel), plus the device atan2f's own error L u |theta|
    p               dw, lr a rounded on the host (1), (lr a) theta (1), the subtraction (1 on |p_new|)
                                                                            dp = dw + lr a dtheta + 2 u |lr a theta| + u |p_new|
What first order leaves out is relative to the bound itself: products of two roundings (u^2) and the linearisation of sqrt and atan2 at the reference
point, which is off by the relative size of the perturbation - at most the ~16 counted roundings, 16 u < 2^-20.  The whole bound is multiplied by
SECOND_ORDER = 1 + 2^-16 for that (and for its own fp64 evaluation); no multiple is raised.

`form='torch'` is the same count for the operations of optim.AdamAtan2, which has no fma: `g + wd w` rounds the product too (2 on |l2 w|), `m.mul_(b1)`
and `v.mul_(b2)` round before the sum (2 on |b1 m| and on |b2 v|), `add_(g, alpha=1 - b1)` and `addcmul_(g, g, value=1 - b2)` round as the kernel's terms
do (3 and 4); everything behind m and v is the kernel's sequence.

L = ATAN2_ULPS = 6.  The kernel calls the ROCm device library's atan2f (`__ocml_atan2_f32`: clang's `__clang_hip_math.h` maps atan2f to it, the code is
`amdgcn/bitcode/ocml.bc`).  A ROCm installation ships that library as bitcode with no accuracy table next to it; the figure is the one OCML is written
to, the OpenCL C specification's table of relative errors for the full profile ("Relative Error as ULPs": atan2 <= 6 ulp).  It is taken from there,
not from what the kernel returns.

Supported magnitudes (tfx.h): g coef and its square are normal fp32 numbers.  The cases here stay inside."""
import math

import numpy as np

U = 2.0 ** -24
ATAN2_ULPS = 6
SECOND_ORDER = 1. + 2.0 ** -16
BLOCK = 1024            # elements per block of the launch: the group is decided per block, per thread only where a block straddles a boundary

F = np.float32
D = np.float64


def f32(x):
    return D(F(x))


def host_consts(grp, step, a, b):
    """what the host side of the launch hands the kernel for one group, as fp32 values: the C code's expressions in double, rounded once"""
    lr, (b1, b2), wd = f32(grp['lr']), (f32(grp['betas'][0]), f32(grp['betas'][1])), f32(grp.get('weight_decay', 0.))
    dec = bool(grp.get('decoupled_weight_decay', False))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(lr_a=F(lr * f32(a)), inv_bc1=F(1.0 / bc1), b_isq=F(f32(b) / math.sqrt(bc2)), beta1=F(b1), beta2=F(b2),
                l2=F(0. if dec else wd), keep=F(1.0 - lr * wd) if dec else F(1.))


def exact_consts(grp, step, a, b):
    """the same quantities in fp64 from the fp32 hyperparameters (nothing rounded to fp32)"""
    lr, (b1, b2), wd = f32(grp['lr']), (f32(grp['betas'][0]), f32(grp['betas'][1])), f32(grp.get('weight_decay', 0.))
    dec = bool(grp.get('decoupled_weight_decay', False))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(lr_a=lr * f32(a), bc1=bc1, bc2=bc2, b=f32(b), beta1=b1, beta2=b2, l2=0. if dec else wd, keep=1.0 - lr * wd if dec else 1.0)


def per_element(groups, gidx, n, fn):
    """{name: fp array over the n elements} of the group constants `fn(group)` gathered by the elements' group index"""
    gidx = np.zeros(n, dtype=np.int64) if gidx is None else np.asarray(gidx, dtype=np.int64)
    recs = [fn(g) for g in groups]
    return {k: np.array([r[k] for r in recs])[gidx] for k in recs[0]}


def coef_f32(sumsq, max_norm, grad_scale=1.):
    """the kernel's clip coefficient: grad_scale min(1, max_norm / fma(sqrt(sumsq), grad_scale, 1e-6)), in fp32"""
    gs = F(grad_scale)
    if not max_norm > 0.:
        return gs
    den = F(D(np.sqrt(F(sumsq))) * D(gs) + D(F(1e-6)))
    return F(gs * min(F(1.), F(F(max_norm) / den)))


def skip_mask(skip, n):
    m = np.zeros(n, dtype=bool)
    for s, e in (skip or ()):
        m[s:e] = True
    return m


def _ref_and_bound(p, g, m, v, step, groups, gidx=None, coef=1., a=1.27, b=1., skip=None, form='kernel'):
    assert form in ('kernel', 'torch')
    k_l2, k_old = (1, 1) if form == 'kernel' else (2, 2)           # roundings on |l2 w| and on |b1 m|, |b2 v| (the docstring counts them)
    p, g, m, v = (np.asarray(t, dtype=F).astype(D) for t in (p, g, m, v))
    n = p.size
    c = per_element(groups, gidx, n, lambda grp: exact_consts(grp, step, a, b))
    coef = f32(coef)
    gc = g * coef
    dg = U * np.abs(gc)
    w = p * c['keep']
    dw = np.where(c['keep'] != 1., 2 * U * np.abs(w), 0.)
    gl = gc + c['l2'] * w
    dg = np.where(c['l2'] != 0., dg + c['l2'] * dw + U * (k_l2 * np.abs(c['l2'] * w) + np.abs(gc)), dg)
    b1, b2 = c['beta1'], c['beta2']
    mn = b1 * m + (1 - b1) * gl
    dm = (1 - b1) * dg + U * (k_old * np.abs(b1 * m) + 3 * np.abs((1 - b1) * gl))
    vn = b2 * v + (1 - b2) * gl * gl
    dv = 2 * (1 - b2) * np.abs(gl) * dg + U * (k_old * np.abs(b2 * v) + 4 * (1 - b2) * gl * gl)
    y = mn / c['bc1']
    x = c['b'] * np.sqrt(vn / c['bc2'])
    dy = dm / c['bc1'] + 2 * U * np.abs(y)
    with np.errstate(divide='ignore', invalid='ignore'):
        dx = np.where(vn > 0, dv * c['b'] / (2 * np.sqrt(vn * c['bc2'])), 0.) + 3 * U * x
        theta = np.arctan2(y, x)
        r2 = x * x + y * y
        dth = np.where(r2 > 0, (np.abs(x) * dy + np.abs(y) * dx) / r2, 0.) + ATAN2_ULPS * U * np.abs(theta)
    pn = w - c['lr_a'] * theta
    dp = dw + c['lr_a'] * dth + 2 * U * np.abs(c['lr_a'] * theta) + U * np.abs(pn)
    sk = skip_mask(skip, n)
    ref = tuple(np.where(sk, old, new) for old, new in ((p, pn), (m, mn), (v, vn)))
    bnd = tuple(np.where(sk, 0., d * SECOND_ORDER) for d in (dp, dm, dv))              # a skipped element keeps its bits
    return ref, bnd, dict(theta=theta, keep=c['keep'], lr_a=c['lr_a'])


def step_cap(p, g, m, v, step, groups, gidx=None, coef=1., a=1.27, b=1., skip=None):
    """(keep p, lr a pi / 2) per element in fp64: whatever the gradient, |p_new - keep p| <= lr a pi / 2"""
    info = _ref_and_bound(p, g, m, v, step, groups, gidx, coef, a, b, skip)[2]
    return np.asarray(p, dtype=F).astype(D) * info['keep'], info['lr_a'] * math.pi / 2


def ref64(p, g, m, v, step, groups, gidx=None, coef=1., a=1.27, b=1., skip=None):
    """(p, m, v) after the step, in fp64.  `groups`: dicts of lr, betas, weight_decay, decoupled_weight_decay; `gidx`: the group of every element (None:
    group 0); `skip`: [start, end) ranges left untouched"""
    return _ref_and_bound(p, g, m, v, step, groups, gidx, coef, a, b, skip)[0]


def bound(p, g, m, v, step, groups, gidx=None, coef=1., a=1.27, b=1., skip=None, form='kernel'):
    """per-element bounds (dp, dm, dv) on |fp32 evaluation - ref64| (the module docstring derives them); `form`: the kernel's operations or optim.AdamAtan2's"""
    return _ref_and_bound(p, g, m, v, step, groups, gidx, coef, a, b, skip, form)[1]


def over(got, ref, bnd):
    """number of elements of (p, m, v) over their bound; NaN counts"""
    return sum(int((~(np.abs(np.asarray(t, dtype=D) - r) <= d)).sum()) for t, r, d in zip(got, ref, bnd))


def worst(got, ref, bnd):
    """largest |got - ref| / bound over p, m, v (elements with a zero bound must be equal and count as 0 or inf)"""
    out = 0.
    for t, r, d in zip(got, ref, bnd):
        e = np.abs(np.asarray(t, dtype=D) - r)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(d > 0, e / d, np.where(e == 0, 0., np.inf))
        out = max(out, float(np.nanmax(q)) if q.size else 0.)
    return out


FAULTS = ('atan2 arguments swapped', 'bias correction 1 dropped', 'bias correction 2 dropped', 'a dropped', 'b applied to the numerator',
          'eps added to the denominator', 'decay applied after the update', 'L2 term added under decoupled', "wrong group's lr in a straddling block",
          'a skipped range stepped')


def _fma(a_, b_, c_):
    return (a_.astype(D) * b_.astype(D) + c_.astype(D)).astype(F)     # the product is exact in fp64


def emulate(p, g, m, v, step, groups, gidx=None, coef=1., a=1.27, b=1., skip=None, fault=None):
    """the kernel's arithmetic in fp32 on the CPU - the same operations in the same order, np.arctan2 in fp32 for atan2f - with one of FAULTS injected"""
    assert fault is None or fault in FAULTS
    p, g, m, v = (np.asarray(t, dtype=F) for t in (p, g, m, v))
    n = p.size
    gidx = np.zeros(n, dtype=np.int64) if gidx is None else np.asarray(gidx, dtype=np.int64)
    c = per_element(groups, gidx, n, lambda grp: host_consts(grp, step, a, b))
    if fault == "wrong group's lr in a straddling block":              # the block's first thread decides for all of it
        first = gidx[(np.arange(n) // BLOCK) * BLOCK]
        c['lr_a'] = per_element(groups, first, n, lambda grp: host_consts(grp, step, a, b))['lr_a']
    if fault == 'bias correction 1 dropped':
        c['inv_bc1'] = np.ones(n, dtype=F)
    if fault == 'bias correction 2 dropped':
        c['b_isq'] = np.full(n, F(b), dtype=F)
    if fault == 'a dropped':
        c['lr_a'] = per_element(groups, gidx, n, lambda grp: host_consts(grp, step, 1., b))['lr_a']
    if fault == 'L2 term added under decoupled':
        c['l2'] = np.array([F(grp.get('weight_decay', 0.)) for grp in groups], dtype=F)[gidx]
    coef = F(coef)
    gc = g * coef
    keep = np.ones(n, dtype=F) if fault == 'decay applied after the update' else c['keep']
    w = p * keep
    gl = np.where(c['l2'] != 0, _fma(c['l2'], w, gc), gc)
    omb1, omb2 = F(1.) - c['beta1'], F(1.) - c['beta2']
    mn = _fma(c['beta1'], m, omb1 * gl)
    vn = _fma(c['beta2'], v, gl * (omb2 * gl))
    y, x = mn * c['inv_bc1'], np.sqrt(vn) * c['b_isq']
    if fault == 'b applied to the numerator':
        nb = per_element(groups, gidx, n, lambda grp: host_consts(grp, step, a, 1.))['b_isq']
        y, x = y * F(b), np.sqrt(vn) * nb
    if fault == 'eps added to the denominator':
        x = x + F(1e-8)
    theta = np.arctan2(x, y) if fault == 'atan2 arguments swapped' else np.arctan2(y, x)
    assert theta.dtype == F
    pn = w - c['lr_a'] * theta
    if fault == 'decay applied after the update':
        pn = pn * c['keep']
    sk = np.zeros(n, dtype=bool) if fault == 'a skipped range stepped' else skip_mask(skip, n)
    return tuple(np.where(sk, old, new) for old, new in ((p, pn), (m, mn), (v, vn)))


def three_groups():
    """an L2 group, a decoupled group with its own lr and betas (large enough that the ORDER of decay and update shows), a plain group"""
    return [dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1, decoupled_weight_decay=False),
            dict(lr=5e-2, betas=(0.8, 0.95), weight_decay=0.5, decoupled_weight_decay=True),
            dict(lr=3e-4, betas=(0.9, 0.99), weight_decay=0., decoupled_weight_decay=False)]


def group_layout(n):
    """(ranges, gidx) for three_groups() over n elements: boundaries that fall inside a block and one on a block edge; bounds multiples of 4, the tail
    of a buffer that is no multiple of 4 belongs to the last range"""
    n4 = -(-n // 4) * 4
    cuts = sorted({min(n4, c) for c in (0, 8, 300, BLOCK, BLOCK + 516, 2 * BLOCK + 100, n4)})
    order = [0, 1, 2, 1, 0, 2]
    ranges = [(s, e, order[i % len(order)]) for i, (s, e) in enumerate(zip(cuts, cuts[1:]))]
    gidx = np.zeros(n, dtype=np.int64)
    for s, e, k in ranges:
        gidx[s:e] = k
    return ranges, gidx


def skip_layout(n):
    """skip ranges at the start, in the middle and at the end (multiples of 4; the last one covers the tail)"""
    n4 = -(-n // 4) * 4
    if n4 <= 12:
        return [(0, 4)] if n4 > 4 else []
    mid = (n4 // 2) // 4 * 4
    return [(0, 4), (mid, min(mid + 40, n4 - 8)), (n4 - 4, n4)] if mid + 4 < n4 - 8 else [(0, 4), (n4 - 4, n4)]


def make_inputs(n, seed, gscale=1., state=True):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(F)
    g = (rng.standard_normal(n) * gscale).astype(F)
    if state:
        m = (rng.standard_normal(n) * gscale * 0.3).astype(F)
        v = (rng.random(n) * gscale * gscale * 0.5 + F(gscale) * F(gscale) * F(1e-3)).astype(F)
    else:
        m, v = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    return p, g, m, v
