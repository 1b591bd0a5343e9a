"""Parameter-side kernel cases (colsum, Muon prep / norm / apply, sumsq, casts, EMA, scale, noise mix, Fourier features, row scatter): builders, float64
references, per-element bounds, guard bands, and an fp32 CPU emulation with a fault list (not collected: no test_ prefix; imports no GPU code at module level).

Shared by tests/test_param_refs_cpu.py (the emulation of a correct kernel stays under every bound in two orders, every listed fault is caught, and the old
whole-tensor ratio is computed next to it) and tests/test_param_kernels_gpu.py (every entry point through the C ABI).  U16, U32, GUARD, FILL_*, guarded,
assert_elementwise and assert_untouched are those of tests/_gemm_cases.py; E(n, M, c) = (n + c) u32 M, new_out and check_out those of tests/_tokenwise_cases.py.

References are float64 from the exact bf16 / fp32 operand values: a host scalar that reaches the kernel as a C float (decay, momentum, lr, eps, scale) enters
the reference as that float.  In-place outputs start from non-zero values that are part of the reference.

Bound of one element, derived, not tuned (u16 = 2^-8, u32 = 2^-24):
  copies, casts      cast_rows, cast_rows_t, scatter_rows, noise_mix without eps or at t = 0 / t = 1 (x 0 + e 1 is exact in fp32), flow = x - e (one IEEE
                     subtraction): tol = 0 against torch's round-to-nearest-even result.
  sums               colsum, sumsq, sumsq_det, Muon partials, muon_norm: E(n, M), n = the number of terms + 1 for the value added to, M = the float64 sum of the
                     magnitudes.  Any order (atomics across row blocks included).  c = 8 covers the rounding of each square.
  colsum             n = (rows the map names) x (columns mapped to this output) + 1,  M = |out| + sum |x|.
  ema                e' = o + d (e - o): subtraction, product, addition = 3 roundings, + 1 for the contracted form: 4 u32 M, M = |o| + |d| (|e| + |o|).
                     The other order of the emulation, d e + (1 - d) o, has 1 - d, two products and a sum: within 3 u32 M as well.
  scale_bf16_dev     y = bf16(x s): one fp32 product: E = 2 u32 |y|, tol = u16 |y| + 2 E.  s == 1: the kernel returns early, every bit stays.
  noise_mix          y = bf16(x t + e (1 - t)): 1 - t, two products, one sum, + 1 for contraction: E = 5 u32 (|x t| + |e (1 - t)|), tol = u16 |y| + 2 E.
  fourier            arg = (t w) 6.2831855f: two fp32 products and the rounded constant (off by 2.8e-8 relative < u32) move it by 3 |arg| u32; |sin'|, |cos'| <= 1.
                     The kernel calls sinf / cosf without fast-math flags: the device library's full-range functions (Payne-Hanek reduction), documented at 2 ulp
                     = 4 u32 of a value <= 1 - inside the 8 u32 the bound allows, so the figure stays (3 |arg| + 8) u32 = E, tol = u16 |y| + 2 E.  Column 0 is bf16(t): u16 |t|.
  Muon coefficient   coef = gs min(1, max_norm / (sqrt(sumsq) gs + 1e-6)): sqrt, product, sum, quotient, product = 5 roundings, g coef one more: the scaled gradient
                     g' is within 7 u32 |g'|.
  Muon buf           b' = lerp(b, g', 1 - mu): the weight (1 rounding), difference, product, sum, + 1 for contraction on top of g': <= 11 u32 (|g'| + |b|).
                     c = 14, M = |g'| + |b|  (stated, with slack for the 1 - w of the upper branch).
  Muon u             u = lerp(g', b', mu) (Nesterov) or b': 11 u32 M from b', 7 from g', difference / product / sum on |g'| + |b'| <= 2 M: c = 20, same M.
                     bf16 copies: u16 |u| + 2 E_u.  The transposed copy must equal the straight one bit for bit.
  Muon buf, u / lerp additionally within 2 ulp of CPU fp32 torch.lerp on the same fp32 g' (what torch.optim.Muon executes); the ulp is the spacing of fp32 at
                     the lerp result.
  Muon partials      sum of u^2 over a 64 x 64 block: E(valid + 1, sum u^2) + sum 2 |u| E_u  (the squares inherit u's error).
  muon_norm          from the partials the kernel is given: tot within E(nb + 1, tot); r = 1 / max(sqrt(tot), eps): half the relative error of tot, sqrt and the
                     reciprocal at 1 ulp each = 4 u32; r^2 twice that + 1.  Below eps (the all-zero matrix): 4 u32 of 1 / eps.
  Muon apply         p' = fma(-(lr ratio), o, p decay): lr ratio, p decay, the fma, + 1: 4 u32 M, M = |p decay| + |lr ratio o|.

Guard bands: every output sits in a guarded buffer (vectors: one row between two guard blocks, so guard elements follow the last one).  The colsum source is a
view that starts GUARD rows inside a larger buffer whose first rows hold 1e4: an index of -1 lands in memory the test owns and is a value error.  The cast
source lies at an odd float offset of a flat buffer with 1e4 behind it.  The Muon matrices lie at multiples of 4 floats of flat buffers with gaps between
them; the gaps of g, buf, p and the padding of the bf16 workspace must come back bit-identical.

Worst error / bound of the fp32 CPU emulation (first | second order; tests/test_param_refs_cpu.py prints them):
  colsum out 0.100 | 0.100   sumsq 0.053 | 0.053   sumsq_det 0.046 | 0.046   ema 0.642 | 0.339   scale 0.663 | 0.663   noise xt 0.987 | 0.987   fourier 0.976 | 0.976
  muon buf 0.161 | 0.161   ws 0.995 | 0.995   partials 0.033 | 0.032   inv 0.149 | 0.166   apply 0.491 | 0.491   (copies, casts, flow: 0 - exact)
The MI355X figures per kernel form are in profiles/param_side_bounds.txt.
"""
from types import SimpleNamespace

import torch

from _gemm_cases import BF, FILL_BF16, FILL_F32, GUARD, U16, U32, _bits, assert_elementwise, assert_untouched, guarded, padded, relerr, tol_bf16  # noqa: F401
from _tokenwise_cases import E, check_out, check_outs, colsum, gen, new_out, old_ratio, seqsum, treesum  # noqa: F401

SENT = 1e4                                           # sentinel in front of / behind sources
NO_DIRECT_TOL = 1e-2                                 # outputs the older suite reaches only through model-level tests: their tightest tolerance
OLD_TOL = {'out': 1e-4, 'cast': 4e-3, 'cast_t': 4e-3, 'xt': 4e-3, 'flow': 1e-6, 'fourier': 4e-3}      # tests/test_kernels_gpu.py

F32 = torch.float32
f32 = lambda v: float(torch.tensor(float(v), dtype=F32))        # a host scalar as the C float the kernel receives


def vec_out(name, n, dtype, device, ref=None, tol=None, mask=None, init=None):
    return new_out(name, 1, n, dtype, device, ref, tol, mask, init)


def bigsum(x, order):
    """fp32 sum of a long vector: `linear` = 1024 lanes striding through it, each in order, then the lanes in order; `tree` = by halving"""
    if order == 'tree' or x.numel() == 0:
        return treesum(x, 0) if x.numel() else torch.zeros((), dtype=x.dtype)
    n = x.numel()
    k = -(-n // 1024)
    xp = torch.cat([x, torch.zeros(k * 1024 - n, dtype=x.dtype)]).reshape(k, 1024)
    return seqsum(seqsum(xp, 0), 0)


# ---------------------------------------------------------------------------------------------- tfx_colsum_bf16
COLSUM8_SHAPES = [(C, C + p) for C in (8, 64, 512, 520, 1024) for p in (0, 8)]                 # (C, ld): C % 8 == 0 and ld % 8 == 0 -> colsum8_k
COLSUM_SCALAR_SHAPES = [(1, 1), (63, 63), (65, 72), (130, 131), (64, 68)]                      # everything else -> colsum_k<bf16>
COLSUM_R = (1, 7, 8, 9, 63, 64, 65, 130, 1001)       # under / at / over the 8-row lanes and the 64-row main loop; 1001: more than one row block (rpb8 >= 64)
COLSUM_MAPS = ('none', 'rows', 'rows_neg', 'cols', 'both')


def colsum_form(C, ld):
    return 'colsum8_k' if C % 8 == 0 and ld % 8 == 0 else 'colsum_k'


def build_colsum(R, C, ld, maps, device='cpu', seed=0):
    """out[colmap[c]] += sum over r of src[rowmap[r]][c].  maps: none | rows (a permutation with repeats) | rows_neg (-1 at the first, the last and an interior
    position) | cols (-1, and two columns onto one output) | both.  Column 3 of the source is zero: its output must not be touched."""
    g = gen(seed, R, C, ld, COLSUM_MAPS.index(maps), 11)
    use_rows, use_cols = maps in ('rows', 'rows_neg', 'both'), maps in ('cols', 'both')
    Rsrc = R // 2 + 1 if use_rows else R
    big = torch.full((GUARD + Rsrc, ld), SENT, dtype=BF)
    data = torch.randn(Rsrc, C, generator=g).to(BF)
    if C >= 4:
        data[:, 3] = 0
    big[GUARD:, :C] = data
    c = SimpleNamespace(R=R, C=C, ld=ld, maps=maps, device=device, form=colsum_form(C, ld), rowmap=None, colmap=None)
    rows = torch.arange(R)
    if use_rows:
        rows = torch.randint(0, Rsrc, (R,), generator=g)
        if maps != 'rows':
            rows[0] = rows[R - 1] = rows[R // 2] = -1
        c.rowmap = rows.to(torch.int32).to(device)
    cols = torch.arange(C)
    if use_cols:
        cols = torch.randperm(C, generator=g)
        if C >= 2:
            cols[1] = cols[0]
        if C >= 3:
            cols[max(C // 2, 2)] = -1
        c.colmap = cols.to(torch.int32).to(device)
    c.rows, c.cols = rows, cols
    c.big = big.to(device)
    c.src = c.big[GUARD:]
    init = torch.randn(C, generator=g)
    valid = rows >= 0
    X = data[rows[valid]].double()
    s, sa = X.sum(0), X.abs().sum(0)
    cv = cols >= 0
    z = torch.zeros(C, dtype=torch.float64)
    add, mag = z.clone().index_add_(0, cols[cv], s[cv]), z.clone().index_add_(0, cols[cv], sa[cv])
    n_cols = z.clone().index_add_(0, cols[cv], torch.ones(int(cv.sum()), dtype=torch.float64))
    ref = init.double() + add
    tol = E(int(valid.sum()) * n_cols + 1, init.double().abs() + mag)
    c.out = vec_out('out', C, F32, device, ref.to(device), tol.to(device), (mag > 0).to(device), init.to(device))
    return c


def emulate_colsum(c, order, fault=None):
    """Faults: neg_row_reads_previous_row (1), colsum8_tail_dropped (2: rows [64 (R / 64), R) never summed), dup_colmap_overwrites (3)"""
    big = c.big.float()
    sel = torch.ones(c.R, dtype=torch.bool) if fault == 'neg_row_reads_previous_row' else c.rows >= 0
    if fault == 'colsum8_tail_dropped':
        sel = sel & (torch.arange(c.R) < c.R // 64 * 64)
    X = big[(c.rows + GUARD)[sel]][:, :c.C]                     # row -1 is the last sentinel row in front of the source
    s = colsum(X, order) if X.shape[0] else torch.zeros(c.C)
    out = c.out.view[0]
    init = out.clone()
    for col in range(c.C):
        co = int(c.cols[col])
        if co < 0 or float(s[col]) == 0.:
            continue
        out[co] = (init[co] if fault == 'dup_colmap_overwrites' else out[co]) + s[col]


# ---------------------------------------------------------------------------------------------- tfx_sumsq / tfx_sumsq_det
SUMSQ_N = (1, 3, 4, 5, 1023, 4099, 2 ** 20 + 7, 2 ** 21 + 5)        # the 4-element groups and their tail; 2^21 + 5: the grid-stride loop of 2048 blocks x 256 x 4 runs a second trip
SUMSQ_INIT = 3.25


def build_sumsq(n, device='cpu', seed=0):
    g = (torch.randn(n, generator=gen(seed, n, 12)) * 0.5).to(device)
    s = (g.double() ** 2).sum().reshape(1)
    c = SimpleNamespace(n=n, g=g, device=device)
    c.out = vec_out('sumsq', 1, F32, device, s + SUMSQ_INIT, E(n + 1, s + SUMSQ_INIT), init=torch.full((1,), SUMSQ_INIT, device=device))
    c.det = vec_out('sumsq_det', 1, F32, device, s, E(n, s))                        # starts poisoned (the guard pattern): overwritten, not accumulated
    return c


def emulate_sumsq(c, order, fault=None):
    """Fault sumsq_tail_dropped (10): the n % 4 elements behind the last group of 4 are never read"""
    x = c.g.float()
    if fault == 'sumsq_tail_dropped':
        x = x[:c.n // 4 * 4]
    s = bigsum(x * x, order)
    c.out.view[0, 0] += s
    c.det.view[0, 0] = s


# ---------------------------------------------------------------------------------------------- tfx_ema_update / tfx_scale_bf16_dev
VEC_N = (1, 3, 4, 5, 7, 8, 9, 1027, 2053)
EMA_DECAYS = (0., 0.5, 0.9999, 1.)
SCALES = (1., 1. / 3., -2.)


def build_ema(n, decay, device='cpu', seed=0):
    g = gen(seed, n, 13)
    e, o = torch.randn(n, generator=g).to(device), torch.randn(n, generator=g).to(device)
    d = f32(decay)
    ref = o.double() + d * (e.double() - o.double())
    tol = 4 * U32 * (o.double().abs() + abs(d) * (e.double().abs() + o.double().abs()))
    c = SimpleNamespace(n=n, decay=d, online=o, device=device)
    c.out = vec_out('ema', n, F32, device, ref, tol, init=e)
    return c


def emulate_ema(c, order, fault=None):
    """Fault ema_online_swapped (12)"""
    e, o, d = c.out.view[0].clone(), c.online, torch.tensor(c.decay, dtype=F32)
    if fault == 'ema_online_swapped':
        e, o = o, e
    c.out.view[0] = o + d * (e - o) if order == 'linear' else d * e + (1 - d) * o


def build_scale(n, scale, device='cpu', seed=0, specials=False):
    x = (torch.randn(n, generator=gen(seed, n, 14)) * 2).to(BF)
    if specials:                                          # NaN with a payload, infinities, -0, a subnormal: a scale of exactly 1 keeps every bit
        sp = torch.tensor([0x7FC1, -0x0041, 0x7F80, -0x0080, -0x8000, 0x0001], dtype=torch.int16)      # (int16 views of 0x7FC1, 0xFFBF, 0x7F80, 0xFF80, 0x8000, 0x0001)
        k = min(n, sp.numel())
        _bits(x)[:k] = sp[:k]
    x = x.to(device)
    s = f32(scale)
    ref = x.double() * s
    c = SimpleNamespace(n=n, scale=torch.tensor([s], dtype=F32, device=device), device=device)
    c.out = vec_out('x', n, BF, device, ref, tol_bf16(ref, 2 * U32 * ref.abs()) if s != 1. else torch.zeros_like(ref), init=x)
    return c


def emulate_scale(c, order, fault=None):
    """Fault scale_through_bf16_twice (14): the scalar is rounded to bf16 before the product, the product once more"""
    s = c.scale[0]
    if float(s) == 1.:
        return
    if fault == 'scale_through_bf16_twice':
        s = s.to(BF).float()
    c.out.view[0] = (c.out.view[0].float() * s).to(BF)


# ---------------------------------------------------------------------------------------------- tfx_cast_rows / tfx_cast_rows_t
CAST_SHAPES = ((1, 1), (33, 31), (200, 70), (64, 64))


def _not32(v):
    return v + 1 if v % 32 == 0 else v


def build_cast(Rs, Cs, use_map, cd, transposed, device='cpu', seed=0):
    """plain: dst[r][c] = src[map(r)][c], Rd logical rows, Cd columns (cd = 'lt': Cd < Cs, 'gt': Cd > Cs), zero elsewhere in [Rd, ld_dst].
    transposed: dst[c][r] = src[map(r)][c] for the Cd logical rows r; dst has Rd = Cs + 3 rows.  Map values in [-1, Rs + 5)."""
    g = gen(seed, Rs, Cs, int(use_map), int(cd == 'lt'), int(transposed), 15)
    tail = 6
    flat = torch.full((3 + (Rs + tail) * Cs + 5,), SENT)
    flat[3:3 + Rs * Cs] = torch.randn(Rs * Cs, generator=g)
    if not transposed:
        Cd = Cs // 2 if cd == 'lt' else Cs + 3
        Rd = _not32(Rs + 24 if use_map else Rs + 5)
        ld = _not32(max(Cs, Cd) + 5)
        nmap = Rd
    else:
        Cd = Cs // 2 if cd == 'lt' else Cs + Rs + 3
        Rd, ld, nmap = _not32(Cs + 3), _not32(Cd + 5), Cd
    c = SimpleNamespace(Rs=Rs, Cs=Cs, Cd=Cd, Rd=Rd, ld=ld, transposed=transposed, device=device, rowmap=None, nmap=nmap)
    rows = torch.arange(nmap)
    if use_map:
        rows = torch.randint(-1, Rs + 5, (max(nmap, 1),), generator=g)
        c.rowmap = rows.to(torch.int32).to(device)
        rows = rows[:nmap]
    c.rows = rows
    c.flat = flat.to(device)
    c.src = c.flat[3:3 + Rs * Cs].view(Rs, Cs)
    c.out = new_out('cast_t' if transposed else 'cast', Rd, ld, BF, device)
    c.out.ref, c.out.tol = _cast_full(c, flat, rows, (rows >= 0) & (rows < Rs)).to(BF).double().to(device), torch.zeros(Rd, ld, dtype=torch.float64, device=device)
    return c


def _cast_full(c, flat, rows, ok):
    logical = torch.zeros(c.nmap, c.Cs)
    idx = 3 + rows[ok].clamp(max=c.Rs + 4)[:, None] * c.Cs + torch.arange(c.Cs)[None]
    logical[ok] = flat.cpu()[idx]
    full = torch.zeros(c.Rd, c.ld)
    if not c.transposed:
        cm = min(c.Cs, c.Cd)
        full[:, :cm] = logical[:, :cm]
    else:
        cc = min(c.Cs, c.Rd)
        full[:cc, :c.Cd] = logical[:, :cc].T
    return full


def emulate_cast(c, order, fault=None):
    """Fault cast_t_reads_rows_past_Rs (11): rs >= Rs is not turned into zeros - the rows behind the source are read"""
    ok = (c.rows >= 0) & (c.rows < c.Rs)
    if fault == 'cast_t_reads_rows_past_Rs':
        ok = c.rows >= 0
    c.out.view[:] = _cast_full(c, c.flat, c.rows, ok).to(BF)


# ---------------------------------------------------------------------------------------------- tfx_noise_mix
NOISE_SHAPES = ((1, 1, 8), (3, 5, 8), (300, 48, 64), (37, 64, 64))


def build_noise(R, dl, ld_xt, device='cpu', seed=0, with_eps=True):
    g = gen(seed, R, dl, ld_xt, 16)
    I = max(3, R // 7 + 1)
    times = torch.rand(I, generator=g)
    times[0], times[1] = 0., 1.
    row_inst = torch.randint(0, I, (R,), generator=g)
    row_inst[0] = 2 if R >= 3 else 0                     # (R = 1: the one row is at t = 0 exactly)
    if R >= 3:
        row_inst[1], row_inst[R - 1] = 0, 1
    x, e = torch.randn(R, dl, generator=g), torch.randn(R, dl, generator=g)
    t = times[row_inst].double()[:, None]
    ref, tol = torch.zeros(R, ld_xt, dtype=torch.float64), torch.zeros(R, ld_xt, dtype=torch.float64)
    if with_eps:
        y = x.double() * t + e.double() * (1 - t)
        exact = (t == 0) | (t == 1)
        y = torch.where(t == 0, e.to(BF).double(), torch.where(t == 1, x.to(BF).double(), y))
        ref[:, :dl] = y
        tol[:, :dl] = torch.where(exact, torch.zeros_like(y), tol_bf16(y, 5 * U32 * ((x.double() * t).abs() + (e.double() * (1 - t)).abs())))
    else:
        ref[:, :dl] = x.to(BF).double()
    c = SimpleNamespace(R=R, dl=dl, ld_xt=ld_xt, device=device, with_eps=with_eps, x=x.to(device), eps=e.to(device), times=times.to(device),
                        row_inst=row_inst.to(torch.int32).to(device))
    c.xt = new_out('xt', R, ld_xt, BF, device, ref.to(device), tol.to(device))
    c.flow = new_out('flow', R, dl, F32, device, (x - e).double().to(device), torch.zeros(R, dl, dtype=torch.float64, device=device),
                     mask=torch.full((R, dl), with_eps, dtype=torch.bool, device=device))
    return c


def emulate_noise(c, order, fault=None, flow=True):
    """Fault noise_time_of_row_0 (13)"""
    xt = torch.zeros(c.R, c.ld_xt)
    if not c.with_eps:
        xt[:, :c.dl] = c.x
        c.xt.view[:] = xt.to(BF)
        return
    ri = c.row_inst.long()
    t = (c.times[ri[0]].expand(c.R) if fault == 'noise_time_of_row_0' else c.times[ri])[:, None]
    xt[:, :c.dl] = c.x * t + c.eps * (1 - t)
    c.xt.view[:] = xt.to(BF)
    if flow:
        c.flow.view[:] = c.x - c.eps


# ---------------------------------------------------------------------------------------------- tfx_fourier
FOURIER_SHAPES = ((1, 1, 8), (40, 32, 128), (3, 200, 520))          # ld = 520 > blockDim: the column loop runs three trips
TWO_PI_F = f32(6.283185307179586)


def build_fourier(I, half, ld, device='cpu', seed=0):
    import math
    g = gen(seed, I, half, ld, 17)
    times = torch.rand(I, generator=g)
    times[0] = 0.
    if I > 1:
        times[1] = 1.
    w = torch.randn(half, generator=g)
    arg = times.double()[:, None] * w.double()[None] * (2 * math.pi)
    Ea = (3 * arg.abs() + 8) * U32
    ref, tol = torch.zeros(I, ld, dtype=torch.float64), torch.zeros(I, ld, dtype=torch.float64)
    ref[:, 0], tol[:, 0] = times.double(), U16 * times.double()
    ref[:, 1:half + 1], ref[:, half + 1:2 * half + 1] = arg.sin(), arg.cos()
    tol[:, 1:half + 1], tol[:, half + 1:2 * half + 1] = tol_bf16(arg.sin(), Ea), tol_bf16(arg.cos(), Ea)
    c = SimpleNamespace(I=I, half=half, ld=ld, device=device, times=times.to(device), w=w.to(device))
    c.out = new_out('fourier', I, ld, BF, device, ref.to(device), tol.to(device))
    return c


def emulate_fourier(c, order):
    k = torch.tensor(TWO_PI_F, dtype=F32)
    a = (c.times[:, None] * c.w[None]) * k if order == 'linear' else c.times[:, None] * (c.w[None] * k)
    o = torch.zeros(c.I, c.ld)
    o[:, 0], o[:, 1:c.half + 1], o[:, c.half + 1:2 * c.half + 1] = c.times, a.sin(), a.cos()
    c.out.view[:] = o.to(BF)


# ---------------------------------------------------------------------------------------------- tfx_scatter_rows_bf16
SCATTER_COLS = (8, 64, 520)


def build_scatter(cols, device='cpu', seed=0, R=37):
    """dst[rowmap[r]][0:cols] = src[r][0:cols]; ld_src = ld_dst = cols + 8: the 8 columns behind `cols` of every destination row, the rows no entry names and
    the rows of -1 entries stay bit-identical"""
    g = gen(seed, cols, R, 18)
    sbuf, src = padded(torch.randn(R, cols, generator=g).to(BF).to(device))            # 1e4 in the padding of the source
    Rdst, ld = R + 11, cols + GUARD
    rowmap = torch.randperm(Rdst, generator=g)[:R]
    rowmap[0] = rowmap[R // 2] = rowmap[R - 1] = -1
    hit = rowmap >= 0
    ref = torch.zeros(Rdst, ld, dtype=torch.float64)
    ref[rowmap[hit], :cols] = src.cpu().double()[hit]
    mask = torch.zeros(Rdst, ld, dtype=torch.bool)
    mask[rowmap[hit], :cols] = True
    c = SimpleNamespace(cols=cols, R=R, Rdst=Rdst, sbuf=sbuf, src=src, ld_src=ld, ld_dst=ld, rowmap=rowmap.to(torch.int32).to(device), device=device)
    c.out = new_out('dst', Rdst, ld, BF, device, ref.to(device), torch.zeros(Rdst, ld, dtype=torch.float64, device=device), mask.to(device))
    return c


def emulate_scatter(c, order=None):
    rm = c.rowmap.long()
    c.out.view[rm[rm >= 0], :c.cols] = c.src[rm >= 0]


# ---------------------------------------------------------------------------------------------- Muon: prep, norm, apply
MUON_SHAPES = ((64, 64), (65, 63), (130, 40), (40, 130), (1, 200), (200, 1), (128, 128), (1088, 1024))      # (130, 40) and (200, 1) are flipped; (1088, 1024): 272 blocks
MUON_SMALL = MUON_SHAPES[:7]
MUON_MOMENTA = (0., 0.3, 0.5, 0.95)                    # 1 - mu and mu on both sides of torch.lerp's 0.5 branch, and on it
MUON_CLIPS = (dict(max_norm=0., grad_scale=1., sumsq=9.), dict(max_norm=1., grad_scale=1., sumsq=9.),       # no clip | active (norm 3)
              dict(max_norm=1., grad_scale=1., sumsq=0.25), dict(max_norm=1., grad_scale=0.5, sumsq=9.))   # inactive (norm 0.5) | grad_scale != 1, active (norm 1.5)
MUON_EPS = 1e-7
PB = 64


def muon_segments(shapes):
    """(offset, rows, cols) at multiples of 4 floats with gaps of 4, 8, 12 floats between the matrices (and in front of the first)"""
    segs, off = [], 4
    for i, (r, c) in enumerate(shapes):
        segs.append((off, r, c))
        off += -(-r * c // 4) * 4 + 4 * (i % 3 + 1)
    return segs, off


def build_muon(shapes=MUON_SHAPES, device='cpu', seed=0, zero_mat=None):
    """flat g / buf / p with the matrices of `shapes`, the host tables of optim._muon_host_tables, and the flat index of every matrix element in the fp32
    buffers (`fi`), in the straight and the transposed bf16 copy (`ps`, `pt`) and its block (`blk`).  zero_mat: that matrix has zero gradient and momentum."""
    from transfusion_pytorch_amd.optim import _muon_host_tables
    g0 = gen(seed, len(shapes), 19)
    segs, total = muon_segments(shapes)
    H = _muon_host_tables(segs)
    ratio0 = [m['lr_ratio'] for m in H['mats']]
    for i, m in enumerate(H['mats']):                       # a distinct ratio per matrix (the shapes alone give 1.0 four times)
        m['lr_ratio'] = ratio0[i] * (1 + i / 8)
    c = SimpleNamespace(shapes=shapes, segs=segs, total=total, H=H, device=device, nmat=len(segs), nblk=len(H['blk_mat']), x_elems=H['x_elems'], ratio0=ratio0)
    fi, ps, pt, blk, mat, lr, lc = [], [], [], [], [], [], []
    for i, m in enumerate(H['mats']):
        r, cc = torch.meshgrid(torch.arange(m['rows']), torch.arange(m['cols']), indexing='ij')
        r, cc = r.reshape(-1), cc.reshape(-1)
        fi.append(m['off'] + r * m['cols'] + cc)
        ps.append(m['s_off'] + r * m['ld_s'] + cc)
        pt.append(m['t_off'] + cc * m['ld_t'] + r)
        nbc = -(-m['cols'] // PB)
        blk.append(m['blk0'] + (r // PB) * nbc + cc // PB)
        mat.append(torch.full_like(r, i)); lr.append(r); lc.append(cc)
    c.fi, c.ps, c.pt, c.blk, c.mat, c.lr, c.lc = (torch.cat(v).to(device) for v in (fi, ps, pt, blk, mat, lr, lc))
    c.in_mat = torch.zeros(total, dtype=torch.bool, device=device)
    c.in_mat[c.fi] = True

    def flat(scale):
        t = torch.randn(total, generator=g0) * scale
        _bits(t)[~c.in_mat.cpu()] = FILL_F32
        return t.to(device)
    c.g, c.buf0, c.p0 = flat(1.), flat(0.5), flat(1.)
    if zero_mat is not None:
        sel = c.fi[c.mat == zero_mat]
        c.g[sel] = 0; c.buf0[sel] = 0
    c.lr_ratio = torch.tensor([m['lr_ratio'] for m in H['mats']], dtype=F32, device=device)
    c.flip = [bool(m['flip']) for m in H['mats']]
    # apply's operand: independent bf16 patterns in the straight and the transposed copy (reading the wrong one is O(1) off)
    wsa = torch.zeros(c.x_elems, dtype=BF)
    n = c.fi.numel()
    wsa[c.ps.cpu()] = torch.randn(n, generator=g0).to(BF)
    wsa[c.pt.cpu()] = torch.randn(n, generator=g0).to(BF)
    c.ws_apply = wsa.to(device)
    return c


def _lerp64(a, b, w):
    return a + w * (b - a) if w < 0.5 else b - (b - a) * (1 - w)


def muon_coef(clip, dtype=torch.float64):
    """the clip coefficient from the fp32 operands, in `dtype` arithmetic"""
    gs, mn, ss = (torch.tensor(f32(clip[k]), dtype=dtype) for k in ('grad_scale', 'max_norm', 'sumsq'))
    coef = gs
    if float(mn) > 0:
        coef = coef * torch.minimum(torch.ones((), dtype=dtype), mn / (ss.sqrt() * gs + torch.tensor(f32(1e-6), dtype=dtype)))
    return coef


def muon_prep_outs(c, momentum, nesterov, clip, ws_poison=False):
    """guarded outputs of one tfx_muon_prep launch with their references: buf (flat, gaps untouched), ws (both copies; the padding untouched, zero or
    poisoned), partials; plus `lerp_buf` / `lerp_u`: what CPU fp32 torch.lerp gives on the same fp32 scaled gradient"""
    dev = c.device
    mu = f32(momentum)
    w1_32 = float(torch.tensor(1., dtype=F32) - torch.tensor(mu, dtype=F32))
    coef = float(muon_coef(clip))
    G, B = c.g.double()[c.fi] * coef, c.buf0.double()[c.fi]
    b1 = _lerp64(B, G, w1_32)
    u = _lerp64(G, b1, mu) if nesterov else b1
    M = G.abs() + B.abs()
    o = SimpleNamespace(momentum=mu, nesterov=bool(nesterov), clip=clip)
    z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
    ref, tol = z(c.total), z(c.total)
    ref[c.fi], tol[c.fi] = b1, 14 * U32 * M
    o.buf = vec_out('buf', c.total, F32, dev, ref, tol, c.in_mat, c.buf0)
    Eu = 20 * U32 * M
    ref, tol, mask = z(c.x_elems), z(c.x_elems), torch.zeros(c.x_elems, dtype=torch.bool, device=dev)
    for pos in (c.ps, c.pt):
        ref[pos], tol[pos], mask[pos] = u, tol_bf16(u, Eu), True
    o.ws = vec_out('ws', c.x_elems, BF, dev, ref, tol, mask, None if ws_poison else torch.zeros(c.x_elems, dtype=BF, device=dev))
    S = z(c.nblk).index_add_(0, c.blk, u * u)
    cnt = z(c.nblk).index_add_(0, c.blk, torch.ones_like(u))
    o.partials = vec_out('partials', c.nblk, F32, dev, S, E(cnt + 1, S) + z(c.nblk).index_add_(0, c.blk, 2 * u.abs() * Eu))
    o.u_ref, o.u_tol = u, Eu
    # torch.lerp in fp32 on the CPU, on the fp32 scaled gradient
    g32 = (c.g[c.fi].cpu() * muon_coef(clip, F32))
    lb = torch.lerp(c.buf0[c.fi].cpu(), g32, torch.tensor(w1_32, dtype=F32))
    o.lerp_buf = lb.to(dev)
    o.lerp_u = (torch.lerp(g32, lb, torch.tensor(mu, dtype=F32)) if nesterov else lb).to(dev)
    return o


def ulps(got, ref32):
    """|got - ref| in units of the fp32 spacing at ref (the spacing of the smallest normal number below it)"""
    a = ref32.abs().clamp_min(2.0 ** -126)
    return ((got.double() - ref32.double()).abs() / (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double())


def _lerp32(a, b, w):
    w = torch.tensor(w, dtype=F32)
    return a + w * (b - a) if float(w) < 0.5 else b - (b - a) * (1 - w)


def emulate_muon_prep(c, o, order, fault=None):
    """fp32 emulation of muon_prep_kernel.  Faults: transposed_edge_block_swapped (4), partial_last_row_group_dropped (5), clip_after_momentum (6),
    nesterov_reads_old_buf (7)"""
    coef = muon_coef(o.clip, F32)
    graw, b0 = c.g[c.fi], c.buf0[c.fi]
    w1 = float(torch.tensor(1., dtype=F32) - torch.tensor(o.momentum, dtype=F32))
    g = graw if fault == 'clip_after_momentum' else graw * coef
    b1 = _lerp32(b0, g, w1)
    u = _lerp32(g, b0 if fault == 'nesterov_reads_old_buf' else b1, o.momentum) if o.nesterov else b1
    if fault == 'clip_after_momentum':
        u = u * coef
    o.buf.view[0, c.fi] = b1
    ub = u.to(BF)
    o.ws.view[0, c.ps] = ub
    ut = ub.clone()
    if fault == 'transposed_edge_block_swapped':           # in a ragged edge block the value for (c0 + j, r0 + i) is taken from tile[j][i], not tile[i][j]
        for i, m in enumerate(c.H['mats']):                # (one matrix: the first with a ragged edge)
            if (m['rows'] % PB == 0 and m['cols'] % PB == 0) or i > 1:
                continue
            sel = (c.mat == i).nonzero().flatten()
            U = torch.zeros(-(-m['rows'] // PB) * PB, -(-m['cols'] // PB) * PB, dtype=BF)
            U[c.lr[sel], c.lc[sel]] = ub[sel]
            r, cc = c.lr[sel], c.lc[sel]
            ragged = ((r // PB + 1) * PB > m['rows']) & (r // PB == (m['rows'] - 1) // PB)      # its bottom edge blocks
            r2, c2 = r // PB * PB + cc % PB, cc // PB * PB + r % PB
            ut[sel] = torch.where(ragged, U[r2, c2], ub[sel])
    o.ws.view[0, c.pt] = ut
    sq = (u * u).clone()
    if fault == 'partial_last_row_group_dropped':
        sq[c.lr % PB >= PB - 4] = 0
    tile = torch.zeros(c.nblk * PB * PB)
    tile[c.blk * PB * PB + (c.lr % PB) * PB + c.lc % PB] = sq
    tile = tile.reshape(c.nblk, PB * PB)
    o.partials.view[0] = seqsum(tile, 1) if order == 'linear' else treesum(tile, 1)


def muon_norm_out(c, partials32, eps=MUON_EPS):
    """reference of tfx_muon_norm from the fp32 partials it is given"""
    dev = c.device
    P = partials32.double()
    e = f32(eps)
    ref, tol = torch.zeros(2 * c.nmat, dtype=torch.float64, device=dev), torch.zeros(2 * c.nmat, dtype=torch.float64, device=dev)
    for i, m in enumerate(c.H['mats']):
        nb = -(-m['rows'] // PB) * -(-m['cols'] // PB)
        tot = float(P[m['blk0']:m['blk0'] + nb].sum())
        s = tot ** 0.5
        rel = 4 * U32 + (0.5 * float(E(nb + 1, 1.)) if s > e else 0.)
        r = 1 / max(s, e)
        ref[2 * i], ref[2 * i + 1] = r, r * r
        tol[2 * i], tol[2 * i + 1] = r * rel, r * r * (2 * rel + U32)
    return vec_out('inv', 2 * c.nmat, F32, dev, ref, tol)


def emulate_muon_norm(c, o, partials32, order, fault=None, eps=MUON_EPS):
    """Fault norm_first_256_partials (9)"""
    for i, m in enumerate(c.H['mats']):
        nb = -(-m['rows'] // PB) * -(-m['cols'] // PB)
        if fault == 'norm_first_256_partials':
            nb = min(nb, 256)
        tot = bigsum(partials32[m['blk0']:m['blk0'] + nb], order)
        r = 1 / torch.maximum(tot.sqrt(), torch.tensor(f32(eps), dtype=F32))
        o.view[0, 2 * i], o.view[0, 2 * i + 1] = r, r * r


def muon_apply_out(c, lr, decay):
    dev = c.device
    lr, decay = f32(lr), f32(decay)
    P, O = c.p0.double()[c.fi], c.ws_apply.double()[c.ps]
    k = lr * c.lr_ratio.double()[c.mat]
    ref, tol = torch.zeros(c.total, dtype=torch.float64, device=dev), torch.zeros(c.total, dtype=torch.float64, device=dev)
    ref[c.fi], tol[c.fi] = P * decay - k * O, 4 * U32 * ((P * decay).abs() + (k * O).abs())
    o = vec_out('p', c.total, F32, dev, ref, tol, c.in_mat, c.p0)
    o.lr, o.decay = lr, decay
    return o


def emulate_muon_apply(c, o, order, fault=None):
    """Fault apply_reads_transposed_copy_of_flipped (8)"""
    src = c.ps
    if fault == 'apply_reads_transposed_copy_of_flipped':
        fl = torch.tensor(c.flip)[c.mat]
        src = torch.where(fl, c.pt, c.ps)
    O = c.ws_apply[src].float()
    k = torch.tensor(o.lr, dtype=F32) * c.lr_ratio[c.mat]
    P = c.p0[c.fi] * torch.tensor(o.decay, dtype=F32)
    o.view[0, c.fi] = P - k * O if order == 'linear' else (-k) * O + P


FAULTS = ('neg_row_reads_previous_row', 'colsum8_tail_dropped', 'dup_colmap_overwrites', 'transposed_edge_block_swapped', 'partial_last_row_group_dropped',
          'clip_after_momentum', 'nesterov_reads_old_buf', 'apply_reads_transposed_copy_of_flipped', 'norm_first_256_partials', 'sumsq_tail_dropped',
          'cast_t_reads_rows_past_Rs', 'ema_online_swapped', 'noise_time_of_row_0', 'scale_through_bf16_twice')
