"""Token-wise kernel cases (csrc/tokenwise.hip): builders, fp64 references, per-element bounds, guard bands, and an fp32 CPU emulation with a fault list
(not collected: no test_ prefix; imports no GPU code at module level).

Shared by tests/test_tokenwise_refs_cpu.py (the emulation of a correct kernel stays under every bound in two summation orders, every listed fault is caught -
and the older whole-tensor ratio misses the subtle ones), tests/test_tokenwise_rows_gpu.py (every launch form through the C ABI) and three tests of
tests/test_kernels_gpu.py.  U16, U32, assert_elementwise, assert_untouched and guarded are those of tests/_gemm_cases.py.

References are float64 from the exact bf16 / fp32 operand values.  Where a kernel chain re-reads a stored bf16 row (tfx_layer_end_fwd, tfx_adaln_post_pre_fwd,
tfx_adaln_pre_post_bwd) the reference of the later stage takes the STORED row as its operand - it rounds where the contract rounds and nowhere else.  The
backward of AdaLN-pre reads `mean` / `rstd` as fp32 operands (the reference values rounded to fp32), as the kernel reads what the forward saved.  In-place
outputs (dx +=, dhiddens with first = 0, every atomically accumulated vector) start from non-zero values that are part of the reference.

Bound of one element, derived, not tuned (u16 = 2^-8, u32 = 2^-24):
  E = (n + c) u32 M     n = the number of accumulated terms (d for a row statistic; the contributing tokens of a column sum or table row, + 1 for the value
                        it is added to), M = the float64 sum of the MAGNITUDES of the terms (so a reference near zero keeps an absolute term and no element
                        is excluded), c = 8 for the handful of elementwise roundings around the sum (c = 12 / 80 where stated).  Any summation order.
  fp32 outputs          tol = E
  bf16 outputs          tol = u16 |y| + 2 E   (u16 |y| is sharp: a correct kernel sits at 0.9 - 1.0 of it; see the table below)
  AdaLN-pre forward     M = (|x - mean| + mean|x|) rstd |1 + gamma| + |beta|: the mean is off by <= d u32 mean|x|, rstd by (d / 2 + 5) u32 relative (the variance
                        sum, the + 1e-5 and rsqrtf at 1 ulp), three more roundings to the output.  mean: E(d, mean|x|); rstd: E(d, rstd).
  AdaLN-pre backward    dx = dx0 (+ add) + rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = du (1 + gamma): M = |dx0| + |add| + rstd (|dxh| + mean|dxh| + |xh| mean|dxh xh|).
                        table / gamma_text gradients: n = tokens of the instance / text tokens, M = sum |du xh| (resp. sum |du|).
  sigmoid               sigmoidf_(z) = v_rcp_f32(1 + __expf(-z)) is within (|z| + 5) u32 relative (the derivation of A_SILU in _gemm_cases.py): A_SIG = (|z| + 5) u32 sigma.
                        sigma (1 - sigma) is then within sigma A_SIG' = (|z| + 5) u32 sigma absolute (both factors move by A_SIG).
  AdaLN-post            out = x + y sc: E(2, |x| + |y| sc) + |y| A_SIG;  dy = g sc: E(1, |dy|) + |g| A_SIG;  dz = (sum g y) sigma (1 - sigma): E(n, sum|g y| sigma (1 - sigma)) + sum|g y| A_SIG;
                        dlayerscale / dbias: column sums over the text / all tokens.
  RMSNorm               y = x r (1 + gamma), r = sqrt(d) / max(|x|, 1e-12): E(d, |y|) (sum of squares d u32, halved by the root, sqrt / divide / three products).
                        dx = r (1 + gamma) dy - x (r^3 / d) S, S = sum (1 + gamma) dy x: M = |r (1 + gamma) dy| + 3 |x| (r^3 / d) sum|(1 + gamma) dy x| - r enters cubed, hence the 3.
  depth softmax         s_l = <h_l, w> / max(|h_l|, 1e-12) is off by e_l = E(d, sum|h_l||w| / |h_l|).  A softmax weight moves by |d s_l - sum_k a_k d s_k| <= 2 max e relative,
                        plus the exponentials: __expf(x) = v_exp_f32(x log2 e) is within (1.5 |x| + 3) u32 relative, every argument lies in [-R, 0], R = max s - min s, and the
                        online form rescales L times: A_SOFT = (L + 8) (1.5 R + 4) u32.  rel_a = 2 max_l e_l + A_SOFT.
  AttentionResidual     out: E = (sum_l a_l |h_l|) rel_a.  save: a_l rel_a | E(d, 1 / |h_l|) | e_l | exactly 0.   out + err against the exact mix: E + u16^2 |out| (the residual
                        of one bf16 rounding, rounded once more: second order).
  push backward         ds_l = a_l (<g, h_l> - sum_k a_k <g, h_k>) has magnitude Mds_l = a_l (sum|g||h_l| + sum_k a_k sum|g||h_k|); with k1 = ds / |h_l|, k2 = k1 s_l / |h_l|
                        M = |dh0| + a_l |g| + Mds_l |w| / |h_l| + Mds_l (sum|h_l||w| / |h_l|) |h_l| / |h_l|^2,  E = 3 (d + L + 12) u32 M + 2 rel_a M   (three nested row sums).
                        dgamma / dpq: n = T L terms of magnitude Mds_l |h_l| / |h_l|, each carrying the relative error above.
  pull backward         the same terms per source j, with the saved (a, 1 / |h|, s) and <g_j, out_j + err_j> as operands: E = 3 (d + n_src + 12) u32 M, no rel_a.
  QK-norm + RoPE        r = ns qs / max(|v|, 1e-12), a = v r (1 + gamma), rotation (a cs - b sn, b cs + a sn): E(64, |a||cs| + |b||sn|).
                        backward: g = inverse rotation of dy, dyn = g c, dx = dyn / |v| - v S / |v|^3: M = |g|~ |c| / |v| + 3 |v| sum(|g|~ |c| |v|) / |v|^3 (|g|~ = |da||cs| + |db||sn|);
                        dgamma: n = T H + 1, c = 80 (each term carries the 64-term norm).
  embedding             forward: bit-exact copies; backward: n = rows of the id + 1, M = |initial| + sum|dx|.

Guard bands: every output has GUARD rows in front and behind (vectors: one row between two guard blocks) filled with the fixed pattern.  Table gradients are
prefilled with the pattern where the contract says STORED (segment mode): the columns an instance owns come back as the plain sum; pad columns [3d, ld), the other
wrapper's columns of a 6d layout and the rows of absent instances come back bit-identical.  The atomic forms start from finite random values and return value + sum.

Worst error / bound of the fp32 CPU emulation (linear order | lane layout with the 64-lane tree; tests/test_tokenwise_refs_cpu.py prints them):
  adaln_pre fwd   u 0.992 | 0.992   mean 0.004 | 0.004   rstd 0.123 | 0.123          adaln_pre bwd   dx 0.993 | 0.993   dtable 0.282 | 0.282   dgamma_text 0.042 | 0.022
  adaln_post fwd  out 0.996 | 0.996        adaln_post bwd  dy 0.995 | 0.995   dtable 0.166 | 0.166   dlayerscale 0.019 | 0.013   dbias 0.035 | 0.027
  rmsnorm         y 0.994 | 0.994   dx 0.992 | 0.992   dgamma 0.016 | 0.010
  attnres fwd     out 0.982 | 0.982   save 0.165 | 0.165   out + err 0.220 | 0.224     push bwd  dhiddens 0.958 | 0.958   dgamma, dpq < 0.001 (sums of T L signed terms
                  against the sum of their magnitudes)
  qk_norm_rope    qk 0.994 | 0.994   dqkv 0.993 | 0.993   dgamma_q 0.002 | 0.001   dgamma_k 0.005 | 0.001        embed bwd  dtable 0.086 | 0.086
The bf16 outputs sit at the rounding term, as the GEMMs' do; what the accumulation uses of its share shows on the fp32 outputs.  The MI355X figures per kernel form
are in profiles/tokenwise_bounds.txt.
"""
from types import SimpleNamespace

import numpy as np
import torch

from _gemm_cases import BF, FILL_BF16, FILL_F32, GUARD, U16, U32, _bits, assert_elementwise, assert_untouched, guarded, relerr, tol_bf16  # noqa: F401

WIDTHS = (8, 64, 512, 520, 1024, 1032, 2048)      # one active lane | NC = 1 | NC = 1 full | NC = 2 with one lane in chunk 2 | NC = 2 full | NC = 4 with two empty chunks | NC = 4 full
TOKENS = (1, 3, 130, 1001)                        # one wave | a ragged block | T % 4 == 2 | T % 4 == 1, several hundred blocks
MAX_TEXT_RUN = 9                                   # text runs of every length 1 .. 9 (packing.token_segments chops longer ones)
EPS_LN = 1e-5


def E(n, M, c=8):
    return (n + c) * U32 * M


def a_sig(z):
    return (z.abs() + 5) * U32 * torch.sigmoid(z)


def gen(*key):
    return torch.Generator(device='cpu').manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def rn(g, *s, scale=1.0, dtype=BF, device='cpu'):
    return (torch.randn(*s, generator=g) * scale).to(dtype).to(device)


# ---------------------------------------------------------------------------------------------- outputs: guarded buffers, checks
def new_out(name, rows, cols, dtype, device, ref=None, tol=None, mask=None, init=None):
    """one output of a launch: guarded buffer, the view the kernel writes, its float64 reference / bound and the mask of elements the contract writes
    (None = all).  `init`: what the view holds before the launch (accumulating outputs); None = the guard pattern."""
    buf, view = guarded(rows, cols, dtype, device, 0)
    if init is not None:
        view.copy_(init.reshape(rows, cols))
    return SimpleNamespace(name=name, buf=buf, view=view, ref=ref, tol=tol, mask=mask, before=buf.clone())


def check_out(label, o):
    """every written element within its bound, everything else (guards, unwritten elements) bit-identical; returns the worst error / bound"""
    got, ref, tol = o.view.double(), o.ref.reshape(o.view.shape), o.tol.reshape(o.view.shape)
    written = torch.zeros(o.buf.shape, dtype=torch.bool, device=o.buf.device)
    if o.mask is None:
        written[GUARD:GUARD + o.view.shape[0]] = True
    else:
        m = o.mask.reshape(o.view.shape)
        written[GUARD:GUARD + o.view.shape[0]] = m
        got, ref, tol = torch.where(m, got, torch.zeros_like(got)), torch.where(m, ref, torch.zeros_like(ref)), torch.where(m, tol, torch.ones_like(tol))
    worst = assert_elementwise(f'{label} {o.name}', got, ref, tol, tile=(4, 512))
    assert_untouched(f'{label} {o.name}', o.buf, o.before, written)
    return worst


def check_outs(label, outs, report=None):
    res = {}
    for o in outs:
        res[o.name] = check_out(label, o)
        if report is not None:
            report[o.name] = max(report.get(o.name, 0.), res[o.name])
    return res


def old_ratio(o):
    """the whole-tensor Frobenius ratio of the first-round tests (their buffers start from zeros: an element still holding the guard pattern counts as 0)"""
    got = o.view
    got = torch.where(_bits(got) == (FILL_BF16 if got.dtype == BF else FILL_F32), torch.zeros_like(got), got).double()
    ref = o.ref.reshape(got.shape)
    if o.mask is not None:
        m = o.mask.reshape(got.shape)
        got, ref = torch.where(m, got, torch.zeros_like(got)), torch.where(m, ref, torch.zeros_like(ref))
    return relerr(got, ref)


# ---------------------------------------------------------------------------------------------- token layouts
def layout(kind, T=0, balance=False, seed=0, n_seg=0):
    """tok_inst of a batch and its segments (packing.token_segments).  Kinds:
       scatter   T tokens, a third of them modality tokens of random instances at random places (per-token forms only: no segments)
       runs      T tokens: modality instance, text run, instance, ... of lengths 1, 1, 2, 2, .. 9, 9, 1, ..
       model     two sample rows: every length 1 - 9 as an instance and as a text run, one instance of 1030 tokens, long text (chopped into runs of 9)
       all_text / all_mod / one_seg     50 text tokens / 60 tokens of instances 1 - 9 long / one instance of 7 tokens
       many      n_seg segments of lengths 1 - 9 (instances and text runs alternating)
    Instance ids are a permutation of the table rows that leaves three rows unused (absent instances)."""
    from transfusion_pytorch_amd.packing import token_segments
    rs = np.random.RandomState(seed + 17)

    def alternating(total=None, count=None):
        out, k = [], 0
        while (total is None or sum(len(o) for o in out) < total) and (count is None or k < count):
            L = (k // 2) % 9 + 1
            out.append(np.full(L, k // 2 if k % 2 == 0 else -1))
            k += 1
        row = np.concatenate(out) if out else np.zeros(0, int)
        return row[:total] if total is not None else row

    if kind == 'scatter':
        tok = np.full((1, T), -1)
        idx = rs.permutation(T)[:max(T // 3, 1 if T > 1 else 0)]
        tok[0, idx] = rs.randint(0, max(1, min(37, T)), len(idx))
    elif kind == 'runs':
        tok = alternating(total=T)[None]
    elif kind == 'model':
        a = alternating(count=18)                                            # 90 tokens: instances 0 .. 8 and text runs, 1 .. 9 long each
        n = 1030 + 30
        r0 = np.full(n, -1); r0[:len(a)] = a
        r1 = np.full(n, -1); r1[7:1037] = 9
        tok = np.stack([r0, r1])
    elif kind == 'all_text':
        tok = np.full((1, 50), -1)
    elif kind == 'all_mod':
        tok = np.concatenate([np.full(k % 9 + 1, k) for k in range(12)])[None]
    elif kind == 'one_seg':
        tok = np.zeros((1, 7), int)
    elif kind == 'many':
        tok = alternating(count=n_seg)[None]
    else:
        raise KeyError(kind)
    tok = tok.astype(np.int64)
    n_inst = int(tok.max()) + 1 if tok.size and tok.max() >= 0 else 0
    I = n_inst + 3
    perm = rs.permutation(I)[:n_inst] if kind != 'scatter' else np.arange(n_inst)
    tok = np.where(tok >= 0, perm[np.clip(tok, 0, None)] if n_inst else tok, -1).astype(np.int32)
    lay = SimpleNamespace(kind=kind, tok=tok, T=tok.size, I=I, balance=balance, seg_start=None, seg_len=None, n_seg=0)
    if kind != 'scatter':
        s, ln = token_segments(tok, max_text_run=MAX_TEXT_RUN, balance=balance)
        assert int(ln.sum()) == tok.size
        lay.seg_start, lay.seg_len, lay.n_seg = s, ln, len(s)
    return lay


# ---------------------------------------------------------------------------------------------- summation orders of the fp32 emulation
def seqsum(x, dim):
    """fp32 sum along `dim`, one term after the other"""
    acc = None
    for v in x.unbind(dim):
        acc = v.clone() if acc is None else acc + v
    return acc if acc is not None else torch.zeros(x.shape[:dim] + x.shape[dim + 1:])


def treesum(x, dim):
    """fp32 sum along `dim` by halving (the xor-shuffle tree)"""
    x = x.movedim(dim, -1)
    n = x.shape[-1]
    p = 1 << max(n - 1, 0).bit_length()
    if p != n:
        x = torch.cat([x, torch.zeros(x.shape[:-1] + (p - n,), dtype=x.dtype)], -1)
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def rowsum(x, order):
    """sum over the last axis (a token row of d values) as one wave does it: `linear` = left to right; `tree` = lane c owns the 8-element chunks c, c + 64, ..
    (summed in order), then the 64-lane tree"""
    if order == 'linear':
        return seqsum(x, -1)
    d = x.shape[-1]
    nc = -(-d // 512)
    xp = torch.cat([x, torch.zeros(x.shape[:-1] + (nc * 512 - d,), dtype=x.dtype)], -1).reshape(x.shape[:-1] + (nc, 64, 8))
    lanes = seqsum(xp.movedim(-2, -3).reshape(x.shape[:-1] + (64, nc * 8)), -1)
    return treesum(lanes, -1)


def colsum(x, order):
    """sum over axis 0 (tokens)"""
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1:], dtype=x.dtype)
    return seqsum(x, 0) if order == 'linear' else treesum(x, 0)


def group_sums(vals, idx, n_groups, order):
    """out[i] = sum of vals[t] over idx[t] == i (fp32, in the given order)"""
    out = torch.zeros((n_groups,) + vals.shape[1:], dtype=vals.dtype)
    for i in torch.unique(idx).tolist():
        out[i] = colsum(vals[idx == i], order)
    return out



# ---------------------------------------------------------------------------------------------- stand-alone references (also called from tests/test_kernels_gpu.py)
def pre_fwd_ref(x, tok_inst, table, gamma_text):
    """(u, tol, mean, rstd, gamma rows, beta rows) in float64 of the AdaLN input side from its operands on any device"""
    d = x.shape[1]
    im, ii = (tok_inst >= 0)[:, None], tok_inst.clamp(min=0).long()
    X = x.double()
    mean = X.mean(-1)
    xc = X - mean[:, None]
    rstd = ((xc * xc).mean(-1) + EPS_LN) ** -0.5
    gam = torch.where(im, table[ii, :d], gamma_text[None]).double()
    bet = torch.where(im, table[ii, d:2 * d], torch.zeros((), device=x.device)).double()
    u = xc * rstd[:, None] * (1 + gam) + bet
    M = (xc.abs() + X.abs().mean(-1, keepdim=True)) * rstd[:, None] * (1 + gam).abs() + bet.abs()
    return u, tol_bf16(u, E(d, M)), mean, rstd, gam, bet


def post_fwd_ref(x, y, tok_inst, z_rows, layerscale):
    """(out, tol) of the AdaLN output side; z_rows = the [I, d] block of z logits"""
    im, ii = (tok_inst >= 0)[:, None], tok_inst.clamp(min=0).long()
    zl = z_rows[ii].double()
    sc = torch.where(im, torch.sigmoid(zl), (1 + layerscale.double())[None].expand_as(zl))
    A = torch.where(im, a_sig(zl), torch.zeros((), dtype=torch.float64, device=x.device))
    X, Y = x.double(), y.double()
    out = X + Y * sc
    return out, tol_bf16(out, E(2, X.abs() + (Y * sc).abs()) + Y.abs() * A)


def rmsnorm_ref(x, gamma, dy):
    """(y, y tol, dx, dx tol, r) of RMSNorm forward and backward"""
    d = x.shape[1]
    X, DY, G1 = x.double(), dy.double(), 1 + gamma.double()
    n2 = X.norm(dim=-1, keepdim=True)
    r = d ** 0.5 / n2.clamp_min(1e-12)
    y = X * r * G1
    # the derivative of x / max(|x|, 1e-12): the projection term exists only where the norm, not the clamp, is the denominator
    k = r ** 3 / d * (n2 > 1e-12).double()
    S, Sa = (G1 * DY * X).sum(-1, keepdim=True), (G1 * DY * X).abs().sum(-1, keepdim=True)
    dx = r * G1 * DY - X * k * S
    return y, tol_bf16(y, E(d, y.abs())), dx, tol_bf16(dx, E(d, (r * G1 * DY).abs() + 3 * X.abs() * k * Sa)), r


# ---------------------------------------------------------------------------------------------- AdaLN (input and output side of a wrapper)
def build_adaln(lay, d, device='cpu', seed=0, eps_rows=False, wrappers=1):
    """operands of tfx_adaln_pre_* and tfx_adaln_post_* over one token layout.  wrappers = 2: the 6d two-wrapper table (input side at columns [0, 3d), the
    output side's wrapper at [3d, 6d)).  eps_rows: rows 1, 5, .. are unit-variance rows scaled by 2^-8 (variance about 1.5e-5), rows 2, 6, .. constant (variance 0)."""
    g = gen(seed, d, lay.T, 1)
    T, I = lay.T, lay.I
    c = SimpleNamespace(lay=lay, T=T, d=d, I=I, device=device, ld=3 * d * wrappers + 8, post_col0=3 * d * (wrappers - 1))
    x = torch.randn(T, d, generator=g) * 2.0
    if eps_rows:
        x[1::4] *= 2.0 ** -9                                                    # unit-variance rows times 2^-8
        x[2::4] = x[2::4, :1]
    c.x = x.to(BF).to(device)
    c.table = (torch.randn(I, c.ld, generator=g) * 0.5).to(device)
    c.gamma_text = (torch.randn(d, generator=g) * 0.3).to(device)
    c.layerscale = (torch.randn(d, generator=g) * 0.3).to(device)
    c.du, c.dx0, c.add, c.y, c.g = (rn(g, T, d, device=device) for _ in range(5))
    c.tok = torch.from_numpy(lay.tok.reshape(-1).copy()).to(device)
    c.init_dgt, c.init_dls, c.init_db = ((torch.randn(d, generator=g)).to(device) for _ in range(3))
    c.init_tab = (torch.randn(I, c.ld, generator=g)).to(device)
    if lay.seg_start is not None:
        c.seg_start, c.seg_len = torch.from_numpy(lay.seg_start).to(device), torch.from_numpy(lay.seg_len).to(device)
    # ---- float64 reference, forward of the input side
    im = c.tok >= 0
    ii = c.tok.clamp(min=0).long()
    c.im, c.ii = im, ii
    c.cnt = torch.bincount(ii[im], minlength=I).double()
    c.present = c.cnt > 0
    X = c.x.double()
    c.u_ref, c.u_tol, mean, rstd, gam, bet = pre_fwd_ref(c.x, c.tok, c.table, c.gamma_text)
    c.gam, c.bet = gam, bet
    c.mean_ref, c.mean_tol = mean, E(d, X.abs().mean(-1))
    c.rstd_ref, c.rstd_tol = rstd, E(d, rstd)
    c.mean32, c.rstd32 = mean.float(), rstd.float()                             # what the backward reads
    # ---- backward of the input side
    r = c.rstd32.double()[:, None]
    xh = (X - c.mean32.double()[:, None]) * r
    DU = c.du.double()
    dxh = DU * (1 + gam)
    c1, c2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    ln = r * (dxh - c1 - xh * c2)
    Mln = r * (dxh.abs() + dxh.abs().mean(-1, keepdim=True) + xh.abs() * (dxh * xh).abs().mean(-1, keepdim=True))
    c.dx_ref = {a: c.dx0.double() + (c.add.double() if a else 0) + ln for a in (False, True)}
    c.dx_tol = {a: tol_bf16(c.dx_ref[a], E(d, c.dx0.double().abs() + (c.add.double().abs() if a else 0) + Mln)) for a in (False, True)}
    z = torch.zeros(I, d, dtype=torch.float64, device=device)
    c.sum_g, c.abs_g = z.clone().index_add_(0, ii[im], (DU * xh)[im]), z.clone().index_add_(0, ii[im], (DU * xh).abs()[im])
    c.sum_b, c.abs_b = z.clone().index_add_(0, ii[im], DU[im]), z.clone().index_add_(0, ii[im], DU.abs()[im])
    c.n_text = int((~im).sum())
    c.dgt_sum, c.dgt_abs = (DU * xh)[~im].sum(0), (DU * xh).abs()[~im].sum(0)
    # ---- output side
    post_refs(c, c.g)
    return c


def post_refs(c, g_rows):
    """float64 reference of the output side for the gradient rows `g_rows` (bf16: the operand, or the dx row the fused launch stored and re-reads)"""
    d, im, ii, device = c.d, c.im, c.ii, c.device
    zl = c.table[ii, c.post_col0 + 2 * d:c.post_col0 + 3 * d].double()
    sg = torch.sigmoid(zl)
    sc = torch.where(im[:, None], sg, (1 + c.layerscale.double())[None].expand_as(sg))
    A = torch.where(im[:, None], a_sig(zl), torch.zeros((), dtype=torch.float64, device=device))
    X, Y, G = c.x.double(), c.y.double(), g_rows.double()
    c.out_ref = X + Y * sc
    c.out_tol = tol_bf16(c.out_ref, E(2, X.abs() + (Y * sc).abs()) + Y.abs() * A)
    c.dy_ref = G * sc
    c.dy_tol = tol_bf16(c.dy_ref, E(1, c.dy_ref.abs()) + G.abs() * A)
    z = torch.zeros(c.I, d, dtype=torch.float64, device=device)
    gy = G * Y
    zi = c.table[:, c.post_col0 + 2 * d:c.post_col0 + 3 * d].double()
    si = torch.sigmoid(zi)
    sgy, agy = z.clone().index_add_(0, ii[im], gy[im]), z.clone().index_add_(0, ii[im], gy.abs()[im])
    c.dz_sum, c.dz_abs, c.dz_extra = sgy * si * (1 - si), agy * si * (1 - si), agy * a_sig(zi)
    c.dls_sum, c.dls_abs = gy[~im].sum(0), gy.abs()[~im].sum(0)
    c.db_sum, c.db_abs, c.db_extra = c.dy_ref.sum(0), c.dy_ref.abs().sum(0), (G.abs() * A).sum(0)


def _table_out(c, name, col0, ncol, ssum, sabs, extra, stored):
    """a table-gradient output: the columns [col0, col0 + ncol) of present instances hold `ssum` (stored) or initial + `ssum` (atomics); everything else untouched"""
    I, ld, device = c.I, c.ld, c.device
    ref = torch.zeros(I, ld, dtype=torch.float64, device=device)
    tol = torch.ones_like(ref)
    mask = torch.zeros(I, ld, dtype=torch.bool, device=device)
    mask[:, col0:col0 + ncol] = c.present[:, None]
    init = None if stored else c.init_tab
    base = 0 if stored else c.init_tab[:, col0:col0 + ncol].double()
    ref[:, col0:col0 + ncol] = ssum + base
    tol[:, col0:col0 + ncol] = E(c.cnt[:, None] + (0 if stored else 1), sabs + (0 if stored else c.init_tab[:, col0:col0 + ncol].double().abs())) + extra
    return new_out(name, I, ld, torch.float32, device, ref, tol, mask, init)


def outs_pre_fwd(c):
    T, d, dev = c.T, c.d, c.device
    return SimpleNamespace(u=new_out('u', T, d, BF, dev, c.u_ref, c.u_tol), mean=new_out('mean', 1, T, torch.float32, dev, c.mean_ref, c.mean_tol),
                           rstd=new_out('rstd', 1, T, torch.float32, dev, c.rstd_ref, c.rstd_tol))


def outs_pre_bwd(c, stored, use_add=False):
    """stored: the segment forms (table gradient stored into a buffer prefilled with the guard pattern); else the per-token atomics onto finite values"""
    T, d, dev = c.T, c.d, c.device
    dx = new_out('dx', T, d, BF, dev, c.dx_ref[use_add], c.dx_tol[use_add], init=c.dx0)
    dtab = _table_out(c, 'dtable[gamma|beta]', 0, 2 * d, torch.cat([c.sum_g, c.sum_b], 1), torch.cat([c.abs_g, c.abs_b], 1), 0., stored)
    dgt = new_out('dgamma_text', 1, d, torch.float32, dev, c.init_dgt.double() + c.dgt_sum, E(c.n_text + 1, c.init_dgt.double().abs() + c.dgt_abs), init=c.init_dgt)
    return SimpleNamespace(dx=dx, dtable=dtab, dgamma_text=dgt)


def outs_post_fwd(c):
    return SimpleNamespace(out=new_out('out', c.T, c.d, BF, c.device, c.out_ref, c.out_tol))


def outs_post_bwd(c, stored):
    T, d, dev = c.T, c.d, c.device
    o = SimpleNamespace(dy=new_out('dy', T, d, BF, dev), dtable=_table_out(c, 'dtable[z]', c.post_col0 + 2 * d, d, c.dz_sum, c.dz_abs, c.dz_extra, stored),
                        dlayerscale=new_out('dlayerscale', 1, d, torch.float32, dev, init=c.init_dls), dbias=new_out('dbias', 1, d, torch.float32, dev, init=c.init_db))
    return refill_post_bwd(c, o, stored)


def refill_post_bwd(c, o, stored, g_rows=None):
    """(re)compute the references of the output side's backward - with g_rows = the bf16 gradient rows a fused launch stored and re-read (post_refs)"""
    if g_rows is not None:
        post_refs(c, g_rows)
    T, d = c.T, c.d
    o.dy.ref, o.dy.tol = c.dy_ref, c.dy_tol
    t = _table_out(c, 'dtable[z]', c.post_col0 + 2 * d, d, c.dz_sum, c.dz_abs, c.dz_extra, stored)
    o.dtable.ref, o.dtable.tol, o.dtable.mask = t.ref, t.tol, t.mask
    o.dlayerscale.ref, o.dlayerscale.tol = c.init_dls.double() + c.dls_sum, E(c.n_text + 1, c.init_dls.double().abs() + c.dls_abs)
    o.dbias.ref, o.dbias.tol = c.init_db.double() + c.db_sum, E(T + 1, c.init_db.double().abs() + c.db_abs) + c.db_extra
    return o


def merge_tables(a, b):
    """one buffer for two table-gradient outputs with disjoint column masks (the 6d layout of the fused launch): returns the merged output, built on a's buffer"""
    ref, tol = torch.where(b.mask, b.ref, a.ref), torch.where(b.mask, b.tol, a.tol)
    return SimpleNamespace(name='dtable[gamma|beta|..|z]', buf=a.buf, view=a.view, ref=ref, tol=tol, mask=a.mask | b.mask, before=a.before)


PRE_FAULTS = ('last_token_unwritten', 'row_stats_from_neighbour', 'last_chunk_out_of_stats', 'double_round', 'eps_dropped', 'beta_on_text_row')


def emulate_pre_fwd(c, o, order, fault=None):
    d, T = c.d, c.T
    x = c.x.float()
    xs = x
    if fault == 'last_chunk_out_of_stats':                  # the lanes of the last (partly filled) 512-column chunk stay out of both reductions
        xs = x.clone(); xs[:, (d - 1) // 512 * 512:] = 0
    mean = rowsum(xs, order) / d
    dv = x - mean[:, None]
    dvs = dv
    if fault == 'last_chunk_out_of_stats':
        dvs = dv.clone(); dvs[:, (d - 1) // 512 * 512:] = 0
    var = rowsum(dvs * dvs, order) / d
    rstd = torch.rsqrt(var if fault == 'eps_dropped' else var + 1e-5)
    o.mean.view[0] = mean; o.rstd.view[0] = rstd
    if fault == 'row_stats_from_neighbour' and T > 1:
        rstd = rstd.clone(); rstd[T // 2] = rstd[T // 2 - 1]
    xh = dv * rstd[:, None]
    if fault == 'double_round':
        xh = xh.to(BF).float()
    gam = torch.where(c.im[:, None], c.table[c.ii, :d], c.gamma_text[None])
    bet = torch.where(c.im[:, None], c.table[c.ii, d:2 * d], torch.zeros(()))
    if fault == 'beta_on_text_row':
        bet = c.table[c.ii, d:2 * d]
    u = xh * (1 + gam) + bet
    n = T - 1 if fault == 'last_token_unwritten' else T
    o.u.view[:n] = u[:n].to(BF)


def emulate_pre_bwd(c, o, order, stored, use_add=False, fault=None):
    """per-token form (stored = False: atomics onto the initial values) or segment form (stored = True).  Faults: segment_tail_token_twice (the tail token of a
    segment whose length is no multiple of U = 4 enters the table sums twice), segment_added_not_stored, table_pad_written, second_trip_skipped (the tokens a
    capped grid reaches only on its second trip - here: from token 4096 on - are never processed)."""
    d, T = c.d, c.T
    n = min(T, 4096) if fault == 'second_trip_skipped' else T
    x, du = c.x.float(), c.du.float()
    mean, rstd = c.mean32[:, None], c.rstd32[:, None]
    gam = torch.where(c.im[:, None], c.table[c.ii, :d], c.gamma_text[None])
    xh = (x - mean) * rstd
    dg = du * xh
    dxh = du * (1 + gam)
    c1 = rowsum(dxh, order)[:, None] / d
    c2 = rowsum(dxh * xh, order)[:, None] / d
    dx = c.dx0.float() + (c.add.float() if use_add else 0) + rstd * (dxh - c1 - xh * c2)
    o.dx.view[:n] = dx[:n].to(BF)
    live = torch.zeros(T, dtype=torch.bool); live[:n] = True
    sel = c.im & live
    wt = torch.ones(T)
    if fault == 'segment_tail_token_twice':
        for s, ln in zip(c.lay.seg_start.tolist(), c.lay.seg_len.tolist()):
            if ln % 4:
                wt[s + ln - 1] = 2
    sg = group_sums((dg * wt[:, None])[sel], c.ii[sel], c.I, order)
    sb = group_sums((du * wt[:, None])[sel], c.ii[sel], c.I, order)
    new = torch.cat([sg, sb], 1)[c.present]
    tv = o.dtable.view
    if stored and fault != 'segment_added_not_stored':
        tv[c.present, :2 * d] = new
    else:
        tv[c.present, :2 * d] += new
    if fault == 'table_pad_written':
        tv[c.present, 3 * d:] = 0
    o.dgamma_text.view[0] += colsum(dg[~c.im & live], order)


def emulate_post_fwd(c, o, order):
    d = c.d
    z = c.table[c.ii, c.post_col0 + 2 * d:c.post_col0 + 3 * d]
    sc = torch.where(c.im[:, None], torch.sigmoid(z), 1 + c.layerscale[None])
    o.out.view[:] = (c.x.float() + c.y.float() * sc).to(BF)


def emulate_post_bwd(c, o, order, stored, g_rows=None, fault=None):
    d, T = c.d, c.T
    n = min(T, 4096) if fault == 'second_trip_skipped' else T
    live = torch.zeros(T, dtype=torch.bool); live[:n] = True
    z = c.table[c.ii, c.post_col0 + 2 * d:c.post_col0 + 3 * d]
    sc = torch.where(c.im[:, None], torch.sigmoid(z), 1 + c.layerscale[None])
    g, y = (c.g if g_rows is None else g_rows).float(), c.y.float()
    gy = g * y
    dy = g * sc
    o.dy.view[:n] = dy[:n].to(BF)
    sel = c.im & live
    col = slice(c.post_col0 + 2 * d, c.post_col0 + 3 * d)
    si = torch.sigmoid(c.table[:, col])
    if stored:
        new = group_sums(gy[sel], c.ii[sel], c.I, order) * si * (1 - si)
        o.dtable.view[:, col][c.present] = new[c.present]
    else:
        new = group_sums((gy * sc * (1 - sc))[sel], c.ii[sel], c.I, order)
        o.dtable.view[:, col][c.present] += new[c.present]
    o.dlayerscale.view[0] += colsum(gy[~c.im & live], order)
    o.dbias.view[0] += colsum(dy[live], order)


# ---------------------------------------------------------------------------------------------- RMSNorm
def build_rmsnorm(T, d, device='cpu', seed=0, zero_row=False):
    g = gen(seed, d, T, 2)
    c = SimpleNamespace(T=T, d=d, device=device)
    x = torch.randn(T, d, generator=g) * 3.0
    if zero_row:
        x[T // 2] = 0
    c.x = x.to(BF).to(device)
    c.gamma = (torch.randn(d, generator=g) * 0.3).to(device)
    c.dy = rn(g, T, d, device=device)
    c.init_dg = torch.randn(d, generator=g).to(device)
    X, DY = c.x.double(), c.dy.double()
    c.y_ref, c.y_tol, c.dx_ref, c.dx_tol, r = rmsnorm_ref(c.x, c.gamma, c.dy)
    c.dg_ref = c.init_dg.double() + (DY * X * r).sum(0)
    c.dg_tol = E(T + 1, c.init_dg.double().abs() + (DY * X * r).abs().sum(0)) + E(d, (DY * X * r).abs().sum(0))
    return c


def outs_rmsnorm(c):
    T, d, dev = c.T, c.d, c.device
    return SimpleNamespace(y=new_out('y', T, d, BF, dev, c.y_ref, c.y_tol), dx=new_out('dx', T, d, BF, dev, c.dx_ref, c.dx_tol),
                           dgamma=new_out('dgamma', 1, d, torch.float32, dev, c.dg_ref, c.dg_tol, init=c.init_dg))


def emulate_rmsnorm(c, o, order, fault=None):
    d, T = c.d, c.T
    n = min(T, 4096) if fault == 'second_trip_skipped' else T
    x, dy, g1 = c.x.float(), c.dy.float(), 1 + c.gamma
    q = rowsum(x * x, order)[:, None]
    r = d ** 0.5 / torch.sqrt(q).clamp_min(1e-12)
    o.y.view[:] = (x * (r * g1)).to(BF)
    S = rowsum(g1 * dy * x, order)[:, None]
    k2 = torch.where(torch.sqrt(q) > 1e-12, r * r * r / d * S, torch.zeros(()))
    o.dx.view[:n] = (r * g1 * dy - x * k2)[:n].to(BF)
    o.dgamma.view[0] += colsum((dy * x * r)[:n], order)


# ---------------------------------------------------------------------------------------------- AttentionResidual
def attnres_state(Hd, gamma, pq):
    """float64 depth softmax of hiddens Hd [L, T, d]: scores, inverse norms, weights, the mix, and the error terms of the docstring"""
    L, T, d = Hd.shape
    w = (1 + gamma.double()) * pq.double()
    nrm = Hd.norm(dim=-1).clamp_min(1e-12)                       # [L, T]
    s = (Hd @ w) / nrm
    SW = (Hd.abs() @ w.abs()) / nrm
    es = E(d, SW)
    a = torch.softmax(s, 0)
    R = s.max(0).values - s.min(0).values
    rel_a = 2 * es.max(0).values + (L + 8) * (1.5 * R + 4) * U32       # [T]
    out = torch.einsum('lt,ltd->td', a, Hd)
    mix = torch.einsum('lt,ltd->td', a, Hd.abs())
    return SimpleNamespace(w=w, nrm=nrm, inv=1 / nrm, s=s, SW=SW, es=es, a=a, rel_a=rel_a, out=out, E_out=mix * rel_a[:, None])


def build_attnres(T, d, L, device='cpu', seed=0, zero_row=False):
    g = gen(seed, d, T, L, 3)
    c = SimpleNamespace(T=T, d=d, L=L, device=device)
    H = torch.randn(L, T, d, generator=g) * 2.0
    if zero_row:
        H[L // 2, T // 2] = 0
    c.H = H.to(BF).to(device)
    c.gamma = (torch.randn(d, generator=g) * 0.3).to(device)
    c.pq = (torch.randn(d, generator=g) * 0.5 * (64 / d) ** 0.5).to(device)        # scores of a few units at every width
    c.g, c.g2 = rn(g, T, d, device=device), rn(g, T, d, device=device)
    c.dH0 = rn(g, L, T, d, device=device)
    c.init_dg, c.init_dpq = torch.randn(d, generator=g).to(device), torch.randn(d, generator=g).to(device)
    Hd = c.H.double()
    st = attnres_state(Hd, c.gamma, c.pq)
    c.st = st
    c.out_ref, c.out_tol = st.out, tol_bf16(st.out, st.E_out)
    c.sum_tol = st.E_out + U16 * U16 * st.out.abs()
    save = torch.stack([st.a, st.inv, st.s, torch.zeros_like(st.s)], -1).permute(1, 0, 2)      # [T, L, 4]
    stol = torch.stack([st.a * st.rel_a[None], E(d, st.inv), st.es, torch.zeros_like(st.s)], -1).permute(1, 0, 2)
    c.save_ref, c.save_tol = save.reshape(T, L * 4), stol.reshape(T, L * 4)
    # ---- push backward, with and without the second addend / the accumulate
    c.bwd = {}
    for first, use_g2 in ((0, True), (1, False)):
        G = c.g.double() + (c.g2.double() if use_g2 else 0)
        da = torch.einsum('ltd,td->lt', Hd, G)
        AD = torch.einsum('ltd,td->lt', Hd.abs(), G.abs())
        dsum, DA = (st.a * da).sum(0), (st.a * AD).sum(0)
        ds = st.a * (da - dsum[None])
        Mds = st.a * (AD + DA[None])
        k1, k2 = ds * st.inv, ds * st.s * st.inv ** 2
        v = st.a[..., None] * G[None] + k1[..., None] * st.w - k2[..., None] * Hd
        M = st.a[..., None] * G.abs()[None] + (Mds * st.inv)[..., None] * st.w.abs() + (Mds * st.SW * st.inv ** 2)[..., None] * Hd.abs()
        base = 0 if first else c.dH0.double()
        ref = base + v
        rel = 3 * (d + L + 12) * U32 + 2 * st.rel_a[None, :, None]
        tol = tol_bf16(ref, (M + (0 if first else c.dH0.double().abs())) * rel)
        dw = torch.einsum('lt,ltd->d', k1, Hd)
        Mw = (Mds * st.inv)[..., None] * Hd.abs()
        Ew = E(T * L, Mw.sum((0, 1))) + (Mw * rel).sum((0, 1))
        res = SimpleNamespace(dh_ref=ref.reshape(L * T, d), dh_tol=tol.reshape(L * T, d))
        for nm, f, init in (('dgamma', c.pq.double(), c.init_dg), ('dpq', 1 + c.gamma.double(), c.init_dpq)):
            setattr(res, nm + '_ref', init.double() + dw * f)
            setattr(res, nm + '_tol', Ew * f.abs() + E(2, init.double().abs() + (dw * f).abs()))
        c.bwd[first] = res
    return c


def outs_attnres_fwd(c):
    T, d, L, dev = c.T, c.d, c.L, c.device
    return SimpleNamespace(out=new_out('out', T, d, BF, dev, c.out_ref, c.out_tol), save=new_out('save', T, L * 4, torch.float32, dev, c.save_ref, c.save_tol),
                           err=new_out('err', T, d, BF, dev, torch.zeros(T, d, dtype=torch.float64, device=dev), torch.full((T, d), float('inf'), dtype=torch.float64, device=dev)))


def check_attnres_fwd(label, c, o, report=None):
    """out and save per element; `err` only through out + err (its own value is whatever the rounding dropped: finite, guards intact)"""
    res = check_outs(label, [o.out, o.save, o.err], report)
    del res['err']
    if report is not None:
        report.pop('err', None)
    tot = o.out.view.double() + o.err.view.double()
    res['out+err'] = assert_elementwise(f'{label} out + err', tot, c.out_ref, c.sum_tol, tile=(4, 512))
    if report is not None:
        report['out+err'] = max(report.get('out+err', 0.), res['out+err'])
    return res


def outs_attnres_bwd(c, first):
    T, d, L, dev = c.T, c.d, c.L, c.device
    b = c.bwd[first]
    return SimpleNamespace(dhiddens=new_out('dhiddens', L * T, d, BF, dev, b.dh_ref, b.dh_tol, init=None if first else c.dH0),
                           dgamma=new_out('dgamma', 1, d, torch.float32, dev, b.dgamma_ref, b.dgamma_tol, init=c.init_dg),
                           dpq=new_out('dpq', 1, d, torch.float32, dev, b.dpq_ref, b.dpq_tol, init=c.init_dpq))


def emulate_attnres_fwd(c, o, order, fault=None):
    """the online form of attnres_mix.  Fault save_lane_ge_32_dropped: the saved state of hiddens 32 .. L - 1 is never written."""
    T, d, L = c.T, c.d, c.L
    w = (1 + c.gamma) * c.pq
    acc = torch.zeros(T, d)
    m = torch.full((T,), -float('inf')); den = torch.zeros(T)
    ss, invs = [], []
    for l in range(L):
        h = c.H[l].float()
        nrm = torch.sqrt(rowsum(h * h, order)).clamp_min(1e-12)
        s = rowsum(h * w, order) / nrm
        ss.append(s); invs.append(1 / nrm)
        mn = torch.maximum(m, s)
        al, ex = torch.exp(m - mn), torch.exp(s - mn)
        den = den * al + ex
        acc = acc * al[:, None] + ex[:, None] * h
        m = mn
    s, inv = torch.stack(ss, 1), torch.stack(invs, 1)                       # [T, L]
    save = torch.stack([torch.exp(s - m[:, None]) / den[:, None], inv, s, torch.zeros_like(s)], -1)
    nl = min(L, 32) if fault == 'save_lane_ge_32_dropped' else L
    o.save.view.reshape(T, L, 4)[:, :nl] = save[:, :nl]
    ex = acc * (1 / den)[:, None]
    o.out.view[:] = ex.to(BF)
    o.err.view[:] = (ex - ex.to(BF).float()).to(BF)


def emulate_attnres_bwd(c, o, order, first, fault=None):
    T, d, L = c.T, c.d, c.L
    n = min(T, 4096) if fault == 'second_trip_skipped' else T
    w = (1 + c.gamma) * c.pq
    G = c.g.float() + (0 if first else c.g2.float())
    H = c.H.float()
    nsq = torch.stack([rowsum(H[l] * H[l], order) for l in range(L)])
    dt = torch.stack([rowsum(H[l] * w, order) for l in range(L)])
    da = torch.stack([rowsum(H[l] * G, order) for l in range(L)])
    inv = 1 / torch.sqrt(nsq).clamp_min(1e-12)
    s = dt * inv
    ex = torch.exp(s - s.max(0).values[None])
    a = ex / (seqsum(ex, 0) if order == 'linear' else treesum(ex, 0))[None]
    dsum = seqsum(a * da, 0) if order == 'linear' else treesum(a * da, 0)
    ds = a * (da - dsum[None])
    k1, k2 = ds * inv, ds * s * inv * inv
    v = a[..., None] * G[None] + k1[..., None] * w - k2[..., None] * H
    dh = v if first else c.dH0.float() + v
    o.dhiddens.view.reshape(L, T, d)[:, :n] = dh[:, :n].to(BF)
    pw = colsum((k1[..., None] * H)[:, :n].reshape(-1, d), order)
    o.dgamma.view[0] += pw * c.pq
    o.dpq.view[0] += pw * (1 + c.gamma)


def pull_ref(h, gs, saves, l, outs_own, ws, add=None):
    """float64 reference and bound of one tfx_attnres_pull_bwd row block: h [T, d] (hidden l), gs[j] [T, d] bf16, saves[j] [T, L_j, 4] fp32 (the saved state
    the kernel reads: operands), outs_own[j] [T, d] float64 = the forward output of source j as stored (out + err), ws[j] [d] fp32, add [T, d] or None"""
    Hd = h.double()
    d = Hd.shape[1]
    ref = add.double().clone() if add is not None else torch.zeros_like(Hd)
    M = ref.abs()
    T = Hd.shape[0]
    rel = 3 * (d + len(gs) + 12) * U32
    dws, dw_tols = [], []
    for g, sv, o, w in zip(gs, saves, outs_own, ws):
        G, W = g.double(), w.double()
        a, inv, s = (sv[:, l, k].double() for k in range(3))
        da, AD = (G * Hd).sum(-1), (G.abs() * Hd.abs()).sum(-1)
        dsum, DS = (G * o).sum(-1), (G.abs() * o.abs()).sum(-1)
        ds, Mds = a * (da - dsum), a * (AD + DS)
        k1 = ds * inv
        ref = ref + a[:, None] * G + k1[:, None] * W - (k1 * s * inv)[:, None] * Hd
        M = M + a[:, None] * G.abs() + (Mds * inv)[:, None] * W.abs() + (Mds * s.abs() * inv * inv)[:, None] * Hd.abs()
        Mw = ((Mds * inv)[:, None] * Hd.abs()).sum(0)
        dws.append((k1[:, None] * Hd).sum(0)); dw_tols.append(E(T, Mw) + rel * Mw)
    return ref, tol_bf16(ref, rel * M), dws, dw_tols


# ---------------------------------------------------------------------------------------------- QK-norm + RoPE
def build_qk(T, H, device='cpu', seed=0):
    g = gen(seed, T, H, 4)
    HD = 64 * H
    c = SimpleNamespace(T=T, H=H, HD=HD, device=device, ld=3 * HD + 8, ld_qk=2 * HD + 8, q_scale=0.125)
    c.qkv = rn(g, T, c.ld, scale=1.5, device=device)
    c.gq, c.gk = (torch.randn(64, generator=g) * 0.3).to(device), (torch.randn(64, generator=g) * 0.3).to(device)
    c.pos = torch.randint(0, 900, (T,), generator=g).to(torch.int32).to(device)
    freqs = 1. / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(1024).float()[:, None] * freqs[None]
    c.cos, c.sin = ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)
    c.dqk = rn(g, T, 2 * HD, device=device)
    c.init_dgq, c.init_dgk = torch.randn(64, generator=g).to(device), torch.randn(64, generator=g).to(device)
    for k, v in vars(qk_refs(c, c.pos)).items():
        setattr(c, k, v)
    return c


def qk_refs(c, pos):
    T, H, dev = c.T, c.H, c.device
    V = c.qkv[:, :2 * c.HD].double().reshape(T, 2 * H, 64)
    gam = torch.cat([c.gq.double()[None].expand(H, 64), c.gk.double()[None].expand(H, 64)])[None]      # [1, 2H, 64]
    qs = torch.cat([torch.full((H,), c.q_scale), torch.ones(H)]).double().to(dev)[None, :, None]
    cs, sn = c.cos[pos.long()].double()[:, None], c.sin[pos.long()].double()[:, None]                  # [T, 1, 32]
    nrm = V.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    inv = 1 / nrm
    a = V * (8.0 * qs * inv) * (1 + gam)
    ae, ao = a[..., 0::2], a[..., 1::2]
    y = torch.stack([ae * cs - ao * sn, ao * cs + ae * sn], -1).reshape(T, 2 * H, 64)
    My = torch.stack([ae.abs() * cs.abs() + ao.abs() * sn.abs(), ao.abs() * cs.abs() + ae.abs() * sn.abs()], -1).reshape(T, 2 * H, 64)
    r = SimpleNamespace(qk_ref=y.reshape(T, -1), qk_tol=tol_bf16(y, E(64, My)).reshape(T, -1))
    DY = c.dqk.double().reshape(T, 2 * H, 64)
    da, db = DY[..., 0::2], DY[..., 1::2]
    gg = torch.stack([da * cs + db * sn, db * cs - da * sn], -1).reshape(T, 2 * H, 64)
    gm = torch.stack([da.abs() * cs.abs() + db.abs() * sn.abs(), db.abs() * cs.abs() + da.abs() * sn.abs()], -1).reshape(T, 2 * H, 64)
    sc = 8.0 * qs
    cc = sc * (1 + gam)
    dyn, dynm = gg * cc, gm * cc.abs()
    S, Sa = (dyn * V).sum(-1, keepdim=True), (dynm * V.abs()).sum(-1, keepdim=True)
    dx = dyn * inv - V * S * inv ** 3
    Mx = dynm * inv + 3 * V.abs() * Sa * inv ** 3
    r.dqkv_ref, r.dqkv_tol = dx.reshape(T, -1), tol_bf16(dx, E(64, Mx)).reshape(T, -1)
    term, terma = gg * V * inv * sc, gm * V.abs() * inv * sc
    for nm, sl, init in (('dgq', slice(0, H), c.init_dgq), ('dgk', slice(H, 2 * H), c.init_dgk)):
        setattr(r, nm + '_ref', init.double() + term[:, sl].sum((0, 1)))
        setattr(r, nm + '_tol', E(T * H + 1, init.double().abs() + terma[:, sl].sum((0, 1)), c=80))
    return r


def outs_qk(c):
    T, HD, dev = c.T, c.HD, c.device

    def padded_rows(name, ref, tol):
        o = new_out(name, T, 2 * HD + 8, BF, dev)
        z, one = torch.zeros(T, 8, dtype=torch.float64, device=dev), torch.ones(T, 8, dtype=torch.float64, device=dev)
        o.ref, o.tol = torch.cat([ref, z], 1), torch.cat([tol, one], 1)
        o.mask = torch.zeros(T, 2 * HD + 8, dtype=torch.bool, device=dev); o.mask[:, :2 * HD] = True
        return o
    return SimpleNamespace(qk=padded_rows('qk', c.qk_ref, c.qk_tol), dqkv=padded_rows('dqkv', c.dqkv_ref, c.dqkv_tol),
                           dgamma_q=new_out('dgamma_q', 1, 64, torch.float32, dev, c.dgq_ref, c.dgq_tol, init=c.init_dgq),
                           dgamma_k=new_out('dgamma_k', 1, 64, torch.float32, dev, c.dgk_ref, c.dgk_tol, init=c.init_dgk))


QK_STRIDE = 32768          # vectors per trip of the capped backward grid: 256 blocks of 1024 threads, 8 threads per vector


def rope_carries(T, H):
    """does the incremental (t, rem) update of the backward's grid-stride loop take its carry at this shape (a second trip, 32768 % 2H != 0)"""
    return T * 2 * H > QK_STRIDE and QK_STRIDE % (2 * H) != 0


def emulate_qk(c, o, order, fault=None):
    """Fault rope_carry_off_by_one (`rem > 2H` for `rem >= 2H`): a vector of a later trip whose `rem` reaches 2H exactly is not carried to the next token - the
    kernel then works on columns [2H 64, ..) of the row before (the v block), so vector (t, 0) is never written, nor does it reach the gain gradients."""
    T, H, HD = c.T, c.H, c.HD
    V = c.qkv[:, :2 * HD].float().reshape(T, 2 * H, 64)
    gam = torch.cat([c.gq[None].expand(H, 64), c.gk[None].expand(H, 64)])[None]
    qs = torch.cat([torch.full((H,), c.q_scale), torch.ones(H)])[None, :, None]
    live = torch.ones(T, 2 * H, dtype=torch.bool)
    if fault == 'rope_carry_off_by_one':
        vid = torch.arange(T * 2 * H).reshape(T, 2 * H)
        live = ~((vid >= QK_STRIDE) & (((vid - QK_STRIDE) % (2 * H)) + QK_STRIDE % (2 * H) == 2 * H))
    cs, sn = c.cos[c.pos.long()][:, None], c.sin[c.pos.long()][:, None]       # [T, 1, 32]
    q = (rowsum(V.reshape(-1, 64) * V.reshape(-1, 64), order)).reshape(T, 2 * H, 1)
    nrm = torch.sqrt(q).clamp_min(1e-12)
    inv = 1 / nrm
    a = V * (8.0 / nrm * qs) * (1 + gam)
    ae, ao = a[..., 0::2], a[..., 1::2]
    y = torch.stack([ae * cs - ao * sn, ao * cs + ae * sn], -1).reshape(T, -1)
    o.qk.view[:, :2 * HD] = y.to(BF)
    DY = c.dqk.float().reshape(T, 2 * H, 64)
    da, db = DY[..., 0::2], DY[..., 1::2]
    gg = torch.stack([da * cs + db * sn, db * cs - da * sn], -1).reshape(T, 2 * H, 64)
    sc = 8.0 * qs
    dyn = gg * (sc * (1 + gam))
    S = rowsum((dyn * V).reshape(-1, 64), order).reshape(T, 2 * H, 1)
    k = S * inv * inv * inv
    dx = (dyn * inv - V * k).to(BF)
    keep = o.dqkv.view[:, :2 * HD].reshape(T, 2 * H, 64).clone()
    o.dqkv.view[:, :2 * HD] = torch.where(live[..., None], dx, keep).reshape(T, -1)
    term = gg * V * (inv * sc) * live[..., None]
    o.dgamma_q.view[0] += colsum(term[:, :H].reshape(-1, 64), order)
    o.dgamma_k.view[0] += colsum(term[:, H:].reshape(-1, 64), order)


# ---------------------------------------------------------------------------------------------- embedding
def build_embed(lay, d, V, device='cpu', seed=0):
    g = gen(seed, d, lay.T, 5)
    T = lay.T
    c = SimpleNamespace(T=T, d=d, V=V, device=device, lay=lay)
    c.tok = torch.from_numpy(lay.tok.reshape(-1).copy()).to(device)
    ids = torch.randint(0, max(V // 2, 1), (T,), generator=g) * 2                 # even ids only, repeated: the odd rows of the table are unused
    c.ids = torch.where(c.tok.cpu() >= 0, torch.full((T,), -1), ids).to(torch.int32).to(device)
    c.table = rn(g, V, d, device=device)
    c.dx = rn(g, T, d, device=device)
    c.x0 = rn(g, T, d, device=device)
    c.init = torch.randn(V, d, generator=g).to(device)
    text = c.tok < 0
    idl = c.ids.clamp(min=0).long()
    c.text = text
    c.x_mask = text[:, None].expand(T, d)
    c.x_ref = torch.where(c.x_mask, c.table[idl].double(), c.x0.double())
    z = torch.zeros(V, d, dtype=torch.float64, device=device)
    s, sa = z.clone().index_add_(0, idl[text], c.dx.double()[text]), z.clone().index_add_(0, idl[text], c.dx.double().abs()[text])
    cnt = torch.bincount(idl[text], minlength=V).double()
    c.used = cnt > 0
    c.dt_ref, c.dt_tol = c.init.double() + s, E(cnt[:, None] + 1, c.init.double().abs() + sa)
    return c


def outs_embed(c):
    T, d, V, dev = c.T, c.d, c.V, c.device
    return SimpleNamespace(x=new_out('x', T, d, BF, dev, c.x_ref, torch.zeros(T, d, dtype=torch.float64, device=dev), mask=c.x_mask, init=c.x0),
                           dtable=new_out('dtable', V, d, torch.float32, dev, c.dt_ref, c.dt_tol, mask=c.used[:, None].expand(V, d), init=c.init))


def emulate_embed(c, o, order):
    idl = c.ids.clamp(min=0).long()
    o.x.view[c.text] = c.table[idl[c.text]]
    o.dtable.view[:] += group_sums(c.dx.float()[c.text], idl[c.text], c.V, order)


FAULTS = PRE_FAULTS + ('segment_tail_token_twice', 'segment_added_not_stored', 'second_trip_skipped', 'table_pad_written', 'rope_carry_off_by_one',
                       'save_lane_ge_32_dropped')
