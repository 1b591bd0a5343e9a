"""Mask layout catalogue of the attention tests (not collected: no test_ prefix; imports no GPU code at module level).

A case is a batch of samples of `n` tokens; each sample lists its modality blocks as (offset, length).  layout_maps() applies the packing rule of
packing.token_maps: a block's rows see the whole block (kv_end = hi, q_start = lo), blocks are clipped at n, every other row is causal.

build_inputs() makes raw q / k (pre QK-RMSNorm), v, gate logits and dout with SENTINELS in the even heads: for every edge of the layout (the rows
that share one kv_end = e: a block, the causal row in front of a block, a row on a 64-key boundary, ...) the last two visible keys e - 2, e - 1
and the first masked key e are aligned with those rows' queries: the three scores tie near the soft-cap plan's bound, and the keys carry large,
distinct values.  The rows' weight splits over the visible sentinels (so dS = P (dP - delta) does not cancel), and one key more or less moves
their output and gradients by O(1), far above the per-row tolerances below - which the CPU mutation test (tests/test_attention_layouts_cpu.py)
proves with the same builder and the same tolerances.  The odd heads stay random.

The tolerances below are MEASURED on the kernels; the derived per-element bounds are in tests/_attn_bounds.py (tests/test_attention_softcap_gpu.py): out, lse,
do_eff, delta, dgate, dq, dk and dv of the plain and the LASER path now have both, the fused QK-norm backward's raw d q | d k and gain gradients only these.
"""
import math
from typing import NamedTuple

import torch

CAP = 50.                        # the model's attention soft-cap
LASER_C = 15.                    # laser_softclamp_value
SENT_COLS = (1, 5, 9, 13, 17, 21, 25, 29)   # sentinel directions (inside the first 32 columns: dim_head 32 heads too)
SENT_Q, SENT_K, SENT_V = 4., 4., 3.          # sentinel scores reach 0.89 of the bound B
BASE_QK = 8.                                 # the shared direction of the other rows / keys of a sentinel head (about half the bound)
# the edge rows' dout lies along a direction of their group, SENT_DO long; key j's value carries VCOEF[j % 3] x SENT_W along it: any three
# consecutive keys have distinct offsets, so dP = do_eff . v differs between e - 2, e - 1 and e by >= SENT_DO SENT_W sigmoid(gate) whatever the
# random parts do - dS of the edge rows cannot cancel by chance
SENT_DO, SENT_W, VCOEF = 8., 6., (1., -1., 2.)
B_OVER_CAP = {0: 0.17, 1: 0.30, None: 0.40}  # B / cap of the gains for plan mode 0 / 1 (tfx.h: <= 0.2 / <= 0.35) and mode 2 (no plan passed)

# Per-row metrics: a row's error is normalised by max(its own norm, ROW_FLOOR x the RMS row norm of its (sample, head)); lse is absolute (nats).
# The GPU sweep asserts these against exact_input_reference() in every head (worst values measured on the MI355X over the catalogue in brackets;
# lse / out also bound the KV-cache tests: 3.2e-4 / 4.6e-3 there).  The CPU mutation test asserts that one key more or less on an edge's rows
# exceeds the out / dq / dk / dv tolerances of every path MUTATION_MARGIN times over (smallest margins: dk 5.5 plain, dv 5.9 LASER, dq 6.5 LASER).
ROW_FLOOR = 0.1
ROW_TOL = {'out': 1e-2, 'lse': 1e-3, 'dq': 3e-2, 'dk': 1.2e-2, 'dv': 6e-3, 'do_eff': 4e-3, 'delta': 1e-5, 'dgate': 6e-3}
#          [6.0e-3,     7.8e-5,      2.3e-2,     8.3e-3,       4.3e-3,     2.8e-3,          3.8e-6,         3.9e-3]
ROW_TOL_LASER = {'out': 1e-2, 'lse': 1e-3, 'dq': 2e-2, 'dk': 8e-3, 'dv': 1.3e-2, 'do_eff': 5e-3, 'delta': 1e-5, 'dgate': 6e-3}
#                [5.0e-3,     5.5e-5,      1.5e-2,     5.6e-3,     9.4e-3,       3.4e-3,          2.0e-7,         3.9e-3]
ROW_TOL_NR = {'dq': 1.1e-2, 'dk': 9e-3, 'dgq': 4e-2, 'dgk': 5e-3}   # d q | d k raw [7.9e-3, 6.2e-3]; gain gradients (gain_err) [2.9e-2, < 5e-3]
MUTATION_MARGIN = 5.


def row_tol(laser=False, nr=False):
    """per-row tolerances of one path of the sweep"""
    t = dict(ROW_TOL_LASER if laser else ROW_TOL)
    if nr:
        t.update(ROW_TOL_NR)
    return t


class Case(NamedTuple):
    name: str
    h: int
    n: int
    samples: tuple               # per sample: tuple of (offset, length) blocks
    dh: int = 64                 # dim_head; 32 = the kernel layout of params.py hdk (upper 32 columns of every head zero)
    sub: bool = False            # in the subset of the LASER / fused QK-norm backward / bit-identity runs

    @property
    def b(self):
        return len(self.samples)


CATALOGUE = [
    Case('n1', 2, 1, ((), ((0, 1),))),                                            # one row: pure causal, a single-token block
    Case('n5', 2, 5, (((0, 5),), ((1, 1), (2, 2)), ((3, 9),))),                  # whole sample one block; single-token + back-to-back; clipped
    Case('n33', 2, 33, (((20, 49),), ((0, 7), (7, 7), (30, 3)))),               # clipped, not the last sample; row 0, back-to-back, ends at n
    Case('n63', 2, 63, (((5, 49),), ())),                                         # 49 at an odd offset; pure causal
    Case('n65', 2, 65, (((1, 64),), ((0, 1), (64, 1))), sub=True),               # ends exactly at n, not the last sample; tokens at 0 and n - 1
    Case('n127', 2, 127, (((63, 64),), ((13, 49), (62, 49)))),                   # crosses key tile 64, ends at n; back-to-back 49s
    Case('n129', 2, 129, (((0, 128),), ((64, 65),)), sub=True),                  # ends ON the 128 boundary; one past it (= n)
    Case('n200', 2, 200, (((3, 196),), ((150, 196),), ((7, 49), (60, 49), (109, 49)))),   # 196 at an odd offset; clipped mid-batch; three 49s
    Case('n1000', 2, 1000, (((1, 196), (197, 196), (500, 300)), ((63, 1), (64, 64), (129, 127), (385, 257))), sub=True),  # ends on 128 / 256
    Case('n1024', 2, 1024, (((0, 1024),), ((5, 49), (100, 196), (700, 324)))),   # whole sample one block; 196; a long block ending at n
    Case('n2048', 2, 2048, (((17, 196), (1000, 256), (1900, 200)),)),            # b 1, h 2; clipped at n
    Case('n4096', 2, 4096, (((0, 49), (2049, 300), (3800, 296)),)),              # b 1, h 2; ends at n
    Case('h16', 16, 300, (((1, 196), (197, 49)),)),
    Case('dh32', 4, 200, (((4, 49), (53, 49), (102, 49)), ((0, 49),)), dh=32, sub=True),
]
CASES = {c.name: c for c in CATALOGUE}


def layout_maps(n, samples):
    """kv_end, q_start (b, n) int32 of the packing rule (packing.token_maps) for per-sample block lists"""
    b = len(samples)
    kv_end = torch.arange(1, n + 1, dtype=torch.int32).repeat(b, 1)
    q_start = torch.arange(n, dtype=torch.int32).repeat(b, 1)
    for s, blocks in enumerate(samples):
        for off, ln in blocks:
            lo, hi = min(off, n), min(off + ln, n)
            if hi > lo:
                kv_end[s, lo:hi] = hi
                q_start[s, lo:hi] = lo
    return kv_end, q_start


def edges(case):
    """[(kind, sample, e)]: the rows of `sample` with kv_end == e form one edge.  Kinds: clipped (a block cut by n) / tile (e on a 64-key
    boundary) / block_end / block_start (the causal row in front of a block) / causal (a row inside a text run)"""
    kv_end, q_start = layout_maps(case.n, case.samples)
    n, out, seen = case.n, [], set()

    def add(kind, s, e):
        if (s, e) not in seen:
            seen.add((s, e))
            out.append((kind, s, e))
    for s, blocks in enumerate(case.samples):
        ke, qs = kv_end[s].tolist(), q_start[s].tolist()
        causal = [ke[r] == r + 1 and qs[r] == r for r in range(n)]
        for off, ln in blocks:
            lo, hi = min(off, n), min(off + ln, n)
            if hi <= lo:
                continue
            add('clipped' if off + ln > n else ('tile' if hi % 64 == 0 else 'block_end'), s, hi)
            if lo >= 1 and causal[lo - 1]:
                add('block_start', s, lo)
        for r in range(n):
            if causal[r] and (r + 1) % 64 == 0:
                add('tile', s, r + 1)
        r = 0
        while r < n:                                       # one row inside every text run of >= 3 rows
            if not causal[r]:
                r += 1
                continue
            a = r
            while r < n and causal[r]:
                r += 1
            if r - a >= 3:
                add('causal', s, (a + r) // 2 + 1)
    return out


def gains_scale(mode, dh):
    """gain spread whose bound B = 1.02 dh^0.5 (1 + g)^2 (norm_scale^2 q_scale = dh^0.5) makes tfx_qk_norm_rope_fwd write a plan of `mode`"""
    return math.sqrt(B_OVER_CAP[mode] * CAP / (1.02 * dh ** 0.5)) - 1.


def build_inputs(case, mode, seed=0):
    """raw inputs on the CPU: qkvg (T, ld) fp32 = raw q | raw k | v | gate logits | pad (the projection's layout), dout (T, h 64), gains (64,) x 2,
    kv_end / q_start (b, n) int32, and the sentinel edges [(kind, sample, rows, keys)]"""
    g = torch.Generator().manual_seed(seed * 1000 + case.n * 7 + case.h)
    b, h, n, dh = case.b, case.h, case.n, case.dh
    T, HD = b * n, h * 64
    ld = 3 * HD + (h + 7) // 8 * 8 + 8
    x = torch.randn(T, ld, generator=g)
    q, k, v = (x[:, i * HD:(i + 1) * HD].view(T, h, 64) for i in range(3))
    if dh < 64:
        q[:, :, dh:] = 0; k[:, :, dh:] = 0; v[:, :, dh:] = 0
    gs = gains_scale(mode, dh)
    gq = (torch.rand(64, generator=g) * 2 - 1) * gs
    gk = (torch.rand(64, generator=g) * 2 - 1) * gs
    for c in SENT_COLS:                                   # the sentinel directions carry the largest gains: their scores reach the bound
        gq[c] = gs; gk[c] = gs
    gq[0] = gk[0] = 0.5 * gs
    for hh in range(0, h, 2):                             # sentinel heads: the other rows and keys share a direction (column 0) and have nothing on
        q[:, hh, list(SENT_COLS)] = 0                     # the sentinel columns, so the other rows all but ignore the sentinel keys - a sentinel
        k[:, hh, list(SENT_COLS)] = 0                     # key's dk / dv come from its edge's rows
        q[:, hh, 0] += BASE_QK
        k[:, hh, 0] += BASE_QK
    kv_end, q_start = layout_maps(n, case.samples)
    E = edges(case)
    parent = list(range(len(E)))                          # edges that share a key share a direction (union-find over keys)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    owner = {}
    for i, (kind, s, e) in enumerate(E):
        for key in (e - 2, e - 1, e):
            if 0 <= key < n:
                if (s, key) in owner:
                    parent[find(i)] = find(owner[(s, key)])
                else:
                    owner[(s, key)] = i
    roots = sorted({find(i) for i in range(len(E))})
    col = {r: SENT_COLS[j % len(SENT_COLS)] for j, r in enumerate(roots)}
    wdir = {r: torch.randn(dh, generator=g) for r in roots}     # per direction group: the edge rows' dout and the keys' value offsets
    wdir = {r: w / w.norm() for r, w in wdir.items()}
    dout = torch.randn(T, h, 64, generator=g)
    sent = []
    ke = kv_end.tolist()
    for i, (kind, s, e) in enumerate(E):
        rows = [r for r in range(n) if ke[s][r] == e]
        keys = [key for key in (e - 2, e - 1, e) if 0 <= key < n]
        c, w = col[find(i)], wdir[find(i)]
        for hh in range(0, h, 2):
            for r in rows:                                # the query IS the direction ...
                q[s * n + r, hh, :dh] = 0
                q[s * n + r, hh, c] = SENT_Q
                dout[s * n + r, hh, :dh] = SENT_DO * w
            for key in keys:                              # ... each key = the direction + its own part of one fixed length on the other sentinel
                u = torch.zeros(dh)                       # columns: the scores tie (the row's weight splits evenly over the visible ones), the
                oth = [c2 for c2 in SENT_COLS if c2 != c]   # keys differ (so do dq and dk)
                u[oth] = torch.randn(len(oth), generator=g)
                k[s * n + key, hh, :dh] = SENT_K * 0.5 * u / u.norm()
                k[s * n + key, hh, c] = SENT_K
                v[s * n + key, hh, :dh] = SENT_V * (torch.randint(0, 2, (dh,), generator=g) * 2 - 1).float() + SENT_W * VCOEF[key % 3] * w
        sent.append((kind, s, rows, keys))
    x[:, 3 * HD + h:] = 0
    if dh < 64:
        dout[:, :, dh:] = 0
    return dict(qkvg=x, ld=ld, dout=dout.reshape(T, HD), gq=gq, gk=gk, kv_end=kv_end, q_start=q_start, edges=sent,
                q_scale=dh ** -0.5, norm_scale=dh ** 0.5)


def norm_qk(raw, h, gq, gk, q_scale, norm_scale):
    """torch restatement of tfx_qk_norm_rope_fwd at identity rotation: raw q | k (T, 2 h 64) -> q~ | k~ (RMSNorm over the head's 64 columns)"""
    T = raw.shape[0]
    y = raw.reshape(T, 2, h, 64)
    y = y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12) * norm_scale * (torch.stack([gq, gk]).to(raw.dtype)[None, :, None, :] + 1)
    return (y * torch.tensor([q_scale, 1.], dtype=raw.dtype, device=raw.device)[None, :, None, None]).reshape(T, 2 * h * 64)


def heads(x, b, n, h):
    """(T, >= h 64) token-major -> (b, h, n, 64)"""
    return x[:, :h * 64].reshape(b, n, h, 64).transpose(1, 2)


def attention_ref(q, k, v, gate, kv_end, laser=False, cap=CAP):
    """q (b, h, nq, 64), k / v (b, h, nk, 64) (raw v), gate logits (b, h, nq), kv_end (b, nq): key j visible to row i iff j < kv_end[i].
    Masked with -inf; returns (gated output, lse).  laser: og = sigmoid(gate) log(P exp(c tanh(v / c)))"""
    s = torch.tanh(torch.einsum('bhid,bhjd->bhij', q, k) / cap) * cap
    mask = torch.arange(k.shape[2], device=q.device)[None, None, :] < kv_end.long()[:, :, None]
    s = s.masked_fill(~mask[:, None], float('-inf'))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    vv = torch.exp(LASER_C * torch.tanh(v / LASER_C)) if laser else v
    o = torch.einsum('bhij,bhjd->bhid', p, vv)
    if laser:
        o = torch.log(o)
    return o * gate.sigmoid()[..., None], lse


def row_err(got, ref, floor=ROW_FLOOR):
    """per-row relative error over the last dim of (b, h, rows, d) tensors, normalised by max(row norm, floor x the RMS row norm of the (b, h) slice)"""
    got, ref = got.double(), ref.double()
    rn = ref.norm(dim=-1)
    rms = rn.pow(2).mean(dim=-1, keepdim=True).sqrt().clamp_min(1e-30)
    return (got - ref).norm(dim=-1) / torch.maximum(rn, floor * rms)


def scalar_err(got, ref, floor=ROW_FLOOR):
    """the same for one value per (b, h, row)"""
    return row_err(got.unsqueeze(-1), ref.unsqueeze(-1), floor)


def reference(inp, case, laser=False, nr=False, qk=None, dev='cpu', kv_end=None):
    """fp64 autograd.  qk: the kernel's own q~ | k~ (T, 2 h 64) as exact inputs; None = through norm_qk from the raw q / k (nr: gradients down to
    the raw q / k and the gains).  kv_end: override of the case's (the mutation test).  Returns (b, h, n, 64) / (b, h, n) tensors."""
    b, h, n = case.b, case.h, case.n
    T, HD = b * n, h * 64
    X = inp['qkvg'].to(dev).double()
    raw = X[:, :2 * HD].clone().requires_grad_(nr)
    gq = inp['gq'].to(dev).double().requires_grad_(nr)
    gk = inp['gk'].to(dev).double().requires_grad_(nr)
    qkt = norm_qk(raw, h, gq, gk, inp['q_scale'], inp['norm_scale']) if qk is None else qk.to(dev).double()
    q, k = heads(qkt[:, :HD], b, n, h), heads(qkt[:, HD:], b, n, h)
    if not nr:
        q, k = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
    v = heads(X[:, 2 * HD:3 * HD], b, n, h).detach().requires_grad_(True)
    g = X[:, 3 * HD:3 * HD + h].reshape(b, n, h).transpose(1, 2).detach().requires_grad_(True)
    out, lse = attention_ref(q, k, v, g, (inp['kv_end'] if kv_end is None else kv_end).to(dev), laser=laser)
    out.backward(heads(inp['dout'].to(dev).double(), b, n, h))
    r = dict(out=out.detach(), lse=lse.detach(), dv=v.grad, dgate=g.grad)
    if nr:
        r.update(dq=heads(raw.grad[:, :HD], b, n, h), dk=heads(raw.grad[:, HD:], b, n, h), dgq=gq.grad, dgk=gk.grad)
    else:
        r.update(dq=q.grad, dk=k.grad)
    return r


def exact_input_reference(inp, case, qk, got, laser=False, nr=False, dev='cpu'):
    """fp64 restatement of what each kernel computes FROM ITS OWN INPUTS - the per-row reference of the sweep:
      forward:  out, lse from the kernel's bf16 q~ | k~ (and, LASER, its bf16 v');
      prep:     do_eff, delta, dgate from the forward kernel's bf16 out (tfx.h tfx_attn_args.laser for the LASER forms);
      dK/dV, dQ: dS = P (dP - delta) (1 - tanh^2) with dP = do_eff v^T from the prep kernel's bf16 do_eff and fp32 delta; dq, dk, dv (LASER: d v'
                through tfx_laser_v_bwd's factor; nr: d q~ | d k~ through the QK-norm backward down to the raw q / k and the gains).
    A row whose exact gradient vanishes (one visible key, all weight on one key) keeps the bf16 residue of delta in the kernels' dS; feeding the
    reference the kernels' own do_eff / delta leaves only the kernels' arithmetic to judge, while do_eff / delta / dgate are checked on their
    own and the whole chain against fp64 autograd (reference()) with the global tolerances."""
    b, h, n = case.b, case.h, case.n
    T, HD = b * n, h * 64
    X = inp['qkvg'].to(dev).double()
    q, k = heads(qk.to(dev).double(), b, n, h), heads(qk[:, HD:].to(dev).double(), b, n, h)
    v = heads(X[:, 2 * HD:3 * HD], b, n, h)
    g = X[:, 3 * HD:3 * HD + h].reshape(b, n, h).transpose(1, 2)
    vin = got['vl'].to(dev).double() if laser else v
    t = torch.tanh(torch.einsum('bhid,bhjd->bhij', q, k) / CAP)
    mask = torch.arange(n, device=dev)[None, None, :] < inp['kv_end'].to(dev).long()[:, :, None]
    s = (t * CAP).masked_fill(~mask[:, None], float('-inf'))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum('bhij,bhjd->bhid', p, vin)
    sg = g.sigmoid()[..., None]
    r = dict(out=(torch.log(o) if laser else o) * sg, lse=lse)
    dout = heads(inp['dout'].to(dev).double(), b, n, h)
    og = got['out'].to(dev).double()
    if laser:
        r['do_eff'] = dout * sg * torch.exp(-og / sg)
        r['delta'] = (dout * sg).sum(-1)
    else:
        r['do_eff'] = dout * sg
        r['delta'] = (dout * og).sum(-1)
    r['dgate'] = (dout * og).sum(-1) * (1 - sg[..., 0])
    de, dl = got['do_eff'].to(dev).double(), got['delta'].to(dev).double()
    ds = p * (torch.einsum('bhid,bhjd->bhij', de, vin) - dl[..., None]) * (1 - t * t)
    dq, dk = torch.einsum('bhij,bhjd->bhid', ds, k), torch.einsum('bhij,bhid->bhjd', ds, q)
    dv = torch.einsum('bhij,bhid->bhjd', p, de)
    if laser:
        th = torch.tanh(v / LASER_C)
        dv = dv * torch.exp(LASER_C * th) * (1 - th * th)
    r['dv'] = dv
    if nr:
        # the gain gradients are sums over every token and head whose terms cancel ~1000-fold in these inputs: their scale is the sum of |terms|
        tok = lambda x: x.transpose(1, 2).reshape(T, HD)
        unit = X[:, :2 * HD].reshape(T, 2, h, 64)
        unit = unit / unit.norm(dim=-1, keepdim=True).clamp_min(1e-12) * inp['norm_scale']
        r['dgq_scale'] = (tok(dq).reshape(T, h, 64) * unit[:, 0] * inp['q_scale']).abs().sum((0, 1))
        r['dgk_scale'] = (tok(dk).reshape(T, h, 64) * unit[:, 1]).abs().sum((0, 1))
        raw = X[:, :2 * HD].clone().requires_grad_(True)
        gq = inp['gq'].to(dev).double().requires_grad_(True)
        gk = inp['gk'].to(dev).double().requires_grad_(True)
        draw, r['dgq'], r['dgk'] = torch.autograd.grad(norm_qk(raw, h, gq, gk, inp['q_scale'], inp['norm_scale']), (raw, gq, gk),
                                                       torch.cat([tok(dq), tok(dk)], 1))
        r['dq'], r['dk'] = heads(draw[:, :HD], b, n, h), heads(draw[:, HD:], b, n, h)
    else:
        r['dq'], r['dk'] = dq, dk
    return r


def gain_err(got, ref, scale):
    """error of a gain gradient (64,) relative to the sum of the magnitudes of its terms"""
    return ((got.double() - ref.double()).norm() / scale.double().norm().clamp_min(1e-30)).item()


def metrics(got, ref):
    """per-row errors (b, h, n) of every quantity both dicts hold"""
    m = {}
    for key in ('out', 'dq', 'dk', 'dv', 'do_eff'):
        if key in got and key in ref:
            m[key] = row_err(got[key], ref[key])
    for key in ('dgate', 'delta'):
        if key in got and key in ref:
            m[key] = scalar_err(got[key], ref[key])
    if 'lse' in got and 'lse' in ref:
        m['lse'] = (got['lse'].double() - ref['lse'].double()).abs()
    return m


# ---------------------------------------------------------------------------------------------- the kernels (GPU only; capi imported lazily)
POISON = 0x7FA5                  # a bf16 NaN: outputs start as it, columns the kernels must not touch must keep its bits


def run_kernels(case, mode, laser=False, nr=False, seed=0, dev='cuda'):
    """tfx_qk_norm_rope_fwd (identity rotation; writes the plan) -> [tfx_laser_v_fwd] -> tfx_attn_fwd -> tfx_attn_bwd [-> tfx_laser_v_bwd] on the
    case's sentinel inputs, in the product's buffer layout: one q | k | v | gate gradient matrix with a pad behind the gates, out with ld > h 64.
    Asserts that every output element was written and every guard column kept its bits.  mode None: no plan passed (the kernels decide from
    the scores).  Returns (inputs as the kernels saw them, the kernels' q~ | k~, outputs as (b, h, n, ...) tensors + 'raw' buffers)."""
    from transfusion_pytorch_amd import capi
    st = torch.cuda.current_stream().cuda_stream
    BF = torch.bfloat16
    inp = build_inputs(case, mode, seed)
    b, h, n = case.b, case.h, case.n
    T, HD, ld = b * n, h * 64, inp['ld']
    qkvg = inp['qkvg'].to(dev).to(BF)
    inp['qkvg'] = qkvg.float().cpu()                        # the bf16-rounded values the kernels see are the reference's inputs
    gq, gk = inp['gq'].to(dev), inp['gk'].to(dev)
    kv_end, q_start = inp['kv_end'].reshape(-1).to(dev), inp['q_start'].reshape(-1).to(dev)
    pos = torch.zeros(T, device=dev, dtype=torch.int32)
    cos_t, sin_t = torch.ones(8, 32, device=dev), torch.zeros(8, 32, device=dev)
    qk = torch.zeros(T, 2 * HD, device=dev, dtype=BF)
    plan = torch.full((8,), float('nan'), device=dev)
    fa = capi.make_args('tfx_qk_norm_rope_args', T=T, H=h, qkv=qkvg, ld_qkv=ld, qk=qk, ld_qk=2 * HD, gamma_q=gq, gamma_k=gk, rot_pos=pos,
                        cos_tab=cos_t, sin_tab=sin_t, q_scale=inp['q_scale'], norm_scale=inp['norm_scale'], sc_plan=plan, softcap=CAP)
    capi.call('tfx_qk_norm_rope_fwd', fa, st)
    torch.cuda.synchronize()
    assert int(plan[0].item()) == (2 if mode is None else mode), (case.name, mode, plan.tolist())

    def poisoned(*shape):
        return torch.full(shape, POISON, device=dev, dtype=torch.int16).view(BF)
    ld_out, ld_qk = HD + 24, 2 * HD + 8
    out = poisoned(T, ld_out)
    lse = torch.full((b, h, n), float('nan'), device=dev)
    dout = inp['dout'].to(dev).to(BF)
    inp['dout'] = dout.float().cpu()
    do_eff = poisoned(T, HD)
    delta = torch.full((b, h, n), float('nan'), device=dev)
    dqk = poisoned(T, ld_qk)
    dqkv = poisoned(T, ld)
    vl = None
    if laser:
        vl = torch.zeros(T, HD, device=dev, dtype=BF)
        la = capi.make_args('tfx_laser_v_args', T=T, H=h, v=qkvg[:, 2 * HD:], ld_v=ld, vl=vl, ld_vl=HD, c=LASER_C)
        capi.call('tfx_laser_v_fwd', la, st)
        v_in, ld_v = vl, HD
    else:
        v_in, ld_v = qkvg[:, 2 * HD:], ld
    kw = dict(q=qk, k=qk[:, HD:], v=v_in, ld_q=2 * HD, ld_k=2 * HD, ld_v=ld_v, gate=qkvg[:, 3 * HD:], ld_gate=ld, kv_end=kv_end, q_start=q_start,
              out=out, ld_out=ld_out, lse=lse, b=b, h=h, n=n, softcap=CAP, dout=dout, ld_dout=HD, do_eff=do_eff, ld_do=HD, delta=delta,
              dgate=dqkv[:, 3 * HD:], ld_dgate=ld, dq=dqk, dk=dqk[:, HD:], dv=dqkv[:, 2 * HD:], ld_dq=ld_qk, ld_dk=ld_qk, ld_dv=ld,
              sc_plan=None if mode is None else plan, laser=int(laser))
    dgq, dgk = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    if nr:
        kw.update(nr_qkv=qkvg, nr_ld_qkv=ld, nr_dqkv=dqkv, nr_ld_dqkv=ld, nr_gamma_q=gq, nr_gamma_k=gk, nr_rot_pos=pos, nr_cos=cos_t, nr_sin=sin_t,
                  nr_q_scale=inp['q_scale'], nr_norm_scale=inp['norm_scale'], nr_dgamma_q=dgq, nr_dgamma_k=dgk)
    a = capi.make_args('tfx_attn_args', **kw)
    capi.call('tfx_attn_fwd', a, st)
    capi.call('tfx_attn_bwd', a, st)
    if laser:
        lb = capi.make_args('tfx_laser_v_args', T=T, H=h, v=qkvg[:, 2 * HD:], ld_v=ld, c=LASER_C, dvl=dqkv[:, 2 * HD:], ld_dvl=ld,
                            dv=dqkv[:, 2 * HD:], ld_dv=ld)
        capi.call('tfx_laser_v_bwd', lb, st)
    torch.cuda.synchronize()

    def untouched(x):
        return bool((x.view(torch.int16) == POISON).all())
    assert torch.isfinite(out[:, :HD].float()).all(), 'out: unwritten or non-finite elements'
    assert untouched(out[:, HD:]), 'out: the ld padding was written'
    assert torch.isfinite(lse).all(), 'lse: unwritten or non-finite'
    assert torch.isfinite(do_eff.float()).all() and torch.isfinite(delta).all(), 'do_eff / delta: unwritten or non-finite'
    assert torch.isfinite(dqkv[:, 2 * HD:3 * HD + h].float()).all(), 'd v | d gate: unwritten or non-finite elements'
    assert untouched(dqkv[:, 3 * HD + h:]), 'the pad behind the gate columns was written'
    if nr:
        assert torch.isfinite(dqkv[:, :2 * HD].float()).all(), 'd q | d k (raw): unwritten or non-finite elements'
        assert untouched(dqk), 'the fused form must not write d q~ / d k~'
    else:
        assert torch.isfinite(dqk[:, :2 * HD].float()).all(), 'd q~ | d k~: unwritten or non-finite elements'
        assert untouched(dqk[:, 2 * HD:]), 'd q~ | d k~: the ld padding was written'
        assert untouched(dqkv[:, :2 * HD]), 'the q / k columns of the gradient matrix were written'

    def hd(x):
        return heads(x.float(), b, n, h)
    got = dict(out=hd(out), lse=lse, dv=hd(dqkv[:, 2 * HD:]), dgate=dqkv[:, 3 * HD:3 * HD + h].float().reshape(b, n, h).transpose(1, 2),
               do_eff=hd(do_eff), delta=delta, raw=dict(out=out[:, :HD], lse=lse, dqk=dqk[:, :2 * HD], dqkv=dqkv[:, :3 * HD + h]))
    if laser:
        got['vl'] = hd(vl)
    if nr:
        got.update(dq=hd(dqkv[:, :HD]), dk=hd(dqkv[:, HD:]), dgq=dgq, dgk=dgk)
    else:
        got.update(dq=hd(dqk[:, :HD]), dk=hd(dqk[:, HD:]))
    return inp, qk, got
