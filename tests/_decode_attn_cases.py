"""Visible-length catalogue of the decode attention tests (not collected: no test_ prefix; imports no GPU code at module level).

A decode case is `lq` NEW query rows per sample against a KV cache of `n_kv` rows per sample; `kv_end` lists, per sample, the visible length of
each of its rows (key j is visible to a row iff j < its kv_end; a sample's rows need not be ordered by visible length).  In the compacted layout
(`units` = (row0, cnt, R)) the query rows are a flat list of R rows of which sample s owns rows row0[s] .. row0[s] + cnt[s] - 1, `kv_end` lists
cnt[s] lengths for it and `lq` is the largest cnt.

build_decode_inputs() follows the sentinel rule of _attn_cases.build_inputs with its constants: in the even heads every distinct (sample, e) with
rows whose kv_end == e is an edge; its keys e - 2, e - 1 and the first masked key e (where e < n_kv) are aligned with those rows' queries along
a sentinel column and carry large, distinct values, so the three scores tie near the soft-cap plan's bound and one key more or less moves the
rows' output and lse by O(1) - which tests/test_decode_attn_cases_cpu.py proves against the tolerances the GPU tests assert
(tests/test_decode_attn_edges_gpu.py).  Cache rows behind a sample's largest kv_end are as loud as the visible ones (random keys and values of
the same scale, and the sample's sentinel at e): a kernel that walks one row too far reads something finite that counts.  The odd heads stay
random.  The CPU proof's smallest margins over the catalogue: out 38 x the tolerance plain, 27 x LASER; lse 167 x.

Worst per-row values measured on the MI355X over the catalogue stand in brackets behind each list (out by row_err, lse absolute in nats; the
tolerances are _attn_cases.row_tol: out 1e-2, lse 1e-3, plain and LASER).
"""
from typing import NamedTuple

import torch

from _attn_cases import (B_OVER_CAP, BASE_QK, CAP, LASER_C, MUTATION_MARGIN, POISON, SENT_COLS, SENT_K, SENT_Q, SENT_V, SENT_W,  # noqa: F401
                         VCOEF, attention_ref, gains_scale, heads, norm_qk, row_err, row_tol, scalar_err)


class DecodeCase(NamedTuple):
    name: str
    h: int
    lq: int                      # new query rows per sample (compacted: the largest unit)
    n_kv: int                    # cache rows per sample
    kv_end: tuple                # per sample (compacted: per unit): the visible length of each of its rows
    dh: int = 64                 # dim_head; 32 = upper 32 columns of every head zero, q_scale / norm_scale from 32
    sub: bool = False            # in the subset of the LASER runs (none with n_kv >= 2048: the log compresses a long row below the margin)
    units: tuple = None          # compacted layout: (row0 per unit, cnt per unit, R flat rows)

    @property
    def b(self):
        return len(self.kv_end)

    @property
    def R(self):
        return self.units[2] if self.units else self.b * self.lq

    def spans(self):
        """[(sample, first flat row, rows)]"""
        if self.units:
            return [(s, r0, c) for s, (r0, c) in enumerate(zip(self.units[0], self.units[1]))]
        return [(s, s * self.lq, self.lq) for s in range(self.b)]


def _blk(n, e, **rows):
    """n rows at visible length e, with the rows named r<i>=<length> set apart"""
    t = [e] * n
    for k, v in rows.items():
        t[int(k[1:])] = v
    return tuple(t)


TRIP = DecodeCase('trip', 2, 1, 77, tuple((e,) for e in (1, 8, 9, 31, 32, 33, 63, 64, 65, 76, 77)), sub=True)
PAIRS = DecodeCase('pairs', 2, 2, 77, ((1, 77), (77, 1), (32, 33), (33, 32), (64, 64), (8, 9), (31, 65), (76, 77)), sub=True)
# the short row beside the long one in both orders (the rows kernel's key walk ends at the longer row's length), both sides of a 32-key trip

# tfx_decode_attn with lq 1 / 2 in the dense layout: decode_attn_rows_k<1> / <2> (4 waves x 8 key groups, 32 keys per trip)
ROWS_CASES = [
    DecodeCase('all_lengths', 8, 1, 40, tuple((s + 1,) for s in range(40))),     # 320 blocks: more than one per CU
    DecodeCase('small', 2, 1, 9, tuple((e,) for e in (1, 2, 3, 7, 8, 9)), sub=True),
    TRIP,
    DecodeCase('odd_heads', 3, 1, 333, tuple((e,) for e in (95, 96, 97, 128, 129, 256, 257, 332, 333))),
    DecodeCase('k1100', 2, 1, 1100, ((1,), (1057,), (1100,)), sub=True),
    PAIRS,
    DecodeCase('long', 2, 2, 4100, ((1, 4100), (4097, 4096), (2049, 2048))),      # plain only
]
# [rows kernel: out 3.2e-3 plain, 2.1e-3 LASER; lse 5.2e-6]

# tfx_attn_fwd with n_kv > 0: attn_fwd_pipe_kernel<true> with cache addressing (128-row query tiles of 4 waves x 32 rows, 64-key tiles of two
# 32-key units); 'trip' and 'pairs' again are the engine's tile_attn plans - one and two rows on the tiled kernel
TILED_CASES = [
    TRIP,
    PAIRS,
    DecodeCase('t7', 2, 7, 40, ((1, 40, 39, 33, 32, 8, 2),), sub=True),           # less than one key tile; also through tfx_decode_attn (delegates)
    DecodeCase('t5', 2, 5, 100, ((96, 97, 1, 100, 64), (33, 32, 31, 65, 63))),
    DecodeCase('t49', 2, 49, 200, (_blk(49, 113, r7=174, r48=64),                  # the largest on an inner row, the smallest on the last row
                                   _blk(49, 128, r0=129),                          # one wave's rows on both sides of a 32-key unit boundary
                                   _blk(49, 200, r31=1, r32=1)), sub=True),        # kv_end == n_kv; one-key rows on both sides of a wave boundary
    DecodeCase('t130', 2, 130, 333, (_blk(128, 256, r100=333) + (65, 257),)),     # two query tiles, the second with two rows
    DecodeCase('t300', 2, 300, 1100, (_blk(300, 700, r5=797, r128=641, r299=1100),), sub=True),   # three query tiles
    DecodeCase('t5_dh32', 4, 5, 100, ((50, 49, 1, 100, 33), (64, 65, 2, 99, 96)), dh=32, sub=True),
    DecodeCase('t2_long', 2, 2, 4100, ((1, 4100), (4097, 4096), (2049, 2048))),   # plain only
]
# [tiled kernel, dense: out 4.5e-3 plain, 4.0e-3 LASER; lse 5.2e-5 (plan mode 0; 1.7e-5 mode 1, 3.9e-6 without a plan)]

# the same kernel in the compacted layout: units of 1, 0, 2, 57 and 140 rows in a flat list of 220 rows; rows 0-2, 4-8, 12, 70-74 and 215-219
# belong to no unit (poisoned, must keep their bits).  The larger units are blocks with a longer inner row.
COMPACT = DecodeCase('compact', 2, 140, 333, ((1,), (), (333, 32), _blk(57, 200, r9=257), _blk(140, 96, r20=129, r133=161)), sub=True,
                     units=((3, 9, 10, 13, 75), (1, 0, 2, 57, 140), 220))
# [tiled kernel, compacted: out 4.3e-3 plain, 2.8e-3 LASER; lse 5.1e-5]

CASES = {c.name: c for c in ROWS_CASES + TILED_CASES + [COMPACT]}
CATALOGUE = list(CASES.values())                       # every case once ('trip' and 'pairs' stand in two lists)


def case_edges(case):
    """[(sample, e, rows of the sample with kv_end == e)] in order of first appearance"""
    out = []
    for s, ke in enumerate(case.kv_end):
        for e in dict.fromkeys(ke):
            out.append((s, e, [i for i, x in enumerate(ke) if x == e]))
    return out


def build_decode_inputs(case, mode, seed=0):
    """raw inputs on the CPU (fp32): q (R, h 64) for the flat query rows, k / v (b n_kv, h 64) for the cache rows (pre QK-RMSNorm q / k, raw
    v), gate logits (R, h), gains gq / gk (64,) for plan mode `mode` (gains_scale), kv_end (R,) int32 (1 on rows no unit owns), and the sentinel
    edges [(kind, sample, rows, keys)] (rows: indices inside the sample; kind: 'one' / 'full' (e == n_kv: no masked key) / 'edge')"""
    g = torch.Generator().manual_seed(seed * 1000 + case.n_kv * 7 + case.h + 31 * case.lq)
    b, h, dh, n_kv, R = case.b, case.h, case.dh, case.n_kv, case.R
    q = torch.randn(R, h, 64, generator=g)
    k = torch.randn(b * n_kv, h, 64, generator=g)
    v = torch.randn(b * n_kv, h, 64, generator=g)
    gate = torch.randn(R, h, generator=g)
    if dh < 64:
        q[:, :, dh:] = 0; k[:, :, dh:] = 0; v[:, :, dh:] = 0
    gs = gains_scale(mode, dh)
    gq = (torch.rand(64, generator=g) * 2 - 1) * gs
    gk = (torch.rand(64, generator=g) * 2 - 1) * gs
    for c in SENT_COLS:                                   # the sentinel directions carry the largest gains: their scores reach the bound
        gq[c] = gs; gk[c] = gs
    gq[0] = gk[0] = 0.5 * gs
    for hh in range(0, h, 2):                             # sentinel heads: the other rows and keys (visible or not) share column 0 and have nothing
        q[:, hh, list(SENT_COLS)] = 0                     # on the sentinel columns
        k[:, hh, list(SENT_COLS)] = 0
        q[:, hh, 0] += BASE_QK
        k[:, hh, 0] += BASE_QK
    kv_end = torch.ones(R, dtype=torch.int32)
    first = {s: r0 for s, r0, _ in case.spans()}
    for s, r0, c in case.spans():
        assert len(case.kv_end[s]) == c and all(1 <= e <= n_kv for e in case.kv_end[s]), case.name
        kv_end[r0:r0 + c] = torch.tensor(case.kv_end[s], dtype=torch.int32)
    E = case_edges(case)
    parent = list(range(len(E)))                          # edges that share a key share a direction (union-find over keys)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    owner = {}
    for i, (s, e, rows) in enumerate(E):
        for key in (e - 2, e - 1, e):
            if 0 <= key < n_kv:
                if (s, key) in owner:
                    parent[find(i)] = find(owner[(s, key)])
                else:
                    owner[(s, key)] = i
    col, per_sample = {}, {}
    for i, (s, e, rows) in enumerate(E):                  # a sample's direction groups take the sentinel columns in turn
        r = find(i)
        if r not in col:
            col[r] = SENT_COLS[per_sample.get(s, 0) % len(SENT_COLS)]
            per_sample[s] = per_sample.get(s, 0) + 1
    wdir = {r: torch.randn(dh, generator=g) for r in col}
    wdir = {r: w / w.norm() for r, w in wdir.items()}
    sent = []
    for i, (s, e, rows) in enumerate(E):
        keys = [key for key in (e - 2, e - 1, e) if 0 <= key < n_kv]
        c, w = col[find(i)], wdir[find(i)]
        for hh in range(0, h, 2):
            for r in rows:                                # the query IS the direction ...
                q[first[s] + r, hh, :dh] = 0
                q[first[s] + r, hh, c] = SENT_Q
            for key in keys:                              # ... each key = the direction + its own part of one fixed length on the other sentinel
                u = torch.zeros(dh)                       # columns: the scores tie, the keys differ
                oth = [c2 for c2 in SENT_COLS if c2 != c]
                u[oth] = torch.randn(len(oth), generator=g)
                k[s * n_kv + key, hh, :dh] = SENT_K * 0.5 * u / u.norm()
                k[s * n_kv + key, hh, c] = SENT_K
                v[s * n_kv + key, hh, :dh] = SENT_V * (torch.randint(0, 2, (dh,), generator=g) * 2 - 1).float() + SENT_W * VCOEF[key % 3] * w
        sent.append(('one' if e == 1 else 'full' if e == n_kv else 'edge', s, rows, keys))
    HD = h * 64
    return dict(q=q.reshape(R, HD), k=k.reshape(b * n_kv, HD), v=v.reshape(b * n_kv, HD), gate=gate, gq=gq, gk=gk, kv_end=kv_end, edges=sent,
                q_scale=dh ** -0.5, norm_scale=dh ** 0.5)


def round_bf16(inp):
    """the inputs as the kernels see them: q, k, v and the gate logits rounded to bf16 (in place; the gains stay fp32)"""
    for key in ('q', 'k', 'v', 'gate'):
        inp[key] = inp[key].to(torch.bfloat16).float()
    return inp


def norm_rows(inp, case, dtype=torch.float64):
    """q~ (R, h 64), k~ (b n_kv, h 64): norm_qk (tfx_qk_norm_rope_fwd at identity rotation) of the query rows and of the cache rows"""
    HD = case.h * 64
    f = lambda x: norm_qk(torch.cat([x, x], 1).to(dtype), case.h, inp['gq'], inp['gk'], inp['q_scale'], inp['norm_scale'])
    return f(inp['q'])[:, :HD], f(inp['k'])[:, HD:]


def attention_ref_from(q, k, vin, gate, kv_end, laser):
    """attention_ref from exact inputs: `vin` is raw v, or under LASER the value the kernel reads, v' = exp(c tanh(v / c))"""
    if not laser:
        return attention_ref(q, k, vin, gate, kv_end)
    o, lse = attention_ref(q, k, vin, torch.full_like(gate, float('inf')), kv_end)            # sigmoid(inf) = 1: P v'
    return torch.log(o) * gate.sigmoid()[..., None], lse


def decode_reference(case, qt, kt, vin, gate, kv_end, laser=False, vprime=False, only=None):
    """fp64 reference per unit from q~ (R, h 64), k~ / values (b n_kv, h 64), gate logits (R, h), kv_end (R,): {sample: (out (1, h, rows, 64),
    lse (1, h, rows))} for the units that own rows (only: that sample alone).  vprime: `vin` already is the LASER v'"""
    h, n_kv, ref = case.h, case.n_kv, {}
    for s, r0, c in case.spans():
        if c == 0 or (only is not None and s != only):
            continue
        qq = heads(qt[r0:r0 + c].double(), 1, c, h)
        kk = heads(kt[s * n_kv:(s + 1) * n_kv].double(), 1, n_kv, h)
        vv = heads(vin[s * n_kv:(s + 1) * n_kv].double(), 1, n_kv, h)
        gg = gate[r0:r0 + c, :h].double().t()[None]
        ke = kv_end[None, r0:r0 + c]
        ref[s] = attention_ref_from(qq, kk, vv, gg, ke, laser) if vprime or not laser else attention_ref(qq, kk, vv, gg, ke, laser=True)
    return ref
