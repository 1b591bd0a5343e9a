"""Cases and a slow scalar reference for the host side of the continuous decode schedule (transfusion_pytorch_amd/sampling.py: `step_roles`,
`dense_layout`, `compact_layout`).  The reference restates, per (guidance half h, sample i), which rows the unit brings to a step - from the rules in
words, one row at a time, sharing no code and no constants with the module under test - and then places them in either layout.

The rules (h = 0: the real history, h = 1: the null-text history of classifier-free guidance):
  * base = cache_len (h = 0) or uncond_len (h = 1): the keys the unit already has in its cache row.
  * A sample in its modality phase brings its ODE block: L rows at cache offsets base + s + j, where s = 1 only in the null-text half while the [som] that
    opened the block is still pending there; every row sees kve = base + s + L keys, sits at rotary position tokens_seen and reads the conditioning table
    of instance ode_k.  The pending [som] itself is a token row at offset base with the null id, kve = base + 1, rotary position uncond_pos.
  * A sample in its text phase brings one token row: id last_token (the null id in the null-text half) at offset base, kve one more, rotary position
    tokens_seen (h = 0) or uncond_pos (h = 1).  In the null-text half a block just committed may still be missing (`commit_pending`): it goes in ahead of the
    token as a finished block - L rows at base + j, kve = base + L, rotary position uncond_pos, instance n_t - 1 (t = 1) - and the token moves behind it:
    offset base + L, rotary position uncond_pos + 1.
  * A done sample brings nothing.
Dense layout: Lq rows per unit, block rows in columns 0 .. L - 1, the token row in column Lq - 1; rows that carry nothing have id 0, pos -1,
kve = max(base, 1), rot 0, instance -1.  Compacted layout: the units' rows back to back (block first), padded to a multiple of the bucket with rows of
id 0, pos -1, kve 1, rot 0, instance -1, plus four per-unit arrays: first row, row count, first block row (-1: none) and - first B entries of the fourth,
the real-history half only - the token row (0: none).  A row's cache position is unit * cap + offset."""
import numpy as np

FIELDS = ('phase', 'cache_len', 'uncond_len', 'tokens_seen', 'uncond_pos', 'last_token', 'length', 'type', 'ode_k', 'som_pending', 'commit_pending')
F = {name: k for k, name in enumerate(FIELDS)}                    # the row order of the host mirror
DONE, TEXT, MOD = 0, 1, 2
NULL_ID = 77


def mirror(*samples):
    """samples as dicts of FIELDS (missing = 0) -> the [11, B] mirror"""
    A = np.zeros((len(FIELDS), len(samples)), np.int64)
    for i, s in enumerate(samples):
        for k, v in s.items():
            A[F[k], i] = v
    return A


def unit_rows(A, h, i, n_t):
    """(block rows, token row | None) of unit (h, i); a row = (id, cache offset, kve, rot, instance)"""
    g = lambda name: int(A[F[name], i])
    base, L = g('uncond_len') if h else g('cache_len'), g('length')
    if g('phase') == MOD:
        s = 1 if h == 1 and g('som_pending') else 0
        blk = [(0, base + s + j, base + s + L, g('tokens_seen'), g('ode_k')) for j in range(L)]
        return blk, ((NULL_ID, base, base + 1, g('uncond_pos'), -1) if s else None)
    if g('phase') == TEXT:
        ahead = h == 1 and g('commit_pending')
        blk = [(0, base + j, base + L, g('uncond_pos'), n_t - 1) for j in range(L)] if ahead else []
        off = base + (L if ahead else 0)
        rot = (g('uncond_pos') + (1 if ahead else 0)) if h else g('tokens_seen')
        return blk, (NULL_ID if h else g('last_token'), off, off + 1, rot, -1)
    return [], None


def is_mixed(A):
    return bool(((A[F['phase']] == MOD) | ((A[F['phase']] == TEXT) & (A[F['commit_pending']] > 0))).any())


def reference_dense(A, H, n_t, Lq, cap):
    B = A.shape[1]
    out = dict(ids=np.zeros((H, B, Lq), np.int64), pos=np.full((H, B, Lq), -1, np.int64), kve=np.zeros((H, B, Lq), np.int64), rot=np.zeros((H, B, Lq), np.int64),
               tok_inst=np.full((H, B, Lq), -1, np.int64), blk_rows=np.zeros((H, B, Lq), bool), row_ty=np.zeros((H, B, Lq), np.int64), unit_row0=np.zeros(H * B, np.int64))
    for h in range(H):
        for i in range(B):
            unit = h * B + i
            out['kve'][h, i, :] = max(int(A[F['uncond_len' if h else 'cache_len'], i]), 1)
            out['row_ty'][h, i, :] = A[F['type'], i]
            out['unit_row0'][unit] = unit * Lq
            blk, tok = unit_rows(A, h, i, n_t)
            for col, row in [(j, r) for j, r in enumerate(blk)] + ([(Lq - 1, tok)] if tok else []):
                assert col < Lq - 1 or row is tok, 'a block never reaches the token column'
                out['ids'][h, i, col], out['kve'][h, i, col], out['rot'][h, i, col], out['tok_inst'][h, i, col] = row[0], row[2], row[3], row[4]
                out['pos'][h, i, col] = unit * cap + row[1]
                out['blk_rows'][h, i, col] = row is not tok
    return out


def reference_compact(A, H, n_t, step, cap):
    B = A.shape[1]
    U = H * B
    rows, units = [], np.zeros(4 * U, np.int64)
    for h in range(H):
        for i in range(B):
            unit = h * B + i
            blk, tok = unit_rows(A, h, i, n_t)
            units[unit], units[U + unit] = len(rows), len(blk) + (tok is not None)
            units[2 * U + unit] = len(rows) if blk else -1
            if h == 0 and tok is not None:
                units[3 * U + i] = len(rows) + len(blk)
            rows += [(unit, int(A[F['type'], i]), True, r) for r in blk] + ([(unit, int(A[F['type'], i]), False, tok)] if tok else [])
    Tb = max(step, -(-len(rows) // step) * step)
    out = dict(ids=np.zeros(Tb, np.int64), pos=np.full(Tb, -1, np.int64), kve=np.ones(Tb, np.int64), rot=np.zeros(Tb, np.int64), tok_inst=np.full(Tb, -1, np.int64),
               blk_rows=np.zeros(Tb, bool), row_ty=np.zeros(Tb, np.int64), unit_row0=units[:U].copy(), units=units)
    for n, (unit, ty, is_blk, row) in enumerate(rows):
        out['ids'][n], out['kve'][n], out['rot'][n], out['tok_inst'][n] = row[0], row[2], row[3], row[4]
        out['pos'][n] = unit * cap + row[1]
        out['blk_rows'][n], out['row_ty'][n] = is_blk, ty
    return out


def random_mirror(rng):
    """(A, H, n_t, Lc, cap): H in {1, 2}, B in 1 .. 6, Lc in 1 .. 9, every phase mix; `som_pending` only on modality-phase samples at ode_k = 0 under guidance,
    `commit_pending` only on text-phase samples under guidance"""
    H, B, Lc, n_t = int(rng.integers(1, 3)), int(rng.integers(1, 7)), int(rng.integers(1, 10)), int(rng.integers(3, 10))
    samples = []
    for i in range(B):
        ph = int(rng.integers(0, 3))
        s = dict(phase=ph, cache_len=int(rng.integers(1, 60)), tokens_seen=int(rng.integers(1, 60)), last_token=int(rng.integers(0, 70)),
                 length=int(rng.integers(0 if ph == DONE else 1, Lc + 1)), type=int(rng.integers(0, 3)))
        if ph == MOD:
            s['ode_k'] = int(rng.integers(0, n_t - 1))
        if H == 2:
            s.update(uncond_len=int(rng.integers(1, 60)), uncond_pos=int(rng.integers(1, 60)))
            if ph == MOD and s['ode_k'] == 0:
                s['som_pending'] = int(rng.integers(0, 2))
            if ph == TEXT:
                s['commit_pending'] = int(rng.integers(0, 2))
        samples.append(s)
    A = mirror(*samples)
    cap = int(max(A[F['cache_len']].max(), A[F['uncond_len']].max())) + Lc + 3 + int(rng.integers(0, 64))
    return A, H, n_t, Lc, cap


def edge_mirrors():
    """hand-written steps: (name, A, H, n_t, Lc, cap, bucket of the compacted layout)"""
    t = lambda **k: dict(phase=TEXT, **k)
    m = lambda **k: dict(phase=MOD, **k)
    d = lambda **k: dict(phase=DONE, **k)
    return [
        ('all done but one', mirror(d(cache_len=9, uncond_len=8, length=4), d(cache_len=1, uncond_len=1), m(cache_len=5, uncond_len=4, tokens_seen=5, uncond_pos=4, length=3, ode_k=1, type=1),
                                    d(cache_len=30, uncond_len=31, length=2)), 2, 5, 4, 64, 8),
        ('B = 1, guidance, pending [som]', mirror(m(cache_len=4, uncond_len=4, tokens_seen=4, uncond_pos=4, length=2, som_pending=1)), 2, 3, 2, 16, 4),
        ('B = 1, no guidance', mirror(m(cache_len=4, tokens_seen=4, length=2, ode_k=2)), 1, 4, 2, 16, 4),
        ('L = Lc and L = 1 side by side', mirror(m(cache_len=7, uncond_len=8, tokens_seen=6, uncond_pos=7, length=9, ode_k=3), m(cache_len=2, uncond_len=2, tokens_seen=2, uncond_pos=2, length=1, type=1),
                                                  t(cache_len=12, uncond_len=3, tokens_seen=11, uncond_pos=3, last_token=5, length=1, commit_pending=1, type=1)), 2, 7, 9, 40, 16),
        ('not a mixed step (Lq = 1)', mirror(t(cache_len=3, uncond_len=3, tokens_seen=3, uncond_pos=3, last_token=9, length=4), d(cache_len=6, uncond_len=6, length=4),
                                             t(cache_len=1, uncond_len=1, tokens_seen=1, uncond_pos=1, last_token=2)), 2, 5, 4, 32, 8),
        # compacted rows: the real half 3 + 1, the null-text half 3 + 1 = 8, exactly the bucket ...
        ('row count exactly the bucket', mirror(m(cache_len=5, uncond_len=5, tokens_seen=5, uncond_pos=5, length=3), t(cache_len=2, uncond_len=2, tokens_seen=2, uncond_pos=2, last_token=1)), 2, 3, 3, 16, 8),
        # ... and with the pending [som] one over it
        ('row count one over the bucket', mirror(m(cache_len=5, uncond_len=5, tokens_seen=5, uncond_pos=5, length=3, som_pending=1), t(cache_len=2, uncond_len=2, tokens_seen=2, uncond_pos=2, last_token=1)), 2, 3, 3, 16, 8),
    ]
