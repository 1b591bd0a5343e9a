"""Decode attention against a KV cache over the visible-length catalogue of tests/_decode_attn_cases.py: the matrix-core-free rows kernel behind
tfx_decode_attn (one and two new rows per sample), the tiled forward kernel with cache addressing (tfx_attn_fwd with n_kv > 0; dense and
compacted rows), each plain and reading the LASER side cache of v', with the soft-cap plan passed exactly as the engine passes it.  Sentinel
inputs: one key more or less on any row moves it by O(1) (proved on the CPU: tests/test_decode_attn_cases_cpu.py).  Per case: tfx_qk_norm_rope_fwd
on the new rows and on the cache rows -> cache buffer k~ | v of the engine's layout -> [tfx_laser_v_fwd over the cache] -> the attention launch;
per-row out / lse against fp64 from the kernels' own bf16 inputs, poisoned outputs, padding and rows no unit owns.  Then the bit-identity the
continuous decode schedule rests on: a row comes out the same whichever launch shape carried it."""
import functools

import pytest
import torch

from _decode_attn_cases import (CAP, CASES, COMPACT, LASER_C, PAIRS, POISON, ROWS_CASES, TILED_CASES, build_decode_inputs, decode_reference,
                                heads, round_bf16, row_err, row_tol)

pytestmark = pytest.mark.gpu
DEV, BF = 'cuda', torch.bfloat16


def _capi():
    from transfusion_pytorch_amd import capi
    return capi, torch.cuda.current_stream().cuda_stream


def _norm(x, h, inp, want_mode):
    """tfx_qk_norm_rope_fwd at identity rotation on rows x (T, h 64) bf16, standing in both the q and the k columns: (q~ | k~ (T, 2 h 64), plan)"""
    capi, st = _capi()
    T, HD = x.shape[0], h * 64
    raw = torch.cat([x, x], 1).contiguous()
    qk = torch.zeros(T, 2 * HD, device=DEV, dtype=BF)
    plan = torch.full((8,), float('nan'), device=DEV)
    gq, gk, pos = inp['gq'].to(DEV), inp['gk'].to(DEV), torch.zeros(T, device=DEV, dtype=torch.int32)      # (the argument block holds addresses only)
    cos_t, sin_t = torch.ones(8, 32, device=DEV), torch.zeros(8, 32, device=DEV)
    a = capi.make_args('tfx_qk_norm_rope_args', T=T, H=h, qkv=raw, ld_qkv=2 * HD, qk=qk, ld_qk=2 * HD, gamma_q=gq, gamma_k=gk, rot_pos=pos,
                       cos_tab=cos_t, sin_tab=sin_t, q_scale=inp['q_scale'], norm_scale=inp['norm_scale'], sc_plan=plan, softcap=CAP)
    capi.call('tfx_qk_norm_rope_fwd', a, st)
    torch.cuda.synchronize()
    assert int(plan[0].item()) == want_mode, (want_mode, plan.tolist())
    return qk, plan


@functools.lru_cache(maxsize=None)
def prepared(name, mode):
    """a case's inputs as the attention launch reads them (built once per (case, gains mode), shared by every test, never written again): q~ of the
    flat query rows (ld 2 h 64), the cache k~ | raw v [b n_kv, 2 h 64], the side cache of v' [b n_kv, h 64], bf16 gate logits, kv_end, the plan"""
    capi, st = _capi()
    case = CASES[name]
    inp = round_bf16(build_decode_inputs(case, mode))
    h, HD, want = case.h, case.h * 64, 2 if mode is None else mode
    qn, plan = _norm(inp['q'].to(DEV).to(BF), h, inp, want)
    kn, plan_k = _norm(inp['k'].to(DEV).to(BF), h, inp, want)
    assert torch.equal(plan[:7], plan_k[:7])
    Tk = case.b * case.n_kv
    cache = torch.cat([kn[:, HD:], inp['v'].to(DEV).to(BF)], 1).contiguous()
    side = torch.zeros(Tk, HD, device=DEV, dtype=BF)
    la = capi.make_args('tfx_laser_v_args', T=Tk, H=h, v=cache[:, HD:], ld_v=2 * HD, vl=side, ld_vl=HD, c=LASER_C)
    capi.call('tfx_laser_v_fwd', la, st)
    torch.cuda.synchronize()
    ldg = (h + 7) // 8 * 8 + 8
    gate = torch.zeros(case.R, ldg, device=DEV, dtype=BF)
    gate[:, :h] = inp['gate'].to(DEV).to(BF)
    return dict(case=case, q=qn, cache=cache, side=side, gate=gate, kv_end=inp['kv_end'].to(DEV), plan=None if mode is None else plan)


def attn(entry, P, laser, q, gate, kv_end, b, lq, units=None):
    """one attention launch against P's cache: q (R, >= h 64) bf16 with its own ld, gate (R, ld) bf16, kv_end (R,) int32.  out has ld > h 64 and
    starts as POISON, lse as NaN.  Returns (out (R, ld_out), lse (b, h, lq))"""
    capi, st = _capi()
    case = P['case']
    h, HD = case.h, case.h * 64
    R = q.shape[0]
    out = torch.full((R, HD + 24), POISON, device=DEV, dtype=torch.int16).view(BF)
    lse = torch.full((b, h, lq), float('nan'), device=DEV)
    kw = dict(q=q, k=P['cache'], v=P['side'] if laser else P['cache'][:, HD:], ld_q=q.stride(0), ld_k=2 * HD, ld_v=HD if laser else 2 * HD,
              gate=gate, ld_gate=gate.stride(0), kv_end=kv_end, q_start=torch.zeros(R, device=DEV, dtype=torch.int32), out=out, ld_out=HD + 24,
              lse=lse, b=b, h=h, n=lq, n_kv=case.n_kv, softcap=CAP, sc_plan=P['plan'], laser=int(laser))
    if units:
        kw.update(q_row0=torch.tensor(units[0], dtype=torch.int32, device=DEV), q_cnt=torch.tensor(units[1], dtype=torch.int32, device=DEV))
    capi.call(entry, capi.make_args('tfx_attn_args', **kw), st)
    torch.cuda.synchronize()
    return out, lse


def bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


def check_case(path, entry, P, mode, laser, case=None):
    """the launch of `case` (default: P's own; or a case over the same flat rows and cache samples) held to the fp64 reference from the kernel's
    own bf16 q~ | k~ and values, row by row in every head; owned elements finite; padding, rows and lse slots the launch does not own keep their bits"""
    case = case or P['case']
    h, HD = case.h, case.h * 64
    out, lse = attn(entry, P, laser, P['q'], P['gate'], P['kv_end'], case.b, case.lq, case.units)
    ref = decode_reference(case, P['q'][:, :HD], P['cache'][:, :HD], P['side'] if laser else P['cache'][:, HD:], P['gate'], P['kv_end'],
                           laser=laser, vprime=True)
    owned = torch.zeros(case.R, dtype=torch.bool, device=DEV)
    worst, worst_lse, where = 0., 0., None
    for s, r0, c in case.spans():
        assert bool(torch.isnan(lse[s, :, c:]).all()), f'{case.name}: lse slots past unit {s} were written'
        if c == 0:
            continue
        owned[r0:r0 + c] = True
        got = heads(out[r0:r0 + c].float(), 1, c, h)
        assert torch.isfinite(got).all() and torch.isfinite(lse[s, :, :c]).all(), f'{case.name}: unit {s} has unwritten or non-finite elements'
        e_out = row_err(got, ref[s][0])[0]
        e_lse = (lse[s, :, :c].double() - ref[s][1][0]).abs()
        if float(e_out.max()) > worst:
            hh, r = (int(i) for i in torch.nonzero(e_out == e_out.max())[0])
            worst, where = float(e_out.max()), (s, hh, r, case.kv_end[s][r])
        worst_lse = max(worst_lse, float(e_lse.max()))
    assert bool((bits(out[:, HD:]) == POISON).all()), f'{case.name}: the ld padding of out was written'
    assert bool((bits(out[~owned]) == POISON).all()), f'{case.name}: rows owned by no unit were written'
    tol = row_tol(laser)
    print(f'DECERR {path} {entry} {case.name} mode={mode} laser={int(laser)} out={worst:.2e}@{where} lse={worst_lse:.2e}')
    assert worst <= tol['out'] and worst_lse <= tol['lse'], (case.name, mode, laser, worst, where, worst_lse)


def _param(cases, modes):
    return [(c.name, m, laser) for c in cases for laser in ((False, True) if c.sub else (False,)) for m in modes]


@pytest.mark.parametrize('name,mode,laser', _param(ROWS_CASES, (None, 0)))
def test_rows_kernel(name, mode, laser):
    """tfx_decode_attn with one / two rows per sample; the plan is passed as the engine passes it, the rows kernel ignores it"""
    check_case('rows', 'tfx_decode_attn', prepared(name, mode), mode, laser)


@pytest.mark.parametrize('name,mode,laser', _param(TILED_CASES, (None, 0, 1)))
def test_tiled_kernel_against_the_cache(name, mode, laser):
    check_case('tiled', 'tfx_attn_fwd', prepared(name, mode), mode, laser)


@pytest.mark.parametrize('mode,laser', [(None, False), (0, False), (1, True)])
def test_decode_entry_hands_three_rows_and_more_to_the_tiled_kernel(mode, laser):
    check_case('tiled', 'tfx_decode_attn', prepared('t7', mode), mode, laser)


@pytest.mark.parametrize('name,mode,laser', _param([COMPACT], (None, 0, 1)))
def test_tiled_kernel_compacted_rows(name, mode, laser):
    check_case('compact', 'tfx_attn_fwd', prepared(name, mode), mode, laser)


@pytest.mark.parametrize('mode,laser', [(None, False), (0, False), (1, False), (0, True)])
def test_decode_entry_compacted_units_of_one_and_two_rows(mode, laser):
    """tfx.h tfx_decode_attn: a compacted call goes to the tiled kernel whatever n is.  The catalogue's one-row, zero-row and two-row units in a
    launch with n = 2: the rows kernel, which addresses rows b * n .., would compute flat rows 0 .. 5 instead of 3, 10 and 11"""
    row0, cnt, R = COMPACT.units
    small = COMPACT._replace(name='compact_n2', lq=2, kv_end=COMPACT.kv_end[:3], units=(row0[:3], cnt[:3], R))
    check_case('compact', 'tfx_decode_attn', prepared('compact', mode), mode, laser, case=small)


# ---------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize('laser', [False, True])
def test_rows_kernel_bits_do_not_depend_on_the_partner_row(laser):
    """decode.hip: "a row's arithmetic does not depend on R or on the other rows of its block".  Every row of the 'pairs' case (query, sample cache,
    visible length, gate) alone in an n = 1 launch, against the same row as row 0 and as row 1 of an n = 2 launch beside a partner that sees 1
    key and beside one that sees the whole cache"""
    for mode in (None, 0):
        P = prepared('pairs', mode)
        b, n_kv, HD = PAIRS.b, PAIRS.n_kv, PAIRS.h * 64
        q, gate, ke = P['q'].view(b, 2, -1), P['gate'].view(b, 2, -1), P['kv_end'].view(b, 2)
        for j in (0, 1):
            out1, lse1 = attn('tfx_decode_attn', P, laser, q[:, j].contiguous(), gate[:, j].contiguous(), ke[:, j].contiguous(), b, 1)
            assert torch.isfinite(out1[:, :HD].float()).all() and torch.isfinite(lse1).all()
            for pos in (0, 1):
                for partner in (1, n_kv):
                    idx = [j, 1 - j] if pos == 0 else [1 - j, j]
                    ke2 = ke[:, idx].clone()
                    ke2[:, 1 - pos] = partner
                    out2, lse2 = attn('tfx_decode_attn', P, laser, q[:, idx].reshape(2 * b, -1), gate[:, idx].reshape(2 * b, -1), ke2.reshape(-1), b, 2)
                    assert torch.equal(bits(out2.view(b, 2, -1)[:, pos, :HD]), bits(out1[:, :HD])), (mode, j, pos, partner, 'out')
                    assert torch.equal(bits(lse2[:, :, pos]), bits(lse1[:, :, 0])), (mode, j, pos, partner, 'lse')


@pytest.mark.parametrize('laser', [False, True])
@pytest.mark.parametrize('mode', [None, 0, 1])
def test_tiled_kernel_bits_do_not_depend_on_the_launch_shape(mode, laser):
    """engine.py Plan: "a token must come out of the same arithmetic whichever plan carried it" (the continuous decode schedule runs a sample's
    token in plans of different row counts).  Rows of the 't49' case - beside rows that see more and fewer keys - against the same row carried by
    tfx_attn_fwd alone (lq 1), as one of two rows (lq 2, either position) and inside a three-row compacted unit at an odd row0.  Twice: with the
    sentinel queries as they are (every row of a wave reaches the same scores), and with the rows under test scaled to an eighth, quiet rows
    beside loud ones: whatever a wave decides from its largest score must not reach the arithmetic of its other rows"""
    P = prepared('t49', mode)
    case = P['case']
    b, lq, HD = case.b, case.lq, case.h * 64
    rounds = [(10, 0, 31), (7, 5, 33), (48, 20, 0)]                                       # one row per sample and round
    differ = []
    for quiet in (False, True):
        q = P['q']
        if quiet:
            q = q.clone()
            for rows in rounds:
                for s, r in enumerate(rows):
                    q[s * lq + r] *= 0.125
        out49, lse49 = attn('tfx_attn_fwd', P, laser, q, P['gate'], P['kv_end'], b, lq)
        assert torch.isfinite(out49[:, :HD].float()).all() and torch.isfinite(lse49).all()
        for k_, rows in enumerate(rounds):
            want_out = torch.stack([out49[s * lq + r, :HD] for s, r in enumerate(rows)])
            want_lse = torch.stack([lse49[s, :, r] for s, r in enumerate(rows)])

            def carry(offsets, pos, units=None, R=None):
                """every sample carries rows r + offsets (mod lq) of its own, the row under test at `pos`"""
                flat = [[s * lq + (r + o) % lq for o in offsets] for s, r in enumerate(rows)]
                n = len(offsets)
                if units:
                    sel = torch.zeros(R, dtype=torch.long)
                    for s, r0 in enumerate(units):
                        sel[r0:r0 + n] = torch.tensor(flat[s])
                    at = [r0 + pos for r0 in units]
                    u = (units, (n,) * b)
                else:
                    sel, at, u = torch.tensor(flat).reshape(-1), [s * n + pos for s in range(b)], None
                sel = sel.to(DEV)
                out, lse = attn('tfx_attn_fwd', P, laser, q[sel], P['gate'][sel], P['kv_end'][sel].contiguous(), b, n, u)
                for what, got, want in (('out', out[at, :HD], want_out), ('lse', lse[:, :, pos], want_lse)):
                    if not torch.equal(bits(got), bits(want)):
                        differ.append((what, 'quiet' if quiet else 'loud', rows, offsets, units,
                                       [s for s in range(b) if not torch.equal(bits(got[s]), bits(want[s]))]))
            carry((0,), 0)
            carry((0, 1), 0) if k_ % 2 else carry((-1, 0), 1)
            carry((-1, 0, 1), 1, units=(1, 7, 11), R=16)
    assert not differ, f'mode {mode} laser {laser}: (what, row under test, rows, carried offsets, units, samples that differ) {differ}'
