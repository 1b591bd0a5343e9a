"""The attention kernels per element against the derived bounds of tests/_attn_bounds.py (no measured tolerances): the eight plan slots tfx_qk_norm_rope_fwd
writes on both sides of every mode threshold; a forward FUNCTION probe - one score per row, placed on the end points of every soft-cap branch, in the saturated
range and in waves that one row pushes to the exact form - through tfx_attn_fwd without and with a plan, against a KV cache (the per-row form) and through
tfx_decode_attn's rows kernel; a DERIVATIVE probe whose dq element scales one to one with the soft-cap derivative, through tfx_attn_bwd in plan modes none / 0 /
1; and the layout catalogue's sentinel cases, every output element.  Outputs sit in guard bands.  Every test prints BOUND <test> <output> <worst error / bound>;
an MI355X run is kept in profiles/attn_bounds.txt.  b <= 4, h = 2, n <= 200 but for the catalogue's n1000."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_bounds as A  # noqa: E402
from _attn_cases import CAP, CASES, exact_input_reference, run_kernels  # noqa: E402
from _gemm_cases import BF, GUARD, PAD, assert_elementwise, assert_untouched, guarded, padded  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _capi():
    from transfusion_pytorch_amd import capi
    return capi, torch.cuda.current_stream().cuda_stream


def tok(x):
    """(b, h, n, d) -> token-major (b n, h d)"""
    b, h, n, d = x.shape
    return x.transpose(1, 2).reshape(b * n, h * d)


def untok(x, b, n, h):
    return x.float().reshape(b, n, h, -1).transpose(1, 2)


# ---------------------------------------------------------------------------------------------- plan coefficients
def write_plan(gains):
    """tfx_qk_norm_rope_fwd on eight rows with the given (gq, gk, norm_scale, q_scale) (gq None: no RMS normalisation): the eight slots, between guards"""
    capi, st = _capi()
    gq, gk, ns, qs = gains
    T, h = 8, 2
    HD = h * 64
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(T, 2 * HD + 8, generator=g).to(BF).to(DEV)
    qk = torch.zeros(T, 2 * HD, device=DEV, dtype=BF)
    buf, view = guarded(1, 8, torch.float32, DEV)
    before = buf.clone()
    dgq, dgk = (None if x is None else x.to(DEV) for x in (gq, gk))             # (the argument struct holds raw pointers: every tensor stays alive in a local)
    pos, cos_t, sin_t = torch.zeros(T, device=DEV, dtype=torch.int32), torch.ones(8, 32, device=DEV), torch.zeros(8, 32, device=DEV)
    a = capi.make_args('tfx_qk_norm_rope_args', T=T, H=h, qkv=qkv, ld_qkv=2 * HD + 8, qk=qk, ld_qk=2 * HD, gamma_q=dgq, gamma_k=dgk, rot_pos=pos, cos_tab=cos_t,
                       sin_tab=sin_t, q_scale=qs, norm_scale=ns, sc_plan=view, softcap=CAP)
    capi.call('tfx_qk_norm_rope_fwd', a, st)
    torch.cuda.synchronize()
    written = torch.zeros_like(buf, dtype=torch.bool)
    written[GUARD, :8] = True
    assert_untouched('sc_plan', buf, before, written)
    return view[0].clone()


PLAN_POINTS = [(0.05, 0, 0), (0.2, 0, 0), (0.2, 1, 1), (0.3, 0, 1), (0.35, 0, 1), (0.35, 1, 2), (0.5, 0, 2)]      # (B / cap, fp32 steps of the largest gain, mode)


def test_plan_slots_match_plan_ref():
    """All eight slots on both sides of 0.2 and 0.35 - one fp32 step of the largest gain apart -, mid-range, and without gains.  The mode and B are exact (B
    is formed in fp32 in the header's order, the mode is a comparison of it); a coefficient slot is a sum of at most three terms of at most 14 fp32 roundings
    each (b^2 three, its cube eleven, 1 / cap^2 two, log2 e and the rational constants one each): |slot - plan_ref| <= 16 u32 x the sum of its terms' magnitudes."""
    worst = 0.
    for bx, step, mode in PLAN_POINTS + [(None, 0, 2)]:
        gains = (None, None, 8., 0.125) if bx is None else A.gains_for(bx, step=step)
        ref = A.plan_ref(gains[0], gains[1], gains[2], gains[3], CAP)
        got = write_plan(gains).cpu().double()
        assert ref.mode == mode, (bx, step, ref.mode)
        assert int(got[0]) == mode and float(got[0]) == float(mode), (bx, step, got.tolist())
        assert float(got[7]) == ref.B, (bx, step, float(got[7]), ref.B)
        if bx is not None:
            assert (A.f32(ref.B) / A.f32(CAP) > A.f32(bx)) == (step > 0) and abs(ref.bx - bx) <= 2e-6 * bx, (bx, step, ref.bx)     # one fp32 step of the gain apart
        err = (got[1:7] - ref.slots[1:7]).abs()
        over = err > ref.slot_tol[1:7]
        assert not bool(over.any()), (bx, step, got.tolist(), ref.slots.tolist())
        worst = max(worst, float((err / ref.slot_tol[1:7].clamp_min(1e-300)).max()))
    print(f'BOUND plan slots {worst:.3f}')


# ---------------------------------------------------------------------------------------------- one launch between guards
def launch(P, entry='tfx_attn_fwd', plan=None, q_start=None, label=''):
    """the problem's bf16 values in padded token-major buffers (1e4 behind every row), every output in a guarded buffer; tfx_attn_fwd / tfx_decode_attn, then
    tfx_attn_bwd when the problem has a dout.  Keys are a cache of P.nk rows per sample when the problem's path says so.  Returns (b, h, n, ...) fp32 tensors."""
    capi, st = _capi()
    b, h, n, nk = P.b, P.h, P.n, P.nk
    T, HD = b * n, h * 64
    cache = P.path in ('row', 'rows')
    (_, q), (_, k), (_, v) = (padded(tok(x).to(BF).to(DEV)) for x in (P.q, P.k, P.v))
    ld = HD + GUARD
    gate = torch.full((T, 8), PAD, dtype=BF, device=DEV)
    gate[:, :h] = P.gate.transpose(1, 2).reshape(T, h).to(BF).to(DEV)
    kv_end = P.kv_end.reshape(-1).to(torch.int32).to(DEV)
    bufs = {'out': guarded(T, HD, BF, DEV), 'lse': guarded(1, b * h * n, torch.float32, DEV)}
    kw = dict(q=q, k=k, v=v, ld_q=ld, ld_k=ld, ld_v=ld, gate=gate, ld_gate=8, kv_end=kv_end, q_start=kv_end if q_start is None else q_start.reshape(-1).to(torch.int32).to(DEV),
              b=b, h=h, n=n, softcap=P.cap, n_kv=nk if cache else 0, sc_plan=plan)
    bwd = P.dout is not None
    if bwd:
        bufs.update({name: guarded(T, HD, BF, DEV) for name in ('do_eff', 'dq', 'dk', 'dv')})
        bufs.update(delta=guarded(1, b * h * n, torch.float32, DEV), dgate=guarded(T, 8, BF, DEV, 0))
        (_, dout) = padded(tok(P.dout).to(BF).to(DEV))
        kw.update(dout=dout, ld_dout=ld, do_eff=bufs['do_eff'][1], ld_do=ld, delta=bufs['delta'][1], dgate=bufs['dgate'][1], ld_dgate=8, dq=bufs['dq'][1],
                  dk=bufs['dk'][1], dv=bufs['dv'][1], ld_dq=ld, ld_dk=ld, ld_dv=ld)
    before = {name: buf.clone() for name, (buf, _) in bufs.items()}
    a = capi.make_args('tfx_attn_args', out=bufs['out'][1], ld_out=ld, lse=bufs['lse'][1], **kw)
    capi.call(entry, a, st)
    if bwd:
        capi.call('tfx_attn_bwd', a, st)
    torch.cuda.synchronize()
    got = {}
    for name, (buf, view) in bufs.items():
        written = torch.zeros_like(buf, dtype=torch.bool)
        if name in ('lse', 'delta'):
            written[GUARD, :b * h * n] = True
            got[name] = view[0].reshape(b, h, n).clone()
        elif name == 'dgate':
            written[GUARD:GUARD + T, :h] = True
            got[name] = view[:, :h].float().reshape(b, n, h).transpose(1, 2)
        else:
            written[GUARD:GUARD + T, :HD] = True
            got[name] = untok(view, b, n, h)
        assert_untouched(f'{label} {name}', buf, before[name], written)
    return got


def check(label, P, got, bounds):
    """every element of every output against its bound; prints the BOUND line of every output, then raises for the ones over"""
    fails = []
    for name, (ref, tol) in bounds.items():
        d = ref.shape[-1] if ref.dim() == 4 else 1
        worst, over, where = A.ratios({name: got[name]}, {name: (ref, tol)})[name]
        print(f'BOUND {label} {name} {worst:.3f}')
        try:
            assert_elementwise(f'{label} {name}', got[name].reshape(-1, d), ref.reshape(-1, d), tol.reshape(-1, d), tile=(P.n, 64))
        except AssertionError as e:
            fails.append(f'{e} [b, h, row, col {where}]')
    assert not fails, '\n'.join(fails)


def on_dev(P):
    for key in ('q', 'k', 'v', 'gate', 'kv_end', 'dout'):
        if getattr(P, key) is not None:
            setattr(P, key, getattr(P, key).to(DEV))
    return P


def probe_plan(mode):
    """(the float64 plan, the kernel-written fp32 slots on the device) of gains whose B / cap sits a step under the mode's threshold; (None, None) without"""
    if mode is None:
        return None, None
    gains = A.gains_for(A.PLAN_THRESH[mode])
    ref = A.plan_ref(gains[0], gains[1], gains[2], gains[3], CAP)
    assert ref.mode == mode
    return ref, write_plan(gains)


# ---------------------------------------------------------------------------------------------- forward function probe
@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('path', ['wave', 'row'])
def test_forward_function_probe(path, mode):
    """tfx_attn_fwd on the probe of _attn_bounds.fwd_probe: lse[i] = cap tanh(s_i / cap) + ln(m_i) and out = sigmoid(gate) v in closed form, per element.
    'wave': the training launch (the form follows the wave's largest score, or the plan); 'row': against a KV cache of 200 rows (the per-row form).  With a plan
    the scores fill [-B, B] and 16 rows per sample and head reach >= 0.95 B, B itself included.  The end points of a branch are the nearest scores of the
    two-column grid on either side of the kernel's fp32 threshold - about 2^-17 relative away (some 100 fp32 ulps), not the threshold's fp32 neighbours: q and k
    keep to two non-zero bf16 columns so that the score is exact."""
    ref, slots = probe_plan(mode)
    P = on_dev(A.fwd_probe(ref, path, n_kv=200 if path == 'row' else 0))
    got = launch(P, 'tfx_attn_fwd', slots, label=f'fwd probe {path}')
    bounds = A.forward_bounds(P)
    if path == 'wave':
        assert float((bounds['lse'][0] - A.closed_form_lse(P)).abs().max()) <= 1e-12
    check(f'fwd_probe[{path},plan={mode}]', P, got, bounds)


@pytest.mark.parametrize('R', [1, 2])
def test_forward_function_probe_rows_kernel(R):
    """tfx_decode_attn with one and two rows per sample (decode_attn_rows_k: its own copy of the exact form): the probe's 192 scores per sample and head, R
    rows of every sample per launch, against a cache of 200 keys.  A plan is passed as the engine passes it on half of the launches; the rows kernel ignores it."""
    ref, slots = probe_plan(0)
    P = on_dev(A.fwd_probe(None, 'rows', n_kv=200))
    bounds = A.forward_bounds(P)
    got = {'out': torch.zeros(P.b, P.h, P.n, 64, device=DEV), 'lse': torch.zeros(P.b, P.h, P.n, device=DEV)}
    for i, r0 in enumerate(range(0, P.n, 2)):
        rows = slice(r0, r0 + R)
        sub = A.problem(P.q[:, :, rows], P.k, P.v, P.gate[:, :, rows], P.kv_end[:, rows], path='rows')
        g = launch(sub, 'tfx_decode_attn', slots if i % 2 else None, label=f'rows kernel R={R}')
        got['out'][:, :, rows], got['lse'][:, :, rows] = g['out'], g['lse']
    keep = torch.zeros(P.n, dtype=torch.bool, device=DEV)
    keep[0::2] = True
    if R == 2:
        keep[:] = True
    sel = {k: (r[:, :, keep], t[:, :, keep]) for k, (r, t) in bounds.items()}
    check(f'fwd_probe[rows,R={R}]', P, {k: v[:, :, keep] for k, v in got.items()}, sel)


# ---------------------------------------------------------------------------------------------- derivative probe
@pytest.mark.parametrize('mode', [None, 0, 1])
def test_derivative_probe(mode):
    """tfx_attn_fwd + tfx_attn_bwd on _attn_bounds.deriv_probe: dq_i[0] carries the soft-cap derivative one to one (every term of its sum has the same sign).
    Mode none walks every polynomial range, its thresholds and the exact form above 0.45 cap (1 - (s2 / cap2)^2 from each form); modes 0 / 1 fill [-B, B].  One
    sample is pure causal, one has blocks across the 32-key boundaries 32 and 128 (the masked and the interior instance of dkv_scores both see swept scores),
    one is a single block.  dq, dk, dv, do_eff, delta, dgate - and out, lse - per element."""
    ref, slots = probe_plan(mode)
    P, q_start = A.deriv_probe(ref)
    P = on_dev(P)
    got = launch(P, 'tfx_attn_fwd', slots, q_start=q_start, label='derivative probe')
    bounds = A.forward_bounds(P)
    bounds.update(A.backward_bounds(P, got))
    check(f'deriv_probe[plan={mode}]', P, got, bounds)
    edge = (P.q[..., :2].sum(-1).abs() >= (0.95 * ref.B if ref is not None else 0.45 * CAP))
    assert int(edge.sum()) >= 16 and float(bounds['dq'][0][..., 0][edge].abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the layout catalogue, every element
def _catalogue(name, mode, laser):
    case = CASES[name]
    inp, qk, got = run_kernels(case, mode, laser=laser)
    P, _, _ = A.catalogue_problem(name, mode, qk=qk, inp=inp, laser=laser, vl=got.get('vl'))
    bounds = A.forward_bounds(P)
    bounds.update(A.backward_bounds(P, got))
    ex = exact_input_reference(inp, case, qk, got, laser=laser, dev=DEV)
    for key, (ref, _) in bounds.items():
        assert float((ref - ex[key]).abs().max()) <= 1e-9 * max(1., float(ex[key].abs().max())), key
    check(f'catalogue[{name},plan={mode}{",laser" if laser else ""}]', P, got, bounds)


@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('name', ['n5', 'n200'] + [c.name for c in CASES.values() if c.sub])
def test_catalogue_per_element(name, mode):
    """run_kernels() on the sentinel inputs (its poisoned outputs and guard columns included): every element of out, lse, do_eff, delta, dgate, dq, dk, dv
    against its bound, next to the per-row sweep of tests/test_attention_layouts_gpu.py.  The reference is exact_input_reference()'s."""
    _catalogue(name, mode, False)


@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('name', [c.name for c in CASES.values() if c.sub])
def test_catalogue_per_element_laser(name, mode):
    """the same through tfx_laser_v_fwd -> the LASER forms -> tfx_laser_v_bwd: og = g log(P v'), the prep kernel's exp(-L), d v' stored in bf16 and taken to dv"""
    _catalogue(name, mode, True)
