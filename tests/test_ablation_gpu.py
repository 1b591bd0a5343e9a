"""The two attention ablations on the MI355X: Transformer(qk_rmsnorm=False) (reference T:948-952; NULL gains in the C ABI) and
Transformer(attn_kwargs=dict(gate_values=False)) (T:901-904, T:1026-1027; tfx_attn_args.gate == NULL), include/tfx.h.

Kernel level, against the float64 restatements of tests/_ablation_cases.py under the bounds of tests/_tokenwise_cases.py, tests/_attn_cases.py and
tests/_decode_attn_cases.py, every output guarded or poisoned: the no-norm QK + RoPE forward and backward; the fused projection epilogue and the
attention backward's nr_* epilogues with NULL gains, bit for bit against the separate launches; tfx_attn_fwd / tfx_attn_bwd / tfx_decode_attn with
gate = NULL, also bit for bit against the same call with gate logits of 3e4 (sigmoid exactly 1 in fp32); unnormalised scores far outside any
polynomial plan's range.
Model level: the reference's fixtures (tools/make_golden_ablation.py) under the gates of tests/test_model_gpu.py / tests/test_laser_gpu.py."""
import ctypes
import os

import pytest
import torch

import test_decode_attn_edges_gpu as dec
from _ablation_cases import (ATTN_CASES, BOTH, FIXTURES, LASER_FIXTURES, NOGATE, NOQK, SAMPLING_FIXTURE, TEXT_FIXTURE, TRAIN_FIXTURES, build_nonorm_qk,
                             exact_input_reference, loud_inputs, metrics, nogate_reference, outs_nonorm_qk, row_tol, run_attention, run_decode,
                             strip_state, transformer_kwargs)
from _decode_attn_cases import CASES as DECODE_CASES, COMPACT, PAIRS, POISON, decode_reference, heads, row_err
from _tokenwise_cases import QK_STRIDE, check_outs, rope_carries

pytestmark = pytest.mark.gpu
DEV, BF = 'cuda', torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOSS_TOL, LOGIT_TOL, GRAD_TOL, GRAD_MEAN_TOL = 1e-3, 1e-2, 4e-2, 1.2e-2                          # tests/test_model_gpu.py, DESIGN section 1
NEAR_TIE = 0.05


def bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF else torch.int32)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _capi():
    from transfusion_pytorch_amd import capi
    return capi, torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- kernels: QK + RoPE without the norm
@pytest.mark.parametrize('T,H,dh', [(70, 3, 64), (2800, 6, 64), (70, 3, 8)], ids=['T70-H3', 'T2800-H6-second_trip_carry', 'T70-H3-dim_head8'])
def test_qk_rope_without_the_norm(T, H, dh):
    """tfx_qk_norm_rope_fwd / _bwd with NULL gains per element against float64; the pad behind the rows and the gain-gradient sentinels keep their bits;
    the plan buffer reads mode 2 with B = +inf.  (2800, 6): the second trip of the backward's 32768-vector grid stride, with its carry."""
    capi, st = _capi()
    assert rope_carries(T, H) == (T == 2800) and (T * 2 * H > QK_STRIDE) == (T == 2800)
    c = build_nonorm_qk(T, H, dh, DEV)
    o = outs_nonorm_qk(c)
    plan = torch.full((8,), float('nan'), device=DEV)
    a = capi.make_args('tfx_qk_norm_rope_args', T=T, H=H, qkv=c.qkv, ld_qkv=c.ld, qk=o.qk.view, ld_qk=c.ld_qk, gamma_q=None, gamma_k=None, rot_pos=c.pos,
                       cos_tab=c.cos, sin_tab=c.sin, q_scale=c.q_scale, dqk=c.dqk, ld_dqk=2 * c.HD, dqkv=o.dqkv.view, ld_dqkv=c.ld_qk,
                       dgamma_q=o.dgamma_q.view, dgamma_k=o.dgamma_k.view, sc_plan=plan, softcap=50.0)
    capi.call('tfx_qk_norm_rope_fwd', a, st); capi.call('tfx_qk_norm_rope_bwd', a, st)
    torch.cuda.synchronize()
    rep = check_outs(f'qk_rope T={T} H={H} dh={dh}', [o.qk, o.dqkv, o.dgamma_q, o.dgamma_k])
    print(f'NONORM-QK T={T} H={H} dh={dh} worst error / bound ' + ' '.join(f'{k}={v:.3f}' for k, v in rep.items()))
    assert int(plan[0].item()) == 2 and plan[7].item() == float('inf') and torch.isfinite(plan[:7]).all(), plan.tolist()
    if dh < 64:
        dead = (torch.arange(2 * c.HD, device=DEV) % 64) >= dh
        assert bool((o.qk.view[:, :2 * c.HD][:, dead] == 0).all()) and bool((o.dqkv.view[:, :2 * c.HD][:, dead] == 0).all()), 'columns past dim_head must stay zero'
    # one NULL gain and one set stays an error
    bad = capi.make_args('tfx_qk_norm_rope_args', T=T, H=H, qkv=c.qkv, ld_qkv=c.ld, qk=o.qk.view, ld_qk=c.ld_qk, gamma_q=c.gq, gamma_k=None, rot_pos=c.pos,
                         cos_tab=c.cos, sin_tab=c.sin, q_scale=c.q_scale)
    assert capi.lib().tfx_qk_norm_rope_fwd(ctypes.byref(bad), st) != 0


@pytest.mark.parametrize('T,H,d,kind,cache', [(70, 8, 1024, 5, True), (1100, 8, 1024, None, True), (66000, 8, 512, 3, False)],
                         ids=['M70-decode_step_kernel', 'M1100-two_launches', 'M66000-ping_pong_kernel'])
def test_fused_projection_epilogue_without_the_norm_is_bit_identical(T, H, d, kind, cache):
    """TFX_EPI_QKV_NORM_ROPE with NULL gains - on the decode-step kernel (cache append fused), off it (the library's own two launches) and on the
    256 x 256 ping-pong kernel - against the plain projection followed by tfx_qk_norm_rope_fwd with NULL gains: raw projection, q~ | k~, plan and
    cache identical bit for bit"""
    capi, st = _capi()
    torch.manual_seed(41)
    HD = H * 64
    N = 3 * HD + H; ldq = (N + 63) // 64 * 64
    u, W = torch.randn(T, d, device=DEV).to(BF), (torch.randn(N, d, device=DEV) * d ** -0.5).to(BF)
    pos = torch.randint(0, 1000, (T,), device=DEV, dtype=torch.int32)
    freqs = 1. / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(1024).float()[:, None] * freqs[None]
    cos_t, sin_t = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    rows_cache = 4 * T
    cpos = torch.randperm(rows_cache, device=DEV)[:T].to(torch.int32)
    cpos[torch.rand(T, device=DEV) < 0.2] = -1
    k_, g_ = ctypes.c_int32(-1), ctypes.c_int32(-1)
    pa = capi.make_args('tfx_gemm_nt_args', A=u, lda=d, B=W, ldb=d, M=T, N=N, K=d, epi=capi.ENUMS['TFX_EPI_QKV_NORM_ROPE'],
                        C=torch.empty(T, ldq, device=DEV, dtype=BF), ldc=ldq)
    capi.lib().tfx_gemm_nt_plan(ctypes.byref(pa), ctypes.byref(k_), ctypes.byref(g_))
    assert (k_.value == kind) if kind is not None else (k_.value not in (3, 5)), k_.value      # (only kinds 3 and 5 carry the fused epilogue)
    outs = []
    for fused in (False, True):
        C = torch.full((T, ldq), float('nan'), device=DEV, dtype=BF); qk = torch.full((T, 2 * HD), float('nan'), device=DEV, dtype=BF)
        kv = torch.full((rows_cache if cache else 1, 2 * HD), 7.0, device=DEV, dtype=BF); plan = torch.full((8,), float('nan'), device=DEV)
        if fused:
            ck = dict(qk_cache=kv, qk_ld_cache=2 * HD, qk_cache_pos=cpos) if cache else {}
            a = capi.make_args('tfx_gemm_nt_args', A=u, lda=d, B=W, ldb=d, M=T, N=N, K=d, epi=capi.ENUMS['TFX_EPI_QKV_NORM_ROPE'], C=C, ldc=ldq, C2=qk, ldc2=2 * HD,
                               qk_heads=H, qk_gamma_q=None, qk_gamma_k=None, qk_rot_pos=pos, qk_cos=cos_t, qk_sin=sin_t, qk_q_scale=0.125, qk_norm_scale=8.0,
                               qk_plan=plan, qk_softcap=50.0, **ck)
            capi.call('tfx_gemm_nt', a, st)
        else:
            capi.call('tfx_gemm_nt', capi.make_args('tfx_gemm_nt_args', A=u, lda=d, B=W, ldb=d, M=T, N=N, K=d, epi=capi.ENUMS['TFX_EPI_BF16'], C=C, ldc=ldq), st)
            ck = dict(cache=kv, ld_cache=2 * HD, cache_pos=cpos) if cache else {}
            capi.call('tfx_qk_norm_rope_fwd', capi.make_args('tfx_qk_norm_rope_args', T=T, H=H, qkv=C, ld_qkv=ldq, qk=qk, ld_qk=2 * HD, gamma_q=None, gamma_k=None,
                                                             rot_pos=pos, cos_tab=cos_t, sin_tab=sin_t, q_scale=0.125, norm_scale=8.0, sc_plan=plan, softcap=50.0, **ck), st)
        torch.cuda.synchronize()
        outs.append((C[:, :N].clone(), qk, kv, plan))
    (C0, qk0, ca0, pl0), (C1, qk1, ca1, pl1) = outs
    assert torch.isfinite(qk1.float()).all() and torch.isfinite(C1.float()).all()
    assert torch.equal(C1, C0), 'raw projection'
    assert torch.equal(qk1, qk0), f'q~ | k~ differ in {(qk1 != qk0).sum().item()} elements'
    assert torch.equal(ca1, ca0), f'cache differs in {(ca1 != ca0).sum().item()} elements'
    assert torch.equal(pl1, pl0) and int(pl1[0].item()) == 2 and pl1[7].item() == float('inf')
    # q~ really is the rotated, scaled, UN-normalised projection: its rows keep the raw rows' norms (a rotation; q scaled by 1 / 8)
    nq, nr_ = qk1[:, :HD].float().reshape(T, H, 64).norm(dim=-1), C1[:, :HD].float().reshape(T, H, 64).norm(dim=-1) * 0.125
    assert float(((nq - nr_).abs() / nr_.clamp_min(1e-6)).max()) < 2e-2
    if cache:
        live = cpos[cpos >= 0].long()
        assert (ca1[live] != 7.0).any() and torch.equal(ca1[live][:, HD:], C1[(cpos >= 0)][:, 2 * HD:3 * HD]) and torch.equal(ca1[live][:, :HD], qk1[(cpos >= 0)][:, HD:])


@pytest.mark.parametrize('laser', [False, True])
@pytest.mark.parametrize('name', list(ATTN_CASES))
def test_attention_backward_epilogue_without_the_norm_equals_the_separate_launch(name, laser):
    """tfx_attn_bwd with the nr_* fields and NULL gains (d q | d k leave through the dQ and dK/dV epilogues; nr_dgamma_* NULL) against the same call
    without them followed by tfx_qk_norm_rope_bwd with NULL gains: every output bit for bit, with the mode-2 plan the no-norm forward wrote passed along,
    gate = NULL as the both-off model runs it; and per row against float64"""
    case = ATTN_CASES[name]
    inp, qk, got, fused = run_attention(case, None, laser, 'null', nonorm=True, nr='fused', plan_given=True)
    _, _, _, sep = run_attention(case, None, laser, 'null', nonorm=True, nr='separate', plan_given=True)
    for k in fused:
        assert torch.equal(bits(fused[k]), bits(sep[k])), (name, laser, k)
    # float64: d q~ | d k~ of the exact-input reference through the no-norm backward (identity rotation here: d q = d q~ / 8, d k = d k~)
    ref = nogate_reference(inp, case, qk.float().cpu(), {k: v.cpu() for k, v in got.items()}, laser)
    ref['dq'] = ref['dq'] * inp['q_scale']
    m = metrics({k: v.cpu() for k, v in got.items()}, ref)
    tol = row_tol(laser)
    worst = {k: float(v.max()) for k, v in m.items()}
    print(f'NONORM-NR {name} laser={int(laser)} ' + ' '.join(f'{k}={v:.2e}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= tol[k], (name, laser, k, v, tol[k])


@pytest.mark.parametrize('laser', [False, True])
@pytest.mark.parametrize('name', list(ATTN_CASES))
def test_scores_outside_the_polynomial_range(name, laser):
    """unnormalised q / k through the no-norm forward, scores up to about 3 x the soft-cap, no plan: the data-dependent form with exact tanh above the
    polynomial's range, forward and backward, every row of every head under the bounds of _attn_cases - the case QK-RMSNorm used to exclude"""
    case = ATTN_CASES[name]
    inp, qk, got, _ = run_attention(case, None, laser, 'own', nonorm=True, inp=loud_inputs(case))
    HD = case.h * 64
    s = torch.einsum('thd,uhd->htu', qk[:, :HD].float().reshape(-1, case.h, 64), qk[:, HD:].float().reshape(-1, case.h, 64))
    print(f'LOUD {name}: max |s| {float(s.abs().max()):.1f}, share of |s| > 17.5 (0.35 cap) {float((s.abs() > 17.5).float().mean()):.2f}')
    assert float(s.abs().max()) > 100.
    cpu = {k: v.cpu() for k, v in got.items()}
    m = metrics(cpu, exact_input_reference(inp, case, qk.float().cpu(), cpu, laser=laser))
    tol = row_tol(laser)
    worst = {k: float(v.max()) for k, v in m.items()}
    print(f'LOUD {name} laser={int(laser)} ' + ' '.join(f'{k}={v:.2e}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= tol[k], (name, laser, k, v, tol[k])


# ---------------------------------------------------------------------------------------------- kernels: training forward and backward
@pytest.mark.parametrize('laser', [False, True])
@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('name', list(ATTN_CASES))
def test_attention_without_a_gate(name, mode, laser):
    """gate = NULL, forward and backward (prep, dK/dV, the generated dQ loop under plan modes 0 / 1): every row of every head under the bounds of
    _attn_cases against fp64 with sigmoid = 1; a dgate buffer handed in keeps its poison (run_attention); and the bits of a gated call whose
    sigmoid is exactly 1"""
    case = ATTN_CASES[name]
    inp, qk, got, raw = run_attention(case, mode, laser, 'null')
    ref = nogate_reference(inp, case, qk.float().cpu(), {k: v.cpu() for k, v in got.items()}, laser)
    m = metrics({k: v.cpu() for k, v in got.items()}, ref)
    tol = row_tol(laser)
    worst = {k: float(v.max()) for k, v in m.items()}
    print(f'NOGATE {name} mode={mode} laser={int(laser)} ' + ' '.join(f'{k}={v:.2e}' for k, v in worst.items()))
    assert set(worst) == {'out', 'lse', 'dq', 'dk', 'dv', 'do_eff', 'delta'}
    for k, v in worst.items():
        assert v <= tol[k], (name, mode, laser, k, v, tol[k])
    _, _, _, big = run_attention(case, mode, laser, 'big')
    for k in raw:
        assert torch.equal(bits(raw[k]), bits(big[k])), (name, mode, laser, k)


# ---------------------------------------------------------------------------------------------- kernels: decode against a KV cache
def _check_decode(entry, P, mode, laser, case=None):
    """test_decode_attn_edges_gpu.check_case for a gate == NULL launch"""
    case = case or P['case']
    h, HD = case.h, case.h * 64
    out, lse = run_decode(entry, P, laser, 'null', b=case.b, lq=case.lq, units=case.units)
    ones = torch.full_like(P['gate'].float(), float('inf'))                                   # sigmoid = 1
    ref = decode_reference(case, P['q'][:, :HD], P['cache'][:, :HD], P['side'] if laser else P['cache'][:, HD:], ones, P['kv_end'], laser=laser, vprime=True)
    owned = torch.zeros(case.R, dtype=torch.bool, device=DEV)
    worst, worst_lse = 0., 0.
    for s, r0, c in case.spans():
        assert bool(torch.isnan(lse[s, :, c:]).all()), f'{case.name}: lse slots past unit {s} were written'
        if c == 0:
            continue
        owned[r0:r0 + c] = True
        got = heads(out[r0:r0 + c].float(), 1, c, h)
        assert torch.isfinite(got).all() and torch.isfinite(lse[s, :, :c]).all(), f'{case.name}: unit {s} has unwritten or non-finite elements'
        worst = max(worst, float(row_err(got, ref[s][0]).max()))
        worst_lse = max(worst_lse, float((lse[s, :, :c].double() - ref[s][1][0]).abs().max()))
    assert bool((bits(out[:, HD:]) == POISON).all()) and bool((bits(out[~owned]) == POISON).all()), f'{case.name}: padding or unowned rows were written'
    tol = row_tol(laser)
    print(f'NOGATE-DEC {entry} {case.name} mode={mode} laser={int(laser)} out={worst:.2e} lse={worst_lse:.2e}')
    assert worst <= tol['out'] and worst_lse <= tol['lse'], (case.name, mode, laser, worst, worst_lse)
    big, lse_big = run_decode(entry, P, laser, 'big', b=case.b, lq=case.lq, units=case.units)
    assert torch.equal(bits(out), bits(big)) and torch.equal(bits(lse[~torch.isnan(lse)]), bits(lse_big[~torch.isnan(lse_big)])), case.name


# (LASER runs take the catalogue's LASER subset: its five-row case there is t5_dh32)
@pytest.mark.parametrize('name,mode,laser', [('trip', None, False), ('pairs', 0, False), ('t5', None, False), ('t5', 1, False),
                                             ('trip', 0, True), ('pairs', None, True), ('t5_dh32', None, True), ('t5_dh32', 1, True)])
def test_decode_without_a_gate(name, mode, laser):
    """tfx_decode_attn with 1 and 2 new rows per sample (the rows kernel) and 5 (the tiled kernel against the cache), held to the sentinel-length
    catalogue of _decode_attn_cases"""
    assert DECODE_CASES[name].sub or not laser
    _check_decode('tfx_decode_attn', dec.prepared(name, mode), mode, laser)


@pytest.mark.parametrize('entry', ['tfx_attn_fwd', 'tfx_decode_attn'])
@pytest.mark.parametrize('laser', [False, True])
def test_compacted_decode_without_a_gate(entry, laser):
    P = dec.prepared('compact', 0)
    if entry == 'tfx_attn_fwd':
        _check_decode(entry, P, 0, laser)
    else:                                                            # units of one, zero and two rows in a launch with n = 2: still the tiled kernel
        row0, cnt, R = COMPACT.units
        _check_decode(entry, P, 0, laser, case=COMPACT._replace(name='compact_n2', lq=2, kv_end=COMPACT.kv_end[:3], units=(row0[:3], cnt[:3], R)))


@pytest.mark.parametrize('laser', [False, True])
def test_decode_row_bits_do_not_depend_on_the_launch_shape_without_a_gate(laser):
    """a row of the 'pairs' case alone (n = 1) and as either row of an n = 2 launch on the rows kernel; a row of 't49' in its 49-row launch, alone
    and inside a three-row compacted unit on the tiled kernel"""
    P = dec.prepared('pairs', None)
    b, HD = PAIRS.b, PAIRS.h * 64
    q, ke = P['q'].view(b, 2, -1), P['kv_end'].view(b, 2)
    out2, lse2 = run_decode('tfx_decode_attn', P, laser, 'null')
    for j in (0, 1):
        out1, lse1 = run_decode('tfx_decode_attn', P, laser, 'null', q=q[:, j].contiguous(), kv_end=ke[:, j].contiguous(), lq=1)
        assert torch.equal(bits(out2.view(b, 2, -1)[:, j, :HD]), bits(out1[:, :HD])) and torch.equal(bits(lse2[:, :, j]), bits(lse1[:, :, 0])), j
    P = dec.prepared('t49', 0)
    case = P['case']
    b, lq, HD = case.b, case.lq, case.h * 64
    out49, lse49 = run_decode('tfx_attn_fwd', P, laser, 'null')
    rows = (10, 0, 31)
    sel = torch.tensor([s * lq + r for s, r in enumerate(rows)], device=DEV)
    out1, lse1 = run_decode('tfx_attn_fwd', P, laser, 'null', q=P['q'][sel], kv_end=P['kv_end'][sel].contiguous(), lq=1)
    assert torch.equal(bits(out1[:, :HD]), bits(out49[sel, :HD])), 'alone'
    assert torch.equal(bits(lse1[:, :, 0]), bits(torch.stack([lse49[s, :, r] for s, r in enumerate(rows)]))), 'alone, lse'
    units, R = (1, 7, 11), 16
    sel3 = torch.zeros(R, dtype=torch.long, device=DEV)
    for s, (r, r0) in enumerate(zip(rows, units)):
        sel3[r0:r0 + 3] = torch.tensor([s * lq + (r + o) % lq for o in (-1, 0, 1)], device=DEV)
    out3, _ = run_decode('tfx_attn_fwd', P, laser, 'null', q=P['q'][sel3], kv_end=P['kv_end'][sel3].contiguous(), lq=3, units=(units, (3,) * b))
    assert torch.equal(bits(out3[[r0 + 1 for r0 in units], :HD]), bits(out49[sel, :HD])), 'compacted'


# ---------------------------------------------------------------------------------------------- the model against the reference's fixtures
def _golden(name):
    return torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)


def _build(cfg, sd, sw, **kw):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, transformer=transformer_kwargs(cfg, **sw), prob_uncond=0., **kw)
    m.load_state_dict(strip_state(sd, sw), strict=True)
    return m.cuda()


def _unread_gammas_have_zero_gradient(model, sw):
    """without QK-RMSNorm the q_norm / k_norm gammas are parameters nothing reads (the reference leaves their .grad None): exactly zero here"""
    for k, p in model.named_parameters():
        if k.endswith(('q_norm.gamma', 'k_norm.gamma')) and not sw.get('qk_rmsnorm', True):
            assert p.grad is not None and bool((p.grad == 0).all()), k


def _grads_match(model, g):
    """per parameter, the norm and the first 1024 elements (all the fixture keeps of a gradient) at GRAD_TOL; norm-weighted mean at GRAD_MEAN_TOL"""
    worst, wname, wsum, nsum = 0., '', 0., 0.
    for k, p in model.named_parameters():
        assert k in g['grad_norms'] or k in g['grad_none'] or not p.requires_grad, k
        if k not in g['grad_norms'] or g['grad_norms'][k] < 1e-7:
            continue
        assert p.grad is not None, k
        r = rel(p.grad.float().reshape(-1)[:1024], g['grad_head'][k])
        gn = float(p.grad.double().norm())
        assert abs(gn - g['grad_norms'][k]) <= GRAD_TOL * g['grad_norms'][k], (k, gn, g['grad_norms'][k])
        if r > worst:
            worst, wname = r, k
        wsum += r * g['grad_norms'][k]; nsum += g['grad_norms'][k]
    print(f'  gradients: worst head rel {worst:.3e} ({wname}, norm {g["grad_norms"].get(wname, 0.):.2e}), norm-weighted mean {wsum / nsum:.3e}')
    assert worst <= GRAD_TOL and wsum / nsum <= GRAD_MEAN_TOL, (wname, worst, wsum / nsum)


@pytest.mark.parametrize('name', [*TRAIN_FIXTURES, *LASER_FIXTURES])
def test_training_step_matches_reference_golden(name):
    """loss and breakdown 1e-3 x max(1, |ref|), logits 1e-2 rel-Frobenius, gradients per parameter 4e-2 (norm and the first 1024 elements, the LASER
    fixture's like the others') and 1.2e-2 norm-weighted"""
    from oracle.cases import build_case
    g = _golden(name)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    model = _build(cfg, sd, FIXTURES[name]).train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss, bd = model(batch, times=times, return_breakdown=True)
    loss.backward()
    torch.cuda.synchronize()
    plan = model._live[0]
    logits = plan.logits.view(plan.b, plan.n, -1)[:, :model._live_n_true, :cfg.vocab].float().cpu()
    loss = loss.detach()
    print(f'  loss native {float(loss):.6f} reference {float(g["loss"]):.6f} (plain {float(g["plain_loss"]):.6f}); '
          f'logits rel {rel(logits, g["logits"]):.3e} (reference bf16 autocast {g["bf16_logits_rel"]:.3e})')
    assert abs(float(loss) - float(g['loss'])) <= LOSS_TOL * max(1., abs(float(g['loss'])))
    assert abs(float(bd.text) - float(g['text_loss'])) <= LOSS_TOL * max(1., abs(float(g['text_loss'])))
    for got, want in zip(bd.flow, g['flow_losses']):
        assert abs(float(got) - float(want)) <= LOSS_TOL * max(1., abs(float(want)))
    assert rel(logits, g['logits']) <= LOGIT_TOL
    _grads_match(model, g)
    _unread_gammas_have_zero_gradient(model, FIXTURES[name])


def test_engine_separate_no_norm_backward_equals_the_fused_epilogue(monkeypatch):
    """the engine's own switch, as tests/test_model_gpu.py test_fused_qk_norm_rope_backward_equals_the_separate_launch throws it: a both-off `small2`
    step with TFX_ATTN_QKNR=0 (attention backward writes d q~ | d k~, one tfx_qk_norm_rope_bwd per layer with NULL gains and NULL gain gradients) and
    with the default (the nr_* epilogues with NULL gains).  The two kernel routes agree bit for bit (above), so what is left between the two steps is
    the order in which fp32 atomics of the weight-gradient products arrive under another launch timing: loss 1e-6 as there, and every gradient at the
    2e-3 that test_side_stream_weight_gradients_equal_single_stream allows identical launches (not that test's 1e-2, which pays for bf16 flips the
    no-norm routes do not have).  The unread gammas' gradient is exactly zero either way."""
    from oracle.cases import build_case
    cfg, sd, batch, times, noise = build_case('small2')
    outs = []
    for mode in ('0', '1'):
        monkeypatch.setenv('TFX_ATTN_QKNR', mode)
        model = _build(cfg, sd, BOTH).train()
        model._noise_override = {t: v.cuda() for t, v in noise.items()}
        loss = model(batch, times=times)
        loss.backward()
        torch.cuda.synchronize()
        n_sep = sum(1 for it in model._live[0].bwd if it[0] == 'tfx_qk_norm_rope_bwd')
        assert n_sep == (cfg.depth if mode == '0' else 0), 'the switch must change the backward list'
        _unread_gammas_have_zero_gradient(model, BOTH)
        outs.append((float(loss.detach()), {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = outs
    assert abs(l1 - l0) <= 1e-6 * max(1., abs(l0))
    assert set(g0) == set(g1)
    live = [k for k in g0 if float(g0[k].norm()) > 0]
    errs = {k: rel(g1[k], g0[k]) for k in live}
    norms = {k: float(g0[k].double().norm()) for k in live}
    mean = sum(errs[k] * norms[k] for k in live) / sum(norms.values())
    print(f'  separate vs fused no-norm backward: worst gradient rel difference {max(errs.values()):.2e}, norm-weighted mean {mean:.2e}')
    for k in live:
        assert errs[k] <= 2e-3, (k, errs[k])


def test_forward_text_generation_and_kv_cache_match_reference_golden():
    from oracle.cases import build_text_case
    g = _golden(TEXT_FIXTURE)
    cfg, sd, text = build_text_case(g['base_case'])
    model = _build(cfg, sd, FIXTURES[TEXT_FIXTURE]).train()
    loss = model.forward_text(text)
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    print(f'  loss native {float(loss):.6f} reference {float(g["loss"]):.6f}')
    assert abs(float(loss) - float(g['loss'])) <= LOSS_TOL * max(1., abs(float(g['loss'])))
    _unread_gammas_have_zero_gradient(model, FIXTURES[TEXT_FIXTURE])
    model.eval()
    with torch.no_grad():
        logits, (kv, seen) = model.forward_text(text[:, :-1].cuda(), return_loss=False, return_kv_cache=True)
    e = rel(logits.float().cpu(), g['logits'])
    assert tuple(kv.shape) == tuple(g['kv_shape']) and int(seen) == g['kv_seen']
    ek = rel(kv[[0, -1], :, 0, :, :32].float().cpu(), g['kv_head'])
    print(f'  logits rel {e:.3e}, kv cache head rel {ek:.3e}')
    assert e <= LOGIT_TOL and ek <= 2e-2
    with torch.no_grad():
        gen = model.generate_text_only(g['gen_prompt'].cuda(), 16 + 24, temperature=0.).cpu()
    firsts = []
    for r in range(gen.shape[0]):
        diff = (gen[r] != g['gen_tokens'][r]).nonzero()
        if len(diff):
            j = int(diff[0])
            assert float(g['gen_margin'][r, j]) <= NEAR_TIE, f'row {r}: token {j} differs at reference margin {float(g["gen_margin"][r, j]):.3f}'
            firsts.append(j)
    print(f'  greedy tokens: {gen.numel()} compared, first divergences (near ties only) {firsts}')


def _sampling_model():
    from oracle.make_golden_sampling import sampling_case
    cfg, sd, prompts, noise = sampling_case(False)
    return _build(cfg, sd, FIXTURES[SAMPLING_FIXTURE], modality_default_shape=(4,)).eval(), prompts, noise


@pytest.mark.parametrize('run,kw', [('free', {}), ('forced', dict(force_modality_at_start=0)), ('forced_nocfg', dict(force_modality_at_start=0, cfg_scale=1.))])
def test_sample_many_matches_reference_golden(run, kw):
    """tests/test_laser_gpu.py's walk: every reference decision with a top-2 margin of NEAR_TIE or more identical, decoded modalities within 5e-2"""
    from test_laser_gpu import _plain, _walk
    g = _golden(SAMPLING_FIXTURE)
    m, prompts, noise = _sampling_model()
    kwargs = dict(max_length=12, text_temperature=0., init_modality_noise=noise, modality_steps=4, fixed_modality_shape=(4,), cfg_scale=3.)
    kwargs.update(kw)
    outs = m.sample_many([p if not isinstance(p, list) else list(p) for p in prompts], **kwargs)
    tot, tot_all, n_mod = 0, 0, 0
    for i, (o, r, mg) in enumerate(zip(outs, g['runs'][run], g['margins'][run])):
        margins = {(pi, pos): v for pi, pos, v in mg}
        n_dec, errs = _walk(_plain(o), r, margins)
        tot += n_dec; tot_all += sum(v >= NEAR_TIE for v in margins.values()); n_mod += len(errs)
        print(f'  [{run}] sample {i}: {n_dec} decisive steps identical; modality rel errs {["%.2e" % e for e in errs]}')
        for e in errs:
            assert e <= 5e-2
    if run != 'free':
        assert n_mod >= 4
    assert tot >= 0.5 * tot_all, f'only {tot} of {tot_all} decisive steps compared'


def test_sample_one_equals_sample_many():
    """a prompt decoded next to another one in sample_many (two samples per launch, rows compacted as they finish) and alone in sample_one: the
    same pieces, text tokens and modality latents bit for bit"""
    from test_laser_gpu import _plain
    m, prompts, noise = _sampling_model()
    kwargs = dict(max_length=10, text_temperature=0., init_modality_noise=noise, modality_steps=4, fixed_modality_shape=(4,), cfg_scale=3.,
                  force_modality_at_start=0)
    many = m.sample_many([prompts[0], prompts[1]], **kwargs)
    for i in (0, 1):
        one = _plain(m.sample_one(prompts[i], **kwargs))
        got = _plain(many[i])
        assert len(got) == len(one) and len(one) > 0
        for a, b in zip(got, one):
            assert a[0] == b[0]
            if a[-1].is_floating_point():
                print(f'  prompt {i}: sample_one vs sample_many {a[0]}: max |delta| {float((a[-1].float() - b[-1].float()).abs().max()):.3e}')
            assert a[-1].shape == b[-1].shape and torch.equal(a[-1], b[-1]), (i, a[0])


# ---------------------------------------------------------------------------------------------- other paths
def _falling(losses):
    print('  losses ' + ' '.join(f'{x:.4f}' for x in losses))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]


@pytest.mark.parametrize('laser', [False, True])
def test_fused_muon_steps_on_a_both_off_model(laser):
    from oracle.cases import build_case
    from transfusion_pytorch_amd.optim import FusedMuon
    cfg, sd, batch, times, noise = build_case('small2')
    model = _build(cfg, sd, dict(BOTH, attn_laser=laser)).train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    opt = FusedMuon(model, lr=3e-3, max_grad_norm=0.5)
    losses = []
    for _ in range(4):
        loss = model(batch, times=times)
        loss.backward()
        opt.step(); opt.zero_grad()
        losses.append(float(loss.detach()))
    _falling(losses)


def test_self_flow_steps_on_a_both_off_model():
    from oracle.cases import build_case
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    from transfusion_pytorch_amd.optim import FusedAdam
    cfg, sd, batch, times, noise = build_case('small2')
    w = SelfMaskedRepTraining(_build(cfg, sd, BOTH), use_asymmetric_dropout=False, rep_loss_weight=0.1, student_layer=-1, teacher_layer=-1).cuda()
    assert w.teacher.ema_model.md.gates is False and w.teacher.ema_model.md.qk_norm is False, 'the Self-Flow teacher is a copy of the architecture'
    ov = {t: v.cuda() for t, v in noise.items()}
    w.student._noise_override = ov
    w.teacher.ema_model._noise_override = ov
    opt = FusedAdam(w.student, lr=3e-3, max_grad_norm=0.5)
    losses = []
    for _ in range(4):
        total, (student_loss, rep_loss) = w(batch, times=times)
        total.backward()
        opt.step(); opt.zero_grad()
        w.update_teacher()
        losses.append(float(total.detach()))
    _falling(losses)


def test_ema_copy_carries_the_switches():
    from oracle.cases import build_case
    cfg, sd, batch, times, noise = build_case('small2')
    model = _build(cfg, sd, BOTH)
    ema = model.create_ema()
    assert ema.ema_model.md.gates is False and ema.ema_model.md.qk_norm is False and sorted(ema.ema_model.state_dict()) == sorted(model.state_dict())
    ema.update()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in ema.ema_model.parameters())
