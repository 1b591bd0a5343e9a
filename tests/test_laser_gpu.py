"""LASER attention on the MI355X (Transformer(attn_laser=True), reference T:979-983, T:1019-1022).

Kernel level: raw v -> tfx_laser_v_fwd -> tfx_attn_fwd (laser = 1) -> tfx_attn_bwd -> tfx_laser_v_bwd against fp32 autograd of the reference formula
(softclamp 50 scores, prefix mask, v' = exp(15 tanh(v / 15)), L = log(P v'), sigmoid gate), and the decode kernels with a KV cache.
End to end: the reference's laser goldens (tools/make_golden_laser.py) under the tolerances of tests/test_model_gpu.py, and a short training run.
"""
import os

import pytest
import torch

from transfusion_pytorch_amd import capi

pytestmark = pytest.mark.gpu
DEV, BF = 'cuda', torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C = 15.
LOSS_TOL, LOGIT_TOL, GRAD_TOL, GRAD_MEAN_TOL, GRAD_HEAD_TOL = 1e-3, 1e-2, 4e-2, 1.2e-2, 8e-2
NEAR_TIE = 0.05


def stream():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def check(name, got, ref, tol):
    assert torch.isfinite(got.float()).all(), f'{name}: non-finite output'
    e = rel(got, ref)
    print(f'  {name}: rel err {e:.3e} (tol {tol})')
    assert e <= tol, f'{name}: rel err {e} > {tol}'


def make_kv_end(b, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    kv_end = torch.arange(1, n + 1).repeat(b, 1)
    q_start = torch.arange(n).repeat(b, 1)
    for bi in range(b):
        pos = 3
        while pos < n - 2:
            L = min(int(torch.randint(1, 9, (1,), generator=g)), n - pos)
            kv_end[bi, pos:pos + L] = pos + L
            q_start[bi, pos:pos + L] = pos
            pos += L + int(torch.randint(1, 30, (1,), generator=g))
    return kv_end.to(torch.int32), q_start.to(torch.int32)


def laser_ref(q, k, v, gate, kv_end, cap=50.):
    """q, k, v (b, h, n, 64) fp32, raw v; gate (b, h, n); kv_end (b, n): reference T:979-983, T:998-1027"""
    n = q.shape[2]
    vl = torch.exp(C * torch.tanh(v / C))
    sim = torch.tanh(torch.einsum('bhid,bhjd->bhij', q, k) / cap) * cap
    mask = torch.arange(n, device=q.device)[None, None, :] < kv_end[:, :, None]
    sim = sim.masked_fill(~mask[:, None], -torch.finfo(torch.float32).max)
    o = torch.einsum('bhij,bhjd->bhid', sim.softmax(-1), vl)
    return torch.log(o.clamp_min(1e-20)) * gate.sigmoid()[..., None]


def laser_v(v, ld_v, vl, ld_vl, T, H, rowmap=None):
    a = capi.make_args('tfx_laser_v_args', T=T, H=H, v=v, ld_v=ld_v, vl=vl, ld_vl=ld_vl, rowmap=rowmap, c=C)
    capi.call('tfx_laser_v_fwd', a, stream())


def _qk(T, h, mode):
    """q~ | k~ [T, 2 h 64]: random (mode None: no soft-cap plan) or through tfx_qk_norm_rope_fwd with gains that make it write a plan of mode 0 / 1"""
    HD = h * 64
    if mode is None:
        qk = torch.randn(T, 2 * HD, device=DEV).to(BF)
        qk[:, :HD] *= 0.35
        qk[:, HD:] *= 2.5
        return qk, None
    gscale = {0: 0.04, 1: 0.22}[mode]                                  # the gains of tests/test_kernels_gpu.py's plan test for these modes
    raw = torch.randn(T, 2 * HD, device=DEV).to(BF)
    gq = (torch.rand(64, device=DEV) * 2 - 1) * gscale; gk = (torch.rand(64, device=DEV) * 2 - 1) * gscale
    pos = torch.randint(0, 50, (T,), device=DEV, dtype=torch.int32)
    ang = torch.arange(50, device=DEV)[:, None] * (10000. ** (-torch.arange(32, device=DEV) / 32.))[None, :]
    qk = torch.zeros(T, 2 * HD, device=DEV, dtype=BF)
    plan = torch.full((8,), float('nan'), device=DEV)
    a = capi.make_args('tfx_qk_norm_rope_args', T=T, H=h, qkv=raw, ld_qkv=2 * HD, qk=qk, ld_qk=2 * HD, gamma_q=gq, gamma_k=gk, rot_pos=pos,
                       cos_tab=ang.cos().contiguous(), sin_tab=ang.sin().contiguous(), q_scale=0.125, sc_plan=plan, softcap=50.0)
    capi.call('tfx_qk_norm_rope_fwd', a, stream())
    torch.cuda.synchronize()
    assert int(plan[0].item()) == mode
    return qk, plan


def _run_attn(qk, plan, vl, ld_v, qkv, kv_end, q_start, dout, b, h, n, **extra):
    T, HD = b * n, h * 64
    ldq, ldv = 2 * HD, qkv.shape[1]
    out = torch.zeros(T, HD, device=DEV, dtype=BF); lse = torch.zeros(b, h, n, device=DEV)
    do_eff = torch.zeros(T, HD, device=DEV, dtype=BF); delta = torch.zeros(b, h, n, device=DEV)
    dqk = torch.zeros(T, ldq, device=DEV, dtype=BF); dqkv = torch.zeros(T, ldv, device=DEV, dtype=BF)
    a = capi.make_args('tfx_attn_args', q=qk, k=qk[:, HD:], v=vl, ld_q=ldq, ld_k=ldq, ld_v=ld_v, gate=qkv[:, 3 * HD:], ld_gate=ldv,
                       kv_end=kv_end, q_start=q_start, out=out, ld_out=HD, lse=lse, b=b, h=h, n=n, softcap=50.0,
                       dout=dout, ld_dout=HD, do_eff=do_eff, ld_do=HD, delta=delta, dgate=dqkv[:, 3 * HD:], ld_dgate=ldv,
                       dq=dqk, dk=dqk[:, HD:], dv=dqkv[:, 2 * HD:], ld_dq=ldq, ld_dk=ldq, ld_dv=ldv, sc_plan=plan, **extra)
    capi.call('tfx_attn_fwd', a, stream())
    capi.call('tfx_attn_bwd', a, stream())
    torch.cuda.synchronize()
    return out, lse, dqk, dqkv


@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('vs', [1., 4., 20.])
@pytest.mark.parametrize('b,h,n', [(2, 2, 200), (1, 3, 128), (2, 2, 64), (1, 8, 1024)])
def test_laser_attention_fwd_bwd(b, h, n, vs, mode):
    """mode: the soft-cap plan the training plans pass (tfx_qk_norm_rope_fwd's sc_plan, polynomial modes 0 / 1), or none (scores decide).
    The gradient tolerances are looser than the plain kernel's: the prep recovers L = og / g from the bf16-rounded output, an absolute error of
    up to |L| 2^-9 (~3 % of exp(-L) as |L| nears c = 15 at value scale 20), which do_eff = dout g exp(-L) carries into dq / dk / dv
    (measured worst 2.56e-2, value scale 20 with a plan; tolerance 4e-2)."""
    torch.manual_seed(11)
    T, HD = b * n, h * 64
    ldv = 3 * HD + 8
    qk, plan = _qk(T, h, mode)
    qkv = torch.randn(T, ldv, device=DEV).to(BF)                       # (unused) | v | gates
    qkv[:, 2 * HD:3 * HD] = (qkv[:, 2 * HD:3 * HD].float() * vs).to(BF)
    kv_end, q_start = (x.to(DEV) for x in make_kv_end(b, n))
    vl = torch.zeros(T, HD, device=DEV, dtype=BF)
    laser_v(qkv[:, 2 * HD:], ldv, vl, HD, T, h)
    dout = torch.randn(T, HD, device=DEV).to(BF)
    out, _, dqk, dqkv = _run_attn(qk, plan, vl, HD, qkv, kv_end, q_start, dout, b, h, n, laser=1)
    bw = capi.make_args('tfx_laser_v_args', T=T, H=h, v=qkv[:, 2 * HD:], ld_v=ldv, c=C, dvl=dqkv[:, 2 * HD:], ld_dvl=ldv, dv=dqkv[:, 2 * HD:], ld_dv=ldv)
    capi.call('tfx_laser_v_bwd', bw, stream())
    torch.cuda.synchronize()

    def heads(x):
        return x.float().reshape(b, n, h, 64).transpose(1, 2)
    q = heads(qk[:, :HD]).requires_grad_(True)
    k = heads(qk[:, HD:]).requires_grad_(True)
    v = heads(qkv[:, 2 * HD:3 * HD]).requires_grad_(True)
    g = qkv[:, 3 * HD:3 * HD + h].float().reshape(b, n, h).transpose(1, 2).requires_grad_(True)
    ref = laser_ref(q, k, v, g, kv_end.long())
    ref.backward(heads(dout))
    check('v\'', vl.float(), torch.exp(C * torch.tanh(qkv[:, 2 * HD:3 * HD].float() / C)), 4e-3)
    check(f'laser fwd b{b} h{h} n{n} vs{vs} plan {mode}', heads(out), ref, 1e-2)
    check('laser dq', heads(dqk[:, :HD]), q.grad, 4e-2)
    check('laser dk', heads(dqk[:, HD:]), k.grad, 4e-2)
    check('laser dv', heads(dqkv[:, 2 * HD:3 * HD]), v.grad, 4e-2)
    check('laser dgate', dqkv[:, 3 * HD:3 * HD + h].float().reshape(b, n, h).transpose(1, 2), g.grad, 4e-2)


@pytest.mark.parametrize('mode', [None, 0])
def test_laser_off_is_the_plain_attention(mode):
    """laser = 0 and args that never name the field give the same bytes (forward, lse and every gradient); laser = 1 on the same inputs differs"""
    torch.manual_seed(5)
    b, h, n = 2, 2, 200
    T, HD = b * n, h * 64
    ldv = 3 * HD + 8
    qk, plan = _qk(T, h, mode)
    qkv = torch.randn(T, ldv, device=DEV).to(BF)
    kv_end, q_start = (x.to(DEV) for x in make_kv_end(b, n))
    dout = torch.randn(T, HD, device=DEV).to(BF)
    unset = _run_attn(qk, plan, qkv[:, 2 * HD:], ldv, qkv, kv_end, q_start, dout, b, h, n)
    zero = _run_attn(qk, plan, qkv[:, 2 * HD:], ldv, qkv, kv_end, q_start, dout, b, h, n, laser=0)
    for x, y in zip(unset, zero):
        assert torch.equal(x, y)
    on = _run_attn(qk, plan, qkv[:, 2 * HD:], ldv, qkv, kv_end, q_start, dout, b, h, n, laser=1)
    assert not torch.equal(on[0], unset[0]) and torch.equal(on[1], unset[1])        # lse does not depend on the flag


@pytest.mark.parametrize('nq', [1, 2, 5])
def test_laser_decode_against_a_kv_cache(nq):
    """tfx_decode_attn (one / two rows: the matrix-core-free kernel; five: the tiled kernel with cache addressing) with laser = 1 reading a side cache
    of v' that tfx_laser_v_fwd filled through a row map, against the fp32 formula"""
    torch.manual_seed(3)
    b, h, nkv, cached = 3, 2, 128, 70
    HD = h * 64
    cache = (torch.randn(b, nkv, 2 * HD, device=DEV) * 2).to(BF)          # k~ | raw v per row
    cache[:, :, :HD] = (cache[:, :, :HD].float() * 1.2).to(BF)
    side = torch.zeros(b * nkv, HD, device=DEV, dtype=BF)
    # rows of the cache the model did not append itself: all of them once, then this step's rows again through the row map
    laser_v(cache.view(b * nkv, 2 * HD)[:, HD:], 2 * HD, side, HD, b * nkv, h)
    pos = (torch.arange(b, device=DEV)[:, None] * nkv + cached + torch.arange(nq, device=DEV)[None]).reshape(-1).to(torch.int32)
    newv = (torch.randn(b * nq, HD, device=DEV) * 4).to(BF)
    cache.view(b * nkv, 2 * HD)[pos.long(), HD:] = newv
    laser_v(newv, HD, side, HD, b * nq, h, rowmap=pos)
    q = (torch.randn(b * nq, HD, device=DEV) * 0.35).to(BF)
    gate = torch.randn(b * nq, 8, device=DEV).to(BF)
    kv_end = torch.full((b * nq,), cached + nq, device=DEV, dtype=torch.int32)
    kv_end[::2] = cached + 1
    out = torch.zeros(b * nq, HD, device=DEV, dtype=BF)
    lse = torch.zeros(b, h, nq, device=DEV)
    a = capi.make_args('tfx_attn_args', q=q, k=cache, v=side, ld_q=HD, ld_k=2 * HD, ld_v=HD, gate=gate, ld_gate=8, kv_end=kv_end, q_start=kv_end,
                       out=out, ld_out=HD, lse=lse, b=b, h=h, n=nq, softcap=50.0, n_kv=nkv, laser=1)
    capi.call('tfx_decode_attn', a, stream())
    torch.cuda.synchronize()
    qf = q.float().reshape(b, nq, h, 64).transpose(1, 2)
    kf = cache[:, :, :HD].float().reshape(b, nkv, h, 64).transpose(1, 2)
    vf = cache[:, :, HD:].float().reshape(b, nkv, h, 64).transpose(1, 2)
    s = torch.tanh(torch.einsum('bhid,bhjd->bhij', qf, kf) / 50.) * 50.
    mask = torch.arange(nkv, device=DEV)[None, None, :] < kv_end.reshape(b, nq)[:, :, None].long()
    s = s.masked_fill(~mask[:, None], -torch.finfo(torch.float32).max)
    o = torch.einsum('bhij,bhjd->bhid', s.softmax(-1), torch.exp(C * torch.tanh(vf / C)))
    ref = torch.log(o) * gate[:, :h].float().reshape(b, nq, h).transpose(1, 2).sigmoid()[..., None]
    check(f'laser decode rows {nq}', out.float().reshape(b, nq, h, 64).transpose(1, 2), ref, 1e-2)


def test_laser_tiled_decode_with_compacted_rows():
    """the tiled kernel in the compacted layout of sample_many's plans (tfx_attn_args.q_row0 / q_cnt: sample s owns query rows q_row0[s] ..
    + q_cnt[s] - 1 of a flat row list, keys / values are its n_kv cache rows; q_cnt = 0 sits the step out), laser = 1 against the fp32 formula"""
    torch.manual_seed(4)
    b, h, nkv, nmax = 4, 2, 96, 6
    HD = h * 64
    cnt = [6, 2, 0, 3]
    row0 = [0, 6, 8, 8]
    R = 16                                                               # flat rows (11 used, the rest padding)
    cache = (torch.randn(b, nkv, 2 * HD, device=DEV) * 2).to(BF)
    cache[:, :, :HD] = (cache[:, :, :HD].float() * 1.2).to(BF)
    side = torch.zeros(b * nkv, HD, device=DEV, dtype=BF)
    laser_v(cache.view(b * nkv, 2 * HD)[:, HD:], 2 * HD, side, HD, b * nkv, h)
    q = (torch.randn(R, HD, device=DEV) * 0.35).to(BF)
    gate = torch.randn(R, 8, device=DEV).to(BF)
    kv_end = torch.zeros(R, dtype=torch.int32)
    for s_, (r0, c) in enumerate(zip(row0, cnt)):
        for j in range(c):
            kv_end[r0 + j] = 40 + 9 * s_ + j
    kv_end = kv_end.to(DEV)
    out = torch.zeros(R, HD, device=DEV, dtype=BF)
    lse = torch.zeros(b, h, nmax, device=DEV)
    a = capi.make_args('tfx_attn_args', q=q, k=cache, v=side, ld_q=HD, ld_k=2 * HD, ld_v=HD, gate=gate, ld_gate=8, kv_end=kv_end, q_start=kv_end,
                       out=out, ld_out=HD, lse=lse, b=b, h=h, n=nmax, softcap=50.0, n_kv=nkv, laser=1,
                       q_row0=torch.tensor(row0, dtype=torch.int32, device=DEV), q_cnt=torch.tensor(cnt, dtype=torch.int32, device=DEV))
    capi.call('tfx_attn_fwd', a, stream())
    torch.cuda.synchronize()
    worst = 0.
    for s_, (r0, c) in enumerate(zip(row0, cnt)):
        if c == 0:
            continue
        qf = q[r0:r0 + c].float().reshape(c, h, 64).transpose(0, 1)
        kf = cache[s_, :, :HD].float().reshape(nkv, h, 64).transpose(0, 1)
        vf = cache[s_, :, HD:].float().reshape(nkv, h, 64).transpose(0, 1)
        sc = torch.tanh(torch.einsum('hid,hjd->hij', qf, kf) / 50.) * 50.
        mask = torch.arange(nkv, device=DEV)[None, :] < kv_end[r0:r0 + c, None].long()
        sc = sc.masked_fill(~mask[None], -torch.finfo(torch.float32).max)
        o = torch.einsum('hij,hjd->hid', sc.softmax(-1), torch.exp(C * torch.tanh(vf / C)))
        ref = torch.log(o) * gate[r0:r0 + c, :h].float().t().sigmoid()[..., None]
        got = out[r0:r0 + c].float().reshape(c, h, 64).transpose(0, 1)
        worst = max(worst, rel(got, ref))
    print(f'  compacted laser decode: worst sample rel err {worst:.3e}')
    assert worst <= 1e-2
    assert out[11:].abs().sum() == 0, 'rows outside every sample\'s range are not written'


def _sampling_model(laser=True):
    from oracle.make_golden_sampling import sampling_case
    from transfusion_pytorch_amd import Transfusion
    cfg, sd, prompts, noise = sampling_case(False)
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=cfg.dim_latents[0], modality_default_shape=(4,),
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, attn_laser=laser))
    m.load_state_dict(sd)
    return m.cuda().eval(), prompts, noise


def _plain(sample):
    return [('mod', int(p[0]), p[1].float().cpu()) if isinstance(p, tuple) else ('text', p.cpu().long()) for p in sample]


def _walk(native, ref, margins):
    """tests/test_sampling_gpu.py's rule: every reference decision with top-2 margin >= NEAR_TIE, and every forced / prompt token, identical; the
    native path may leave the reference's only AT a recorded near-tie.  Returns (decisive steps verified, modality rel errors)."""
    n_dec, errs = 0, []
    for pi, (pn, pr) in enumerate(zip(native, ref)):
        assert pn[0] == pr[0], f'part {pi}: kind {pn[0]} vs reference {pr[0]}'
        if pn[0] == 'mod':
            assert pn[2].shape == pr[2].shape
            errs.append(((pn[2] - pr[2]).norm() / pr[2].norm()).item())
            continue
        a, b = pn[1].tolist(), pr[1].tolist()
        for pos, y in enumerate(b):
            mg = margins.get((pi, pos))
            if pos >= len(a) or a[pos] != y:
                assert mg is not None and mg < NEAR_TIE, f'part {pi} pos {pos}: native != reference on a decisive step (margin {mg})'
                return n_dec, errs
            n_dec += mg is not None and mg >= NEAR_TIE
        assert len(a) == len(b)
    assert len(native) == len(ref)
    return n_dec, errs


@pytest.mark.parametrize('run,kw', [('free', {}), ('forced', dict(force_modality_at_start=0)), ('forced_nocfg', dict(force_modality_at_start=0, cfg_scale=1.))])
def test_laser_sample_many_matches_reference_golden(run, kw):
    """sample_many with attn_laser=True (compacted decode plans, the v' side cache, the midpoint ODE with / without CFG) against the reference
    (tests/golden/laser_sampling.pt, tools/make_golden_laser.py)"""
    g = torch.load(os.path.join(GOLDEN, 'laser_sampling.pt'), weights_only=False)
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


def test_laser_sample_one_equals_sample_many():
    m, prompts, noise = _sampling_model()
    kwargs = dict(max_length=10, text_temperature=0., init_modality_noise=noise, modality_steps=4, fixed_modality_shape=(4,), cfg_scale=3.,
                  force_modality_at_start=0)
    many = m.sample_many([prompts[0], prompts[1]], **kwargs)
    one = m.sample_one(prompts[0], **kwargs)
    for a, b in zip(_plain(many[0]), _plain(one)):
        assert a[0] == b[0]
        if a[0] == 'text':
            assert a[1].tolist() == b[1].tolist()
        else:
            d = float((a[2] - b[2]).abs().max())
            print(f'  sample_one vs sample_many modality: max |delta| {d:.3e}')
            assert d <= 1e-4


def test_laser_generate_modality_only_is_finite_and_differs_from_plain():
    """generate_modality_only (the flow decode without text) honours the flag: same weights and noise, laser on / off give different latents"""
    outs = []
    for laser in (True, False):
        m, _, _ = _sampling_model(laser)
        torch.manual_seed(0)
        outs.append(m.generate_modality_only(batch_size=2, modality_type=0, fixed_modality_shape=(4,), modality_steps=4).float().cpu())
    assert torch.isfinite(outs[0]).all()
    assert outs[0].shape == outs[1].shape and not torch.equal(outs[0], outs[1])


def _build(cfg, sd, laser=True):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, attn_laser=laser), prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _grads_match(model, g):
    worst, wsum, nsum = 0., 0., 0.
    for k, p in model.named_parameters():
        if k not in g['grad_norms'] or g['grad_norms'][k] < 1e-7:
            continue
        assert p.grad is not None, k
        r = rel(p.grad.float().reshape(-1)[:1024], g['grad_head'][k])
        gn = float(p.grad.double().norm())
        assert abs(gn - g['grad_norms'][k]) <= GRAD_TOL * g['grad_norms'][k], (k, gn, g['grad_norms'][k])
        worst = max(worst, r); wsum += r * g['grad_norms'][k]; nsum += g['grad_norms'][k]
    print(f'  gradients: worst head rel {worst:.3e}, norm-weighted mean {wsum / nsum:.3e}')
    assert worst <= GRAD_HEAD_TOL and wsum / nsum <= GRAD_MEAN_TOL


@pytest.mark.parametrize('name', ['laser_small2', 'laser_head8'])
def test_laser_training_step_matches_reference_golden(name):
    from oracle.cases import build_case
    g = torch.load(os.path.join(GOLDEN, f'{name}.pt'))
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    model = _build(cfg, sd).train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss = model(batch, times=times)
    loss.backward()
    torch.cuda.synchronize()
    plan = model._live[0]
    nt = model._live_n_true
    logits = plan.logits.view(plan.b, plan.n, -1)[:, :nt, :cfg.vocab].float().cpu()
    print(f'  loss native {float(loss):.6f} reference {float(g["loss"]):.6f} (plain {float(g["plain_loss"]):.6f}); '
          f'logits rel {rel(logits, g["logits"]):.3e} (reference bf16 autocast {g["bf16_logits_rel"]:.3e})')
    assert abs(float(loss) - float(g['loss'])) <= LOSS_TOL * max(1., abs(float(g['loss'])))
    assert rel(logits, g['logits']) <= LOGIT_TOL
    _grads_match(model, g)


def test_laser_forward_text_generation_and_kv_cache_match_reference_golden():
    from oracle.cases import build_text_case
    g = torch.load(os.path.join(GOLDEN, 'laser_text1.pt'))
    cfg, sd, text = build_text_case(g['base_case'])
    model = _build(cfg, sd).train()
    loss = model.forward_text(text)
    loss.backward()
    torch.cuda.synchronize()
    print(f'  loss native {float(loss):.6f} reference {float(g["loss"]):.6f}')
    assert abs(float(loss) - float(g['loss'])) <= 2e-3 * max(1., abs(float(g['loss'])))
    _grads_match(model, g)
    model.eval()
    with torch.no_grad():
        logits, (kv, seen) = model.forward_text(text[:, :-1].cuda(), return_loss=False, return_kv_cache=True)
    assert rel(logits.float().cpu(), g['logits']) <= LOGIT_TOL
    # the KV cache holds RAW v (stacked before the laser transform, T:977)
    assert tuple(kv.shape) == tuple(g['kv_shape']) and int(seen) == g['kv_seen']
    got = kv[[0, -1], :, 0, :, :32].float().cpu()
    e = rel(got, g['kv_head'])
    print(f'  kv cache head rel {e:.3e}')
    assert e <= 2e-2
    with torch.no_grad():
        gen = model.generate_text_only(g['gen_prompt'].cuda(), 16 + 24, temperature=0.).cpu()
    firsts = []
    for r in range(gen.shape[0]):
        diff = (gen[r] != g['gen_tokens'][r]).nonzero()
        if len(diff):
            j = int(diff[0])
            assert float(g['gen_margin'][r, j]) < NEAR_TIE, f'row {r}: token {j} differs at reference margin {float(g["gen_margin"][r, j]):.3f}'
            firsts.append(j)
    print(f'  greedy tokens: {gen.numel()} compared, first divergences (near ties only) {firsts}')


def test_laser_text_only_training_loss_falls():
    """the reference's train_text_only.py model (dim 384, depth 8, dim_head 64, heads 8, attn_laser) for 40 fused-Adam steps on synthetic bytes"""
    from transfusion_pytorch_amd import Transfusion
    from transfusion_pytorch_amd.optim import FusedAdam
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=256, transformer=dict(dim=384, depth=8, dim_head=64, heads=8, attn_laser=True)).cuda().train()
    opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
    # a learnable synthetic stream: repeated random byte phrases
    g = torch.Generator().manual_seed(0)
    phrases = torch.randint(0, 256, (16, 32), generator=g)
    losses = []
    for step in range(40):
        idx = torch.randint(0, 16, (8, 8), generator=g)
        batch = phrases[idx].reshape(8, -1)[:, :257].cuda()
        loss = model.forward_text(batch)
        loss.backward()
        opt.step(); opt.zero_grad()
        losses.append(float(loss))
    print(f'  loss {losses[0]:.3f} -> {losses[-1]:.3f}')
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sum(losses[-5:]) / 5 < 0.8 * sum(losses[:5]) / 5
