"""Cases of the attention-ablation tests (not collected: no test_ prefix; imports no GPU code at module level).

Two switches of the reference's attention block, each a NULL in the C ABI (include/tfx.h):
  Transformer(attn_kwargs=dict(gate_values=False))   no sigmoid output gate (T:901-904, T:1026-1027)      tfx_attn_args.gate == NULL
  Transformer(qk_rmsnorm=False)                      no QK-RMSNorm (T:948-952)                            gamma_q == gamma_k == NULL
The float64 restatements of the gate-less attention are those of tests/_attn_cases.py and tests/_decode_attn_cases.py with gate logits of +inf,
whose sigmoid is exactly 1: out = P v (LASER: log(P v')), do_eff = dout (LASER: dout exp(-og)), delta as with g = 1; the bounds are theirs too
(_attn_cases.row_tol), per row in every head.  The no-norm q~ = rope(q) q_scale, k~ = rope(k) and its backward are restated here per element
with bounds formed as tests/_tokenwise_cases.py forms them."""
from types import SimpleNamespace

import torch

from _attn_cases import CAP, LASER_C, POISON, Case, build_inputs, exact_input_reference, heads, metrics, row_tol      # noqa: F401
from _tokenwise_cases import BF, E, build_qk, new_out, tol_bf16

# fixtures of tools/make_golden_ablation.py and the switches they were made with
NOQK, NOGATE = dict(qk_rmsnorm=False), dict(attn_kwargs=dict(gate_values=False))
BOTH = dict(NOQK, **NOGATE)
TRAIN_FIXTURES = {'ablate_noqk_small2': NOQK, 'ablate_nogate_small2': NOGATE, 'ablate_both_head8': BOTH}
LASER_FIXTURES = {'ablate_both_laser_small2': dict(BOTH, attn_laser=True)}
TEXT_FIXTURE, SAMPLING_FIXTURE = 'ablate_both_text1', 'ablate_both_sampling'
FIXTURES = {**TRAIN_FIXTURES, **LASER_FIXTURES, TEXT_FIXTURE: BOTH, SAMPLING_FIXTURE: BOTH}

# a bf16 gate logit whose sigmoid is exactly 1 in fp32 (exp(-3e4) = 0): the gated call a gate == NULL call must equal bit for bit
BIG_LOGIT = 3e4

# (b, h, n) = (2, 2, 200), (1, 3, 128), (2, 2, 64): more than one 128-row query tile and an odd tail; an odd head count on one exact tile; less than a tile
ATTN_CASES = {c.name: c for c in (
    Case('g200', 2, 200, (((3, 196),), ((7, 49), (60, 49), (109, 49)))),
    Case('g128', 3, 128, (((0, 128),),)),
    Case('g64', 2, 64, (((5, 49),), ())),
)}


def has_gates(sw):
    return sw.get('attn_kwargs', {}).get('gate_values', True)


def transformer_kwargs(cfg, **switches):
    return dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, **switches)


def strip_state(sd, sw):
    """a case's state_dict in the shape of the switched model: without value gating the reference has no `to_gates` module (T:901-904)"""
    return sd if has_gates(sw) else {k: v for k, v in sd.items() if '.to_gates.' not in k}


# ---------------------------------------------------------------------------------------------- no-norm QK + RoPE, per element
def build_nonorm_qk(T, H, dh=64, device='cpu', seed=0):
    """_tokenwise_cases.build_qk's inputs (raw q | k | v rows with a pad, positions, rotary tables, d q~ | d k~) with the float64 references and
    per-element bounds of the NO-NORM forms.  dh < 64: the kernel layout of a smaller head - columns past dim_head of every head zero, in the raw
    rows and in the incoming gradient.  An element is two products and their sum: E(2, sum of the magnitudes), bf16 outputs u16 |y| + 2 E."""
    c = build_qk(T, H, device, seed)
    if dh < 64:
        live = (torch.arange(c.ld, device=device) % 64 < dh) | (torch.arange(c.ld, device=device) >= 3 * c.HD)
        c.qkv = torch.where(live[None], c.qkv, torch.zeros_like(c.qkv))
        c.dqk = torch.where(live[None, :2 * c.HD], c.dqk, torch.zeros_like(c.dqk))
    c.dh = dh
    V = c.qkv[:, :2 * c.HD].double().reshape(T, 2 * H, 64)
    qs = torch.cat([torch.full((H,), c.q_scale), torch.ones(H)]).double().to(device)[None, :, None]
    cs, sn = c.cos[c.pos.long()].double()[:, None], c.sin[c.pos.long()].double()[:, None]
    a = V * qs
    ae, ao = a[..., 0::2], a[..., 1::2]
    y = torch.stack([ae * cs - ao * sn, ao * cs + ae * sn], -1).reshape(T, 2 * H, 64)
    My = torch.stack([ae.abs() * cs.abs() + ao.abs() * sn.abs(), ao.abs() * cs.abs() + ae.abs() * sn.abs()], -1).reshape(T, 2 * H, 64)
    c.qk_ref, c.qk_tol = y.reshape(T, -1), tol_bf16(y, E(2, My)).reshape(T, -1)
    DY = c.dqk.double().reshape(T, 2 * H, 64)
    da, db = DY[..., 0::2], DY[..., 1::2]
    gg = torch.stack([da * cs + db * sn, db * cs - da * sn], -1).reshape(T, 2 * H, 64) * qs
    gm = torch.stack([da.abs() * cs.abs() + db.abs() * sn.abs(), db.abs() * cs.abs() + da.abs() * sn.abs()], -1).reshape(T, 2 * H, 64) * qs
    c.dqkv_ref, c.dqkv_tol = gg.reshape(T, -1), tol_bf16(gg, E(2, gm)).reshape(T, -1)
    return c


def outs_nonorm_qk(c):
    """guarded outputs (q~ | k~ and d q | d k rows with an 8-column pad that must keep its bits) and the gain-gradient sentinels nothing may touch"""
    T, HD, dev = c.T, c.HD, c.device

    def padded_rows(name, ref, tol):
        o = new_out(name, T, 2 * HD + 8, BF, dev)
        z, one = torch.zeros(T, 8, dtype=torch.float64, device=dev), torch.ones(T, 8, dtype=torch.float64, device=dev)
        o.ref, o.tol = torch.cat([ref, z], 1), torch.cat([tol, one], 1)
        o.mask = torch.zeros(T, 2 * HD + 8, dtype=torch.bool, device=dev); o.mask[:, :2 * HD] = True
        return o
    never = torch.zeros(1, 64, dtype=torch.bool, device=dev)
    sent = lambda name, init: new_out(name, 1, 64, torch.float32, dev, torch.zeros(64, dtype=torch.float64, device=dev),
                                      torch.ones(64, dtype=torch.float64, device=dev), mask=never, init=init)
    return SimpleNamespace(qk=padded_rows('qk', c.qk_ref, c.qk_tol), dqkv=padded_rows('dqkv', c.dqkv_ref, c.dqkv_tol),
                           dgamma_q=sent('dgamma_q', c.init_dgq), dgamma_k=sent('dgamma_k', c.init_dgk))


def loud_inputs(case, seed=0):
    """_attn_cases.build_inputs' layout with random UNNORMALISED q / k rows whose scores q~ . k~ (q~ = q / 8, k~ = k) have a standard deviation
    of 0.75 x the soft-cap and reach about 3 x the soft-cap: far outside [-B, B] of any polynomial plan - what QK-RMSNorm used to exclude"""
    inp = build_inputs(case, None, seed)
    g = torch.Generator().manual_seed(seed * 977 + case.n)
    T, HD = case.b * case.n, case.h * 64
    x = inp['qkvg']
    x[:, :HD] = torch.randn(T, HD, generator=g) * 12.
    x[:, HD:2 * HD] = torch.randn(T, HD, generator=g) * 3.1
    x[:, 2 * HD:3 * HD] = torch.randn(T, HD, generator=g)
    inp['dout'] = torch.randn(T, HD, generator=g)
    inp['q_scale'], inp['norm_scale'] = 0.125, 8.
    return inp


def nogate_reference(inp, case, qk, got, laser):
    """_attn_cases.exact_input_reference with sigmoid(gate) = 1: the per-row fp64 reference of every kernel from its own inputs"""
    HD = case.h * 64
    inp = dict(inp)
    x = inp['qkvg'].clone()
    x[:, 3 * HD:3 * HD + case.h] = float('inf')
    inp['qkvg'] = x
    r = exact_input_reference(inp, case, qk, got, laser=laser)
    r.pop('dgate')
    return r


def run_attention(case, mode, laser, gate, nonorm=False, nr=None, inp=None, plan_given=None, dev='cuda'):
    """tfx_qk_norm_rope_fwd (identity rotation; writes the plan) -> [tfx_laser_v_fwd] -> tfx_attn_fwd -> tfx_attn_bwd on the case's sentinel inputs
    (_attn_cases.build_inputs, or `inp`), in _attn_cases.run_kernels' buffer layout, every output poisoned.
      mode    the plan mode the gains are built for; None = no plan passed to the attention (plan_given overrides: True passes whatever was written)
      gate    'null': gate = NULL, the dgate columns are still handed in and must keep their poison; 'big': a gate buffer of logits BIG_LOGIT;
              'own': the inputs' gate logits
      nonorm  NULL gains: q~ = rope(q) q_scale, k~ = rope(k); the plan written must read mode 2 with B = +inf
      nr      None: the backward writes d q~ | d k~;  'fused': the nr_* epilogues write d q | d k (raw) into the gradient matrix;
              'separate': d q~ | d k~, then tfx_qk_norm_rope_bwd as its own launch into the gradient matrix
    Returns (inputs as the kernels saw them, the kernels' q~ | k~, outputs as (b, h, n, ...) tensors, raw buffers)."""
    from transfusion_pytorch_amd import capi
    st = torch.cuda.current_stream().cuda_stream
    inp = inp or build_inputs(case, mode)
    b, h, n = case.b, case.h, case.n
    T, HD, ld = b * n, h * 64, inp['ld']
    qkvg = inp['qkvg'].to(dev).to(BF)
    if gate == 'big':
        qkvg[:, 3 * HD:3 * HD + h] = BIG_LOGIT
    inp['qkvg'] = qkvg.float().cpu()
    gq, gk = (None, None) if nonorm else (inp['gq'].to(dev), inp['gk'].to(dev))
    kv_end, q_start = inp['kv_end'].reshape(-1).to(dev), inp['q_start'].reshape(-1).to(dev)
    pos = torch.zeros(T, device=dev, dtype=torch.int32)
    cos_t, sin_t = torch.ones(8, 32, device=dev), torch.zeros(8, 32, device=dev)
    qk = torch.zeros(T, 2 * HD, device=dev, dtype=BF)
    plan = torch.full((8,), float('nan'), device=dev)
    rope = dict(T=T, H=h, gamma_q=gq, gamma_k=gk, rot_pos=pos, cos_tab=cos_t, sin_tab=sin_t, q_scale=inp['q_scale'], norm_scale=inp['norm_scale'])
    capi.call('tfx_qk_norm_rope_fwd', capi.make_args('tfx_qk_norm_rope_args', qkv=qkvg, ld_qkv=ld, qk=qk, ld_qk=2 * HD, sc_plan=plan, softcap=CAP, **rope), st)
    torch.cuda.synchronize()
    if nonorm:
        assert int(plan[0].item()) == 2 and plan[7].item() == float('inf') and torch.isfinite(plan[:7]).all(), plan.tolist()
    else:
        assert int(plan[0].item()) == (2 if mode is None else mode), (case.name, mode, plan.tolist())
    if plan_given is None:
        plan_given = mode is not None

    def poisoned(*shape):
        return torch.full(shape, POISON, device=dev, dtype=torch.int16).view(BF)
    ld_out, ld_qk = HD + 24, 2 * HD + 8
    out, do_eff, dqk, dqkv = poisoned(T, ld_out), poisoned(T, HD), poisoned(T, ld_qk), poisoned(T, ld)
    lse, delta = torch.full((b, h, n), float('nan'), device=dev), torch.full((b, h, n), float('nan'), device=dev)
    dout = inp['dout'].to(dev).to(BF)
    inp['dout'] = dout.float().cpu()
    vl = None
    if laser:
        vl = torch.zeros(T, HD, device=dev, dtype=BF)
        capi.call('tfx_laser_v_fwd', capi.make_args('tfx_laser_v_args', T=T, H=h, v=qkvg[:, 2 * HD:], ld_v=ld, vl=vl, ld_vl=HD, c=LASER_C), st)
    kw = dict(q=qk, k=qk[:, HD:], v=vl if laser else qkvg[:, 2 * HD:], ld_q=2 * HD, ld_k=2 * HD, ld_v=HD if laser else ld,
              gate=None if gate == 'null' else qkvg[:, 3 * HD:], ld_gate=ld, kv_end=kv_end, q_start=q_start,
              out=out, ld_out=ld_out, lse=lse, b=b, h=h, n=n, softcap=CAP, dout=dout, ld_dout=HD, do_eff=do_eff, ld_do=HD, delta=delta,
              dgate=dqkv[:, 3 * HD:], ld_dgate=ld, dq=dqk, dk=dqk[:, HD:], dv=dqkv[:, 2 * HD:], ld_dq=ld_qk, ld_dk=ld_qk, ld_dv=ld,
              sc_plan=plan if plan_given else None, laser=int(laser))
    dgq, dgk = torch.full((64,), 3., device=dev), torch.full((64,), 5., device=dev)
    if nr == 'fused':
        kw.update(nr_qkv=qkvg, nr_ld_qkv=ld, nr_dqkv=dqkv, nr_ld_dqkv=ld, nr_gamma_q=gq, nr_gamma_k=gk, nr_rot_pos=pos, nr_cos=cos_t, nr_sin=sin_t,
                  nr_q_scale=inp['q_scale'], nr_norm_scale=inp['norm_scale'], nr_dgamma_q=None if nonorm else dgq, nr_dgamma_k=None if nonorm else dgk)
    a = capi.make_args('tfx_attn_args', **kw)
    capi.call('tfx_attn_fwd', a, st)
    capi.call('tfx_attn_bwd', a, st)
    if nr == 'separate':
        capi.call('tfx_qk_norm_rope_bwd', capi.make_args('tfx_qk_norm_rope_args', qkv=qkvg, ld_qkv=ld, dqk=dqk, ld_dqk=ld_qk, dqkv=dqkv, ld_dqkv=ld,
                                                         dgamma_q=dgq, dgamma_k=dgk, **rope), st)
    if laser:
        capi.call('tfx_laser_v_bwd', capi.make_args('tfx_laser_v_args', T=T, H=h, v=qkvg[:, 2 * HD:], ld_v=ld, c=LASER_C, dvl=dqkv[:, 2 * HD:], ld_dvl=ld,
                                                    dv=dqkv[:, 2 * HD:], ld_dv=ld), st)
    torch.cuda.synchronize()

    def untouched(x):
        return bool((x.view(torch.int16) == POISON).all())
    assert torch.isfinite(out[:, :HD].float()).all() and untouched(out[:, HD:]), 'out: unwritten elements, or the ld padding was written'
    assert torch.isfinite(lse).all() and torch.isfinite(delta).all() and torch.isfinite(do_eff.float()).all(), 'lse / delta / do_eff: unwritten or non-finite'
    assert torch.isfinite(dqkv[:, 2 * HD:3 * HD].float()).all(), 'd v: unwritten or non-finite elements'
    assert untouched(dqkv[:, 3 * HD + h:]), 'the pad of the gradient matrix was written'
    if nr == 'fused':
        assert untouched(dqk), 'the fused form must not write d q~ / d k~'
    else:
        assert torch.isfinite(dqk[:, :2 * HD].float()).all() and untouched(dqk[:, 2 * HD:]), 'd q~ | d k~: unwritten elements, or the ld padding was written'
    if nr is None:
        assert untouched(dqkv[:, :2 * HD]), 'the q / k columns of the gradient matrix were written'
    else:
        assert torch.isfinite(dqkv[:, :2 * HD].float()).all(), 'd q | d k (raw): unwritten or non-finite elements'
        if nonorm:
            assert bool((dgq == 3.).all()) and bool((dgk == 5.).all()), 'no gains: the gain gradients must not be touched'
    if gate == 'null':
        assert untouched(dqkv[:, 3 * HD:]), 'gate == NULL: the dgate columns were written'
    else:
        assert torch.isfinite(dqkv[:, 3 * HD:3 * HD + h].float()).all()

    def hd(x):
        return heads(x.float(), b, n, h)
    src = dqkv if nr else dqk
    got = dict(out=hd(out), lse=lse, dv=hd(dqkv[:, 2 * HD:]), do_eff=hd(do_eff), delta=delta, dq=hd(src[:, :HD]), dk=hd(src[:, HD:2 * HD]))
    if gate == 'own':
        got['dgate'] = dqkv[:, 3 * HD:3 * HD + h].float().reshape(b, n, h).transpose(1, 2)
    if laser:
        got['vl'] = hd(vl)
    raw = dict(out=out[:, :HD], lse=lse, do_eff=do_eff, delta=delta, dqk=src[:, :2 * HD], dv=dqkv[:, 2 * HD:3 * HD])
    return inp, qk, got, raw


def run_decode(entry, P, laser, gate, q=None, kv_end=None, b=None, lq=None, units=None, dev='cuda'):
    """one attention launch against the prepared cache P of tests/test_decode_attn_edges_gpu.py (`prepared`): its query rows (or `q` / `kv_end`, rows
    of them) with gate = NULL ('null') or a buffer of BIG_LOGIT logits ('big').  out starts as POISON with ld > h 64, lse as NaN."""
    from transfusion_pytorch_amd import capi
    st = torch.cuda.current_stream().cuda_stream
    BF = torch.bfloat16
    case = P['case']
    h, HD = case.h, case.h * 64
    q = P['q'] if q is None else q
    kv_end = P['kv_end'] if kv_end is None else kv_end
    b, lq = case.b if b is None else b, case.lq if lq is None else lq
    R = q.shape[0]
    out = torch.full((R, HD + 24), POISON, device=dev, dtype=torch.int16).view(BF)
    lse = torch.full((b, h, lq), float('nan'), device=dev)
    big = torch.full((R, 8 * ((h + 7) // 8)), BIG_LOGIT, device=dev, dtype=BF)
    kw = dict(q=q, k=P['cache'], v=P['side'] if laser else P['cache'][:, HD:], ld_q=q.stride(0), ld_k=2 * HD, ld_v=HD if laser else 2 * HD,
              gate=None if gate == 'null' else big, ld_gate=big.stride(0), kv_end=kv_end, q_start=torch.zeros(R, device=dev, dtype=torch.int32),
              out=out, ld_out=HD + 24, lse=lse, b=b, h=h, n=lq, n_kv=case.n_kv, softcap=CAP, sc_plan=P['plan'], laser=int(laser))
    if units:
        kw.update(q_row0=torch.tensor(units[0], dtype=torch.int32, device=dev), q_cnt=torch.tensor(units[1], dtype=torch.int32, device=dev))
    capi.call(entry, capi.make_args('tfx_attn_args', **kw), st)
    torch.cuda.synchronize()
    return out, lse
