"""Parameter groups, decoupled weight decay and resumable state of optim.FusedAdam / FusedMuon on the MI355X (csrc/tokenwise.hip `flat_rule_k<adam_rule>`).

Gradients are INJECTED (a seeded tensor in `model.store.grad`, `p.grad` of the external parameters): the training backward sums with fp32 atomics
and is not repeatable to the bit, the optimizer kernels are - with the fixed-order clip norm (`deterministic_norm`) or no clip, where bits are compared.

Bound against torch: allclose(rtol=1e-5, atol=1e-6), the project's bound for this kernel (tests/test_model_gpu.py, fused step against torch.optim.Adam).
Every comparison with torch is a ONE-step comparison: the reference starts each step from the native parameters and moments.

The model (dim 64, depth 2, positional-embedding MLP) has external parameters, and 64-element gains between its matrices: group boundaries fall inside
one 1024-element block of the launch, where the per-block decision of the group must give way to the per-thread one."""
import copy
import io

import pytest
import torch

from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.optim import FusedAdam, FusedMuon, decay_groups

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RTOL, ATOL = 1e-5, 1e-6


def stream():
    return torch.cuda.current_stream().cuda_stream


def small(seed=0):
    torch.manual_seed(seed)
    return Transfusion(num_text_tokens=32, dim_latent=16, add_pos_emb=True, modality_num_dim=1,
                       transformer=dict(dim=64, depth=2, heads=2, dim_head=8)).cuda().train()


def make_grads(model, seed, scale=0.05):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ps = model.store
    flat = torch.randn(ps.numel, device=DEV, generator=gen) * scale
    real = torch.zeros(ps.numel, dtype=torch.bool, device=DEV)
    for n, p in ps.params.items():
        real[ps.offsets[n][0]:ps.offsets[n][0] + p.numel()] = True
    flat = flat * real                                                 # the padding behind a segment carries no gradient
    ext = [torch.randn(p.shape, device=DEV, generator=gen) * scale for p in model.external_parameters()]
    return flat, ext


def inject(model, grads):
    model.store.grad.copy_(grads[0])
    for p, g in zip(model.external_parameters(), grads[1]):
        p.grad = g.clone()                                             # the step scales these in place


def grad_of(model, grads, p):
    """the injected gradient of parameter `p` (a clone, in its shape)"""
    ps = model.store
    for q, g in zip(model.external_parameters(), grads[1]):
        if q is p:
            return g.clone()
    off = (p.data_ptr() - ps.flat.data_ptr()) // 4
    return grads[0][off:off + p.numel()].view(p.shape).clone()


def same_state(a, b, oa, ob):
    assert torch.equal(a.store.flat, b.store.flat), 'parameters differ'
    assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), 'moments differ'
    for p, q in zip(a.external_parameters(), b.external_parameters()):
        assert torch.equal(p, q), 'external parameters differ'
    assert oa.step_count == ob.step_count


def four_groups(model):
    """(a) L2 decay, (b) decoupled decay with its own lr and betas, (c) one gain alone with its own eps, (d) lr 0.  Parameters nobody names (the
    conditioning tables, biases, most gains) fall into (a), the default group."""
    named = dict(model.named_parameters())
    ext = [n for n in named if n.startswith('pos_emb_mlp')]
    a = [n for n, p in named.items() if p.ndim >= 2 and '.layers.0.' in n] + [n for n in ext if n.endswith('weight')]
    b = [n for n, p in named.items() if p.ndim >= 2 and '.layers.1.' in n] + [n for n in ext if n.endswith('bias')]
    c = ['transformer.layers.0.1.layernorm_gamma']
    d = ['text_embed.weight', 'transformer.norm.gamma', 'transformer.layers.1.2.layerscale', 'to_text_logits.weight']
    return [dict(params=a, lr=1e-3, weight_decay=0.1),
            dict(params=b, lr=3e-4, betas=(0.8, 0.95), weight_decay=0.1, decoupled_weight_decay=True),
            dict(params=c, lr=1e-3, eps=1e-6, weight_decay=0.),
            dict(params=d, lr=0., weight_decay=0.)]


def torch_one_step(model, opt, grads, max_norm):
    """clip_grad_norm_ + torch.optim.Adam (AdamW's rule where a group is decoupled) for ONE step from the native state as it is now: returns
    {id(native parameter): (parameter, exp_avg, exp_avg_sq) after the step} over the parameters the Adam rule owns"""
    flat = opt._flat_offsets()
    ref_groups, pairs = [], []
    for g in opt._adam_groups():
        members = [p for p in g['params'] if p.requires_grad]
        clones = [p.detach().clone().requires_grad_(True) for p in members]
        for p, c in zip(members, clones):
            c.grad = grad_of(model, grads, p)
        pairs += list(zip(members, clones))
        ref_groups.append(dict(params=clones, lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'],
                               decoupled_weight_decay=g['decoupled_weight_decay']))
    # the clip norm is over ALL gradients: those of the matrices another rule steps too
    others = [grad_of(model, grads, p) for p in (opt.muon_params if isinstance(opt, FusedMuon) else [])]
    carriers = [torch.nn.Parameter(torch.zeros_like(g)) for g in others]
    for c, g in zip(carriers, others):
        c.grad = g
    torch.nn.utils.clip_grad_norm_([c for _, c in pairs] + carriers, max_norm)
    ref = torch.optim.Adam(ref_groups)
    if opt.step_count:
        for p, c in pairs:
            if id(p) in flat:
                off = flat[id(p)][0]
                ref.state[c] = dict(step=torch.tensor(float(opt.step_count)), exp_avg=opt.m[off:off + p.numel()].view(p.shape).clone(),
                                    exp_avg_sq=opt.v[off:off + p.numel()].view(p.shape).clone())
            else:
                ref.state[c] = {k: v.clone() for k, v in opt.ext_opt.state[p].items()}
    ref.step()
    return {id(p): (c.detach(), ref.state[c]['exp_avg'], ref.state[c]['exp_avg_sq']) for p, c in pairs}


def moments_of(opt, p):
    flat = opt._flat_offsets()
    if id(p) in flat:
        off = flat[id(p)][0]
        return opt.m[off:off + p.numel()].view(p.shape), opt.v[off:off + p.numel()].view(p.shape)
    return opt.ext_opt.state[p]['exp_avg'], opt.ext_opt.state[p]['exp_avg_sq']


def check_three_steps_against_torch(model, opt, seed):
    for step in range(3):
        grads = make_grads(model, seed + step)
        want = torch_one_step(model, opt, grads, 0.5)
        frozen = {id(p): (p.detach().clone(), moments_of(opt, p)[0].clone() if opt.step_count else None) for p in opt.param_groups[3]['params']}
        inject(model, grads)
        opt.step()
        torch.cuda.synchronize()
        worst = 0.
        for g in opt._adam_groups():
            for p in g['params']:
                if not p.requires_grad:
                    continue
                rp, rm, rv = want[id(p)]
                m, v = moments_of(opt, p)
                worst = max(worst, float(((p.detach() - rp).abs() / (ATOL + RTOL * rp.abs())).max()))
                assert torch.allclose(p.detach(), rp, rtol=RTOL, atol=ATOL)
                assert torch.allclose(m, rm, rtol=RTOL, atol=ATOL) and torch.allclose(v, rv, rtol=RTOL, atol=ATOL)
        print(f'  step {step + 1}: worst |native - torch| / (atol + rtol |torch|) = {worst:.3f}')
        for p in opt.param_groups[3]['params']:                    # lr 0: the parameter keeps its bits, its moments move
            before, m0 = frozen[id(p)]
            assert torch.equal(p.detach(), before)
            assert m0 is None or not torch.equal(moments_of(opt, p)[0], m0)
            assert moments_of(opt, p)[0].abs().sum() > 0
        for g in opt.param_groups:                                   # the lr changes between steps
            g['lr'] = g['lr'] * 0.7


# ---------------------------------------------------------------------------------------------------------------- kernel alone
def test_grouped_kernel_is_the_ungrouped_one_per_group():
    """tfx_adam_step_groups on a buffer that is no multiple of the block, with ranges that cut blocks, a gap (elements of no range: group 0) and a
    skip table: every L2 group's elements carry the bits tfx_adam_step gives with that group's scalars, a decoupled group's match torch.optim.AdamW,
    skipped elements are untouched; groups that all carry the global values give the ungrouped launch's bits"""
    n = 100_000
    gen = torch.Generator(device=DEV).manual_seed(3)
    p0, g = torch.randn(n, device=DEV, generator=gen), torch.randn(n, device=DEV, generator=gen) * 0.1
    m0, v0 = torch.randn(n, device=DEV, generator=gen) * 0.01, torch.rand(n, device=DEV, generator=gen) * 1e-3
    sumsq = (g.double() ** 2).sum().float().reshape(1)
    recs = [dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1), dict(lr=1e-3, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.),
            dict(lr=0., beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.3), dict(lr=2e-3, beta1=0.85, beta2=0.98, eps=1e-7, weight_decay=0.2)]
    decoupled = [0, 0, 0, 1]
    # whole blocks (0 .. 4096), boundaries inside a block (4096 .. 6144), a gap (6144 .. 8192: group 0), a long range, a cut 4 short of a block's end, the tail
    ranges = [(0, 4096, 1), (4096, 4100, 2), (4100, 5000, 3), (5000, 6144, 1), (8192, 50_172, 3), (50_172, 51_196, 2), (51_196, 99_996, 1), (99_996, 100_000, 3)]
    skip = [(1024, 1032), (4092, 4104), (60_000, 70_000)]
    group = torch.zeros(n, dtype=torch.long, device=DEV)
    for a, b, k in ranges:
        group[a:b] = k
    skipped = torch.zeros(n, dtype=torch.bool, device=DEV)
    for a, b in skip:
        skipped[a:b] = True
    skip_t = torch.tensor(skip, dtype=torch.int64, device=DEV).reshape(-1)
    common = dict(g=g, n=n, max_norm=0.5, grad_scale=1., step=3, sumsq=sumsq)

    def ungrouped(rec):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        capi.call('tfx_adam_step', capi.make_args('tfx_adam_args', p=p, m=m, v=v, **rec, **common), stream())
        return p, m, v

    def grouped(recs, decoupled, with_skip=True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        tab = torch.tensor(ranges, dtype=torch.int64, device=DEV).reshape(-1)
        a = capi.make_args('tfx_adam_group_args', p=p, m=m, v=v, ranges=tab, nrange=len(ranges), ngroup=len(recs), group_decoupled=decoupled,
                           skip=skip_t if with_skip else None, nskip=len(skip) if with_skip else 0, **recs[0],
                           **{f'group_{k}': [r[k] for r in recs] for k in recs[0]}, **common)
        capi.call('tfx_adam_step_groups', a, stream())
        torch.cuda.synchronize()
        return p, m, v

    got = grouped(recs, decoupled)
    for t, t0 in zip(got, (p0, m0, v0)):
        assert torch.equal(t[skipped], t0[skipped]), 'a skipped element changed'
    for k in (0, 1, 2):
        sel = (group == k) & ~skipped
        assert int(sel.sum()) > 0
        for t, w in zip(got, ungrouped(recs[k])):
            assert torch.equal(t[sel], w[sel]), f'group {k} differs from the ungrouped launch with its scalars'
    assert torch.equal(got[0][(group == 2) & ~skipped], p0[(group == 2) & ~skipped])              # lr 0
    # the decoupled group against torch.optim.AdamW, one step from the same moments
    rp = p0.clone().requires_grad_(True)
    rp.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([rp], 0.5)
    r = recs[3]
    ref = torch.optim.AdamW([rp], lr=r['lr'], betas=(r['beta1'], r['beta2']), eps=r['eps'], weight_decay=r['weight_decay'])
    ref.state[rp] = dict(step=torch.tensor(2.), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    ref.step()
    sel = (group == 3) & ~skipped
    assert torch.allclose(got[0][sel], rp.detach()[sel], rtol=RTOL, atol=ATOL)
    assert torch.allclose(got[1][sel], ref.state[rp]['exp_avg'][sel], rtol=RTOL, atol=ATOL)
    assert not torch.equal(got[0][sel], ungrouped(r)[0][sel])                                      # and it is not the L2 form
    # the ungrouped decoupled launch (no table) is the same rule
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    capi.call('tfx_adam_step_groups', capi.make_args('tfx_adam_group_args', p=p, m=m, v=v, decoupled=1, **r, **common), stream())
    for t, w in zip((p, m, v), got):
        assert torch.equal(t[sel], w[sel])
    # all groups with the global values: the ungrouped launch's bits everywhere; no table and L2: that launch itself
    same = grouped([recs[0]] * 4, [0] * 4, with_skip=False)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    capi.call('tfx_adam_step_groups', capi.make_args('tfx_adam_group_args', p=p, m=m, v=v, **recs[0], **common), stream())
    for t, u, w in zip(same, (p, m, v), ungrouped(recs[0])):
        assert torch.equal(t, w) and torch.equal(u, w)


def test_grouped_kernel_tail_of_a_buffer_that_is_no_multiple_of_four():
    n = 1024 + 7
    gen = torch.Generator(device=DEV).manual_seed(4)
    p0, g = torch.randn(n + 1, device=DEV, generator=gen)[:n], torch.randn(n + 1, device=DEV, generator=gen)[:n] * 0.1
    guard = torch.full((64,), 7., device=DEV)
    bufs = [torch.cat([t, guard]) for t in (p0, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))]
    a = capi.make_args('tfx_adam_group_args', p=bufs[0], g=g.contiguous(), m=bufs[1], v=bufs[2], n=n, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                       weight_decay=0.1, decoupled=1, max_norm=0., grad_scale=1., step=1)
    capi.call('tfx_adam_step_groups', a, stream())
    torch.cuda.synchronize()
    rp = p0.clone().requires_grad_(True)
    rp.grad = g.clone()
    torch.optim.AdamW([rp], lr=1e-3, weight_decay=0.1).step()
    assert torch.allclose(bufs[0][:n], rp.detach(), rtol=RTOL, atol=ATOL)
    for b in bufs:
        assert torch.equal(b[n:], guard), 'written behind the buffer'


# ---------------------------------------------------------------------------------------------------------------- 5. one group / equal groups = no groups
@pytest.mark.parametrize('groups', ['one', 'equal'])
def test_groups_with_the_global_scalars_equal_no_groups(groups):
    """'one': a single explicit group of all parameters.  'equal': decay_groups' two groups plus one gain alone, all with the same scalars - the
    grouped launch, whose arithmetic must be the ungrouped one's to the bit"""
    a, b = small(0), small(0)
    kw = dict(lr=1e-3, betas=(0.85, 0.98), eps=1e-7, weight_decay=0.1, max_grad_norm=0.5)
    if groups == 'one':
        pg = [dict(params=list(a.parameters()), lr=1e-3, betas=(0.85, 0.98), eps=1e-7, weight_decay=0.1)]
    else:
        pg = [dict(params=g['params']) for g in decay_groups(a, 0.)]
        gamma = a.store.params['transformer.layers.1.1.layernorm_gamma']
        pg[1]['params'] = [p for p in pg[1]['params'] if p is not gamma]
        pg.append(dict(params=[gamma]))
    oa, ob = FusedAdam(a, param_groups=pg, **kw), FusedAdam(b, **kw)
    oa.deterministic_norm = ob.deterministic_norm = True
    assert len(oa.group_ranges()) == (1 if groups == 'one' else 21)
    for step in range(2):
        for model in (a, b):
            inject(model, make_grads(model, 10 + step))
        oa.step(); ob.step()
    torch.cuda.synchronize()
    same_state(a, b, oa, ob)
    assert not torch.equal(a.store.flat, small(0).store.flat)


# ---------------------------------------------------------------------------------------------------------------- 6. groups against torch
def test_four_groups_match_torch_adam_and_adamw_step_by_step():
    model = small(1)
    opt = FusedAdam(model, max_grad_norm=0.5, param_groups=four_groups(model))
    assert len(opt.ext_opt.param_groups) == 2 and [g['decoupled_weight_decay'] for g in opt.ext_opt.param_groups] == [False, True]
    ranges = opt.group_ranges()
    assert {k for _, _, k in ranges} == {0, 1, 2, 3}
    assert any(a // 1024 == (b - 1) // 1024 for a, b, _ in ranges), 'no range inside one block: the test lost its point'
    check_three_steps_against_torch(model, opt, seed=20)


# ---------------------------------------------------------------------------------------------------------------- 7. FusedMuon with a grouped Adam share
def test_muon_with_grouped_adam_share():
    a, b = small(2), small(2)
    kw = dict(max_grad_norm=0.5, muon_lr=2e-3, muon_weight_decay=0.05)
    oa, ob = FusedMuon(a, param_groups=four_groups(a), **kw), FusedMuon(b, **kw)
    assert len(oa.param_groups) == 5 and len(oa.muon_params) == 8
    for step in range(2):
        for model in (a, b):
            inject(model, make_grads(model, 30 + step))
        oa.step(); ob.step()
    torch.cuda.synchronize()
    for p, q in zip(a.muon_parameters(), b.muon_parameters()):         # Muon's share does not see the Adam groups
        assert torch.equal(p, q) and torch.equal(oa.momentum_buffer(p), ob.momentum_buffer(q))
    assert not torch.equal(a.store.flat, b.store.flat)
    check_three_steps_against_torch(a, oa, seed=40)


# ---------------------------------------------------------------------------------------------------------------- 8. resume
@pytest.mark.parametrize('cls', [FusedAdam, FusedMuon])
def test_resume_continues_to_the_bit(cls):
    from torch.optim.lr_scheduler import LambdaLR
    warm = lambda s: min(1., (s + 1) / 4)

    def build(seed):
        model = small(seed)
        opt = cls(model, lr=1e-3, max_grad_norm=0.5, param_groups=decay_groups(model, 0.1))
        opt.deterministic_norm = True
        return model, opt, LambdaLR(opt, warm)
    a, oa, sa = build(5)
    for step in range(3):
        inject(a, make_grads(a, 50 + step))
        oa.step(); sa.step()
    blob = io.BytesIO()
    torch.save(dict(model=a.state_dict(), opt=oa.state_dict(), sched=sa.state_dict()), blob)
    blob.seek(0)
    ck = torch.load(blob, map_location=DEV)
    b, ob, sb = build(6)
    assert not torch.equal(a.store.flat, b.store.flat)
    b.load_state_dict(ck['model']); ob.load_state_dict(ck['opt']); sb.load_state_dict(ck['sched'])
    same_state(a, b, oa, ob)
    assert [g['lr'] for g in oa.param_groups] == [g['lr'] for g in ob.param_groups] and sa.get_last_lr() == sb.get_last_lr()
    for step in range(3, 5):
        for model, opt, sched in ((a, oa, sa), (b, ob, sb)):
            inject(model, make_grads(model, 50 + step))
            opt.step(); sched.step()
        assert [g['lr'] for g in oa.param_groups] == [g['lr'] for g in ob.param_groups]
    torch.cuda.synchronize()
    same_state(a, b, oa, ob)
    assert oa.step_count == 5
    # a cold restart - weights only - does NOT continue the same way
    c, oc, _ = build(6)
    c.load_state_dict(ck['model'])
    inject(c, make_grads(c, 53)); oc.step()
    assert oc.step_count == 1


# ---------------------------------------------------------------------------------------------------------------- 9. interchange with torch
def set_param_grads(model, grads):
    for p in model.parameters():
        if p.requires_grad:
            p.grad = grad_of(model, grads, p)


def test_state_interchange_with_torch_adam_and_adamw():
    # torch.optim.Adam -> FusedAdam
    a, b = small(7), small(8)
    ta = torch.optim.Adam(a.parameters(), lr=3e-4)
    for step in range(2):
        set_param_grads(a, make_grads(a, 60 + step))
        ta.step()
    b.load_state_dict(a.state_dict())
    ob = FusedAdam(b)
    ob.load_state_dict(ta.state_dict())
    assert ob.step_count == 2 and ob.lr == 3e-4
    grads = make_grads(a, 62)
    set_param_grads(a, grads); ta.step()
    inject(b, grads); ob.step()
    torch.cuda.synchronize()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p.detach(), q.detach(), rtol=RTOL, atol=ATOL), n
    # FusedAdam(decoupled) -> torch.optim.AdamW
    a, b = small(9), small(10)
    oa = FusedAdam(a, lr=1e-3, weight_decay=0.1, decoupled_weight_decay=True)
    for step in range(2):
        inject(a, make_grads(a, 70 + step))
        oa.step()
    b.load_state_dict(a.state_dict())
    tb = torch.optim.AdamW(b.parameters(), lr=5e-2, weight_decay=0.)
    tb.load_state_dict(copy.deepcopy(oa.state_dict()))               # (torch keeps same-device tensors of a state dict as they are: the moments are views of oa.m)
    assert tb.param_groups[0]['lr'] == 1e-3 and tb.param_groups[0]['weight_decay'] == 0.1 and tb.param_groups[0]['decoupled_weight_decay'] is True
    grads = make_grads(a, 72)
    inject(a, grads); oa.step()
    set_param_grads(b, grads); tb.step()
    torch.cuda.synchronize()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p.detach(), q.detach(), rtol=RTOL, atol=ATOL), n
    assert float(tb.state[next(iter(b.store.params.values()))]['step']) == 3. == oa.step_count


# ---------------------------------------------------------------------------------------------------------------- 10. end to end
def test_training_with_decay_groups_scheduler_and_a_checkpoint_halfway():
    """the model of test_laser_text_only_training_loss_falls (train_text_only.py's), without LASER, at depth 2: decay groups, clip, a warm-up
    schedule, 40 steps, a checkpoint written and loaded in place after 20; that test's criterion"""
    from torch.optim.lr_scheduler import LambdaLR
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=256, transformer=dict(dim=384, depth=2, dim_head=64, heads=8)).cuda().train()
    opt = FusedAdam(model, lr=3e-4, param_groups=decay_groups(model, 0.1), max_grad_norm=0.5)
    sched = LambdaLR(opt, lambda s: min(1., (s + 1) / 10))
    g = torch.Generator().manual_seed(0)
    phrases = torch.randint(0, 256, (16, 32), generator=g)
    losses = []
    for step in range(40):
        idx = torch.randint(0, 16, (8, 8), generator=g)
        batch = phrases[idx].reshape(8, -1)[:, :257].cuda()
        loss = model.forward_text(batch)
        loss.backward()
        opt.step(); opt.zero_grad(); sched.step()
        losses.append(float(loss))
        if step == 19:
            blob = io.BytesIO()
            torch.save(dict(model=model.state_dict(), opt=opt.state_dict(), sched=sched.state_dict()), blob)
            blob.seek(0)
            ck = torch.load(blob, map_location=DEV)
            with torch.no_grad():
                model.store.flat.zero_()                             # what is loaded is what the run goes on with
            opt.m.fill_(1.); opt.step_count = 0
            model.load_state_dict(ck['model']); opt.load_state_dict(ck['opt']); sched.load_state_dict(ck['sched'])
            assert opt.step_count == 20 and opt.lr == pytest.approx(3e-4)
    print(f'  loss {losses[0]:.3f} -> {losses[-1]:.3f}')
    assert all(torch.isfinite(torch.tensor(losses)))
    assert sum(losses[-5:]) / 5 < 0.8 * sum(losses[:5]) / 5
