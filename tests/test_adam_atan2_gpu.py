"""The Adam-atan2 rule on the MI355X: `tfx_adam_atan2_step` (csrc/tokenwise.hip `flat_rule_k<atan2_rule>`) through the C ABI, element by element against the fp64
reference and the per-element bound of tests/_adam_atan2_cases.py (which derives the bound and says where the atan2f figure was read), with guard
bands around p, m and v; then optim.FusedAdamAtan2 / FusedMuonAdamAtan2 on a small model, their checkpoints, and the example script.

Where bits are compared the gradients are INJECTED (the training backward sums with fp32 atomics and is not repeatable to the bit; the optimizer
launches are, with the fixed-order clip norm).  The model (dim 64, depth 2, heads 2, a positional-embedding MLP) has external parameters and 64-element
gains between its matrices: group boundaries fall inside one 1024-element block of the launch."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

import _adam_atan2_cases as C
from transfusion_pytorch_amd import Transfusion, capi

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64                                    # elements in front of and behind every written buffer (a multiple of 4: the buffers stay 16-byte aligned)
SENTINEL = 0x4B1D5EED                         # the guard bands' bit pattern (a finite float)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]  # the cnt < 4 tail, one block, a block boundary, several blocks


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(x):
    """(whole buffer, the n elements in the middle) with GUARD sentinel elements on both sides"""
    n = x.size
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    whole[GUARD:GUARD + n].copy_(torch.from_numpy(x))
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    bits = whole.view(torch.int32)
    return bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + n:] == SENTINEL).all())


VARIANTS = {
    # name: (step, state, grouped, skip, clip: max_norm as a fraction of the gradient norm, ungrouped group)
    'plain step 1':            (1, False, False, False, 0., dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.)),
    'L2 decay step 1000':      (1000, True, False, False, 0., dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1)),
    'decoupled decay, clip':   (2, True, False, False, 0.5, dict(lr=5e-2, betas=(0.8, 0.95), weight_decay=0.5, decoupled_weight_decay=True)),
    'skip table':              (2, True, False, True, 0., dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.)),
    'three groups':            (1, False, True, False, 0., None),
    'groups, skip, clip':      (1000, True, True, True, 0.5, None),
}


def launch(n, p, g, m, v, step, groups, ranges, skip, max_norm, a, b, sumsq=None):
    """one tfx_adam_atan2_step over guarded copies of p, m, v: returns (p, m, v) as numpy and checks the guard bands"""
    return launch_entry('tfx_adam_atan2_step', 'tfx_adam_atan2_args', dict(eps=123., atan2_a=a, atan2_b=b), 456., n, p, g, m, v, step, groups, ranges,
                        skip, max_norm, sumsq)


def launch_adam_groups(n, p, g, m, v, step, groups, ranges, skip, max_norm, eps, sumsq=None):
    """the same for one tfx_adam_step_groups (the other rule of the kernel template), every group with `eps`"""
    return launch_entry('tfx_adam_step_groups', 'tfx_adam_group_args', dict(eps=eps), eps, n, p, g, m, v, step, groups, ranges, skip, max_norm, sumsq)


def launch_entry(entry, struct_, fields, group_eps, n, p, g, m, v, step, groups, ranges, skip, max_norm, sumsq):
    (wp, dp), (wm, dm), (wv, dv) = guarded(p), guarded(m), guarded(v)
    dg = torch.from_numpy(g).to(DEV)
    g0 = groups[0]
    kw = dict(p=dp, g=dg, m=dm, v=dv, n=n, lr=g0['lr'], beta1=g0['betas'][0], beta2=g0['betas'][1], weight_decay=g0.get('weight_decay', 0.),
              decoupled=int(g0.get('decoupled_weight_decay', False)), max_norm=max_norm, grad_scale=1., step=step, **fields)
    keep = [dg]
    if max_norm > 0:
        keep.append(torch.tensor([sumsq], dtype=torch.float32, device=DEV)); kw['sumsq'] = keep[-1]
    if ranges:
        keep.append(torch.tensor(ranges, dtype=torch.int64, device=DEV).reshape(-1))
        kw.update(ranges=keep[-1], nrange=len(ranges), ngroup=len(groups), group_lr=[x['lr'] for x in groups], group_beta1=[x['betas'][0] for x in groups],
                  group_beta2=[x['betas'][1] for x in groups], group_eps=[group_eps] * len(groups), group_weight_decay=[x.get('weight_decay', 0.) for x in groups],
                  group_decoupled=[int(x.get('decoupled_weight_decay', False)) for x in groups])
    if skip:
        keep.append(torch.tensor(skip, dtype=torch.int64, device=DEV).reshape(-1))
        kw.update(skip=keep[-1], nskip=len(skip))
    capi.call(entry, capi.make_args(struct_, **kw), stream())
    torch.cuda.synchronize()
    for w in (wp, wm, wv):
        assert guards_intact(w, n), 'written outside the buffer'
    return tuple(t.cpu().numpy() for t in (dp, dm, dv))


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_kernel_element_by_element(variant):
    step, state, grouped, with_skip, clip, group = VARIANTS[variant]
    a, b = 1.27, 0.5 if grouped else 1.
    for n in SIZES:
        p, g, m, v = C.make_inputs(n, seed=n + step, gscale=0.05, state=state)
        groups, ranges, gidx = [group], None, None
        if grouped:
            groups = C.three_groups()
            ranges, gidx = C.group_layout(n)
        skip = C.skip_layout(n) if with_skip else None
        sumsq = float(np.float32((g.astype(np.float64) ** 2).sum()))
        max_norm = clip * float(np.sqrt(sumsq))                              # whatever n, the clip roughly halves the gradient
        coef = C.coef_f32(sumsq, max_norm)
        got = launch(n, p, g, m, v, step, groups, ranges, skip, max_norm, a, b, sumsq)
        kw = dict(step=step, groups=groups, gidx=gidx, coef=coef, a=a, b=b, skip=skip)
        ref, bnd = C.ref64(p, g, m, v, **kw), C.bound(p, g, m, v, **kw)
        print(f'  n {n}: worst |kernel - ref64| / bound = {C.worst(got, ref, bnd):.3f}')
        assert C.over(got, ref, bnd) == 0, n
        for s, e in (skip or ()):
            for t, t0 in zip(got, (p, m, v)):
                assert np.array_equal(t[s:e].view(np.uint32), t0[s:e].view(np.uint32)), 'a skipped element changed'
        if max_norm > 0:
            assert 0.4 < coef < 0.6                                          # the clip is on
        assert not np.array_equal(got[0], p)


def test_kernel_leaves_zero_gradient_on_zero_state_alone():
    for n in SIZES:
        p = C.make_inputs(n, seed=n)[0]
        p[0] = -0.
        z = np.zeros(n, dtype=np.float32)
        got = launch(n, p, z, z, z, 1, [dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.)], None, None, 0., 1.27, 1.)
        assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32)), n
        assert not got[1].any() and not got[2].any()


def test_kernel_argument_errors_launch_nothing():
    n = 1024
    p, g, m, v = C.make_inputs(n, seed=0)
    bufs = [torch.from_numpy(t).to(DEV) for t in (p, g, m, v)]
    tab = torch.tensor([0, n, 0], dtype=torch.int64, device=DEV)
    ok = dict(p=bufs[0], g=bufs[1], m=bufs[2], v=bufs[3], n=n, lr=1e-3, beta1=0.9, beta2=0.99, grad_scale=1., step=1, atan2_a=1.27, atan2_b=1.)
    call = lambda **kw: capi.lib().tfx_adam_atan2_step(ctypes.byref(capi.make_args('tfx_adam_atan2_args', **{**ok, **kw})), stream())
    assert call(atan2_a=0.) != 0
    assert call(atan2_b=-1.) != 0
    assert call(p=bufs[0].data_ptr() + 4, n=n - 4) != 0                      # where tfx_adam_step_groups rejects a pointer: 16-byte alignment
    assert call(ranges=tab, nrange=1, ngroup=0) != 0
    assert call(max_norm=0.5) != 0                                           # a clip without the sum of squares
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, (p, g, m, v)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), t0.view(np.uint32)), 'a refused call wrote'
    assert call() == 0
    torch.cuda.synchronize()
    assert not np.array_equal(bufs[0].cpu().numpy(), p)


def test_launch_is_repeatable_to_the_bit():
    n = 100_003
    p, g, m, v = C.make_inputs(n, seed=11, gscale=0.05)
    ranges, _ = C.group_layout(n)
    sumsq = float(np.float32((g.astype(np.float64) ** 2).sum()))
    runs = [launch(n, p, g, m, v, 3, C.three_groups(), ranges, C.skip_layout(n), 0.5, 1.27, 0.5, sumsq) for _ in range(2)]
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_moments_are_the_same_bits_under_both_rules():
    """the two rules are one kernel template (`flat_rule_k`) and differ in the update of p alone: over the same inputs, groups, skip table and clip,
    tfx_adam_atan2_step and tfx_adam_step_groups leave the same bits in m and v"""
    step, bits = 2, lambda t: t.view(np.uint32)
    for n in SIZES:
        p, g, m, v = C.make_inputs(n, seed=n + step, gscale=0.05, state=True)
        groups, (ranges, _), skip = C.three_groups(), C.group_layout(n), C.skip_layout(n)
        sumsq = float(np.float32((g.astype(np.float64) ** 2).sum()))
        max_norm = 0.5 * float(np.sqrt(sumsq))
        assert 0.4 < C.coef_f32(sumsq, max_norm) < 0.6                       # the clip is on
        atan2 = launch(n, p, g, m, v, step, groups, ranges, skip, max_norm, 1.27, 0.5, sumsq)
        adam = launch_adam_groups(n, p, g, m, v, step, groups, ranges, skip, max_norm, 1e-8, sumsq)
        assert np.array_equal(bits(atan2[1]), bits(adam[1])) and np.array_equal(bits(atan2[2]), bits(adam[2])), n
        assert not np.array_equal(atan2[1], m) and not np.array_equal(atan2[2], v), n
        for s, e in skip:
            for got in (atan2, adam):
                for t, t0 in zip(got, (p, m, v)):
                    assert np.array_equal(bits(t[s:e]), bits(t0[s:e])), 'a skipped element changed'
        assert not np.array_equal(atan2[0], adam[0]), n


# ---------------------------------------------------------------------------------------------------------------- the optimizer classes
def small(seed=0):
    torch.manual_seed(seed)
    return Transfusion(num_text_tokens=32, dim_latent=16, add_pos_emb=True, modality_num_dim=1,
                       transformer=dict(dim=64, depth=2, heads=2, dim_head=8)).cuda().train()


def ragged_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    ids = lambda k: torch.randint(0, 32, (k,), generator=gen).cuda()
    lat = lambda k: torch.randn(k, 16, generator=gen).cuda()
    return [[ids(5), lat(4), ids(3)], [ids(7), lat(6)], [ids(2), lat(3), ids(4), lat(2)]]


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


def same_state(a, b, oa, ob):
    assert torch.equal(a.store.flat, b.store.flat), 'parameters differ'
    assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), 'moments differ'
    for p, q in zip(a.external_parameters(), b.external_parameters()):
        assert torch.equal(p, q), 'external parameters differ'
    assert oa.step_count == ob.step_count


def in_range(gc):
    """the supported magnitudes of tfx.h: g coef is zero or a normal fp32 number whose square is normal too"""
    mag = np.abs(gc.astype(np.float64))
    return (mag == 0) | ((mag >= 1e-18) & (mag <= 1e18))


def snapshot(model, opt):
    """everything the reference needs, taken between the backward and the step: parameters, gradients and moments of the flat buffer and of every
    external parameter"""
    ps = model.store
    zeros = lambda t: torch.zeros_like(t)
    flat = [t.clone().cpu().numpy() for t in (ps.flat, ps.grad, opt.m if opt.m is not None else zeros(ps.flat), opt.v if opt.v is not None else zeros(ps.flat))]
    ext = []
    for p in opt.ext_params:
        st = opt.ext_opt.state.get(p) or {}
        ext.append([t.detach().clone().cpu().numpy().reshape(-1) for t in (p, p.grad, st.get('exp_avg', zeros(p)), st.get('exp_avg_sq', zeros(p)))])
    return flat, ext


def held_outside(got, start, kw, out):
    """the elements whose gradient is outside the supported magnitudes are not held to ref64 (v underflows or overflows there) but to what the rule
    promises for ANY finite gradient: p finite, m and v no NaN (v may overflow above the range), |p_new - keep p| <= lr a pi / 2 (plus the three roundings
    of the fp32 form: keep, keep p, the subtraction)"""
    if not out.any():
        return True
    w, cap = C.step_cap(*start, **kw)
    p = got[0].astype(np.float64)
    finite = np.isfinite(p[out]).all() and not any(np.isnan(x[out]).any() for x in got)
    return bool(finite and (np.abs(p - w)[out] <= (cap + 3 * C.U * np.abs(p) * C.SECOND_ORDER)[out]).all())


def group_of(opt, p):
    return next(g for g in opt._adam_groups() if any(q is p for q in g['params']))


def check_step(model, opt, before, max_norm, skip=None):
    """the step that just ran against ref64, every element of the flat buffer and of the external parameters - inside the supported magnitudes of the gradient against
    ref64 and the bound, outside them (`held_outside`) against what the rule promises for any gradient"""
    ps = model.store
    flat, ext = before
    t = opt.step_count
    groups = [dict(lr=g['lr'], betas=g['betas'], weight_decay=g['weight_decay'], decoupled_weight_decay=g['decoupled_weight_decay']) for g in opt._adam_groups()]
    gidx = np.zeros(ps.numel, dtype=np.int64)
    for s, e, k in opt.group_ranges():
        gidx[s:e] = k
    coef = C.coef_f32(float(opt.sumsq[0]), max_norm)
    kw = dict(step=t, groups=groups, gidx=gidx, coef=coef, a=opt.a, b=opt.b, skip=skip)
    ref, bnd = C.ref64(*flat, **kw), C.bound(*flat, **kw)
    got = tuple(x.detach().cpu().numpy() for x in (ps.flat, opt.m, opt.v))
    inside = in_range(flat[1] * np.float32(coef))
    ok = inside & ~C.skip_mask(skip, ps.numel)                               # (the other rule's elements: its own tests)
    print(f'  step {t}: clip coefficient {float(coef):.4f}, {int((~inside).sum())} of {ps.numel} elements outside the supported magnitudes (left out), '
          f'{int(ok.sum())} checked, worst |native - ref64| / bound = {C.worst([x[ok] for x in got], [x[ok] for x in ref], [x[ok] for x in bnd]):.3f}')
    assert inside.mean() > 0.99 and ok.sum() > 0.5 * ps.numel
    assert C.over([x[ok] for x in got], [x[ok] for x in ref], [x[ok] for x in bnd]) == 0
    assert held_outside(got, flat, kw, ~inside & ~C.skip_mask(skip, ps.numel)), 'an element outside the supported magnitudes is not finite or moved too far'
    # the external parameters: their gradients are scaled by the step's own fp32 coefficient (optim.FusedAdam.step), then AdamAtan2
    ecoef = 1.
    if max_norm > 0:
        ecoef = float((torch.full((), 1., device=DEV) * (max_norm / (opt.sumsq[0].sqrt() * 1. + 1e-6)).clamp(max=1.)).cpu())
    assert len(opt.ext_params) > 0
    for p, (p0, g0, m0, v0) in zip(opt.ext_params, ext):
        grp = group_of(opt, p)
        kw = dict(step=t, groups=[dict(lr=grp['lr'], betas=grp['betas'], weight_decay=grp['weight_decay'], decoupled_weight_decay=grp['decoupled_weight_decay'])],
                  coef=ecoef, a=opt.a, b=opt.b)
        st = opt.ext_opt.state[p]
        got = tuple(x.detach().cpu().numpy().reshape(-1) for x in (p, st['exp_avg'], st['exp_avg_sq']))
        ok = in_range(g0 * np.float32(ecoef))
        ref, bnd = C.ref64(p0, g0, m0, v0, **kw), C.bound(p0, g0, m0, v0, form='torch', **kw)      # AdamAtan2's operations: no fma
        assert C.over([x[ok] for x in got], [x[ok] for x in ref], [x[ok] for x in bnd]) == 0
        assert held_outside(got, (p0, g0, m0, v0), kw, ~ok)
        assert float(st['step']) == t and not np.array_equal(got[0], p0)


@pytest.mark.parametrize('grouped', [False, True])
def test_fused_adam_atan2_three_real_steps(grouped):
    from transfusion_pytorch_amd.optim import FusedAdamAtan2, decay_groups
    model = small(1)
    kw = dict(param_groups=decay_groups(model, 0.1)) if grouped else dict(weight_decay=0.05)
    opt = FusedAdamAtan2(model, lr=1e-3, max_grad_norm=0.5, **kw)
    opt.deterministic_norm = True
    if grouped:
        ranges = opt.group_ranges()
        assert {k for _, _, k in ranges} == {0, 1} and any(a // 1024 == (b - 1) // 1024 for a, b, _ in ranges), 'no range inside one block'
    for step in range(3):
        loss = model(ragged_batch(step))
        loss.backward()
        torch.cuda.synchronize()
        before = snapshot(model, opt)
        opt.step()
        torch.cuda.synchronize()
        check_step(model, opt, before, 0.5)
        opt.zero_grad()
        for g in opt.param_groups:                                     # the lr changes between steps
            g['lr'] = g['lr'] * 0.7
    assert torch.isfinite(loss)


def test_resume_continues_to_the_bit():
    from transfusion_pytorch_amd.optim import FusedAdamAtan2, decay_groups

    def build(seed):
        model = small(seed)
        opt = FusedAdamAtan2(model, lr=1e-3, max_grad_norm=0.5, param_groups=decay_groups(model, 0.1))
        opt.deterministic_norm = True
        return model, opt
    a, oa = build(5)
    for step in range(2):
        inject(a, make_grads(a, 50 + step)); oa.step()
    blob = io.BytesIO()
    torch.save(dict(model=a.state_dict(), opt=oa.state_dict()), blob)
    blob.seek(0)
    ck = torch.load(blob, map_location=DEV)
    sd = ck['opt']
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'} and all('eps' not in g for g in sd['param_groups'])
    b, ob = build(6)
    b.load_state_dict(ck['model']); ob.load_state_dict(sd)
    same_state(a, b, oa, ob)
    for model, opt in ((a, oa), (b, ob)):
        inject(model, make_grads(model, 52)); opt.step()
    torch.cuda.synchronize()
    same_state(a, b, oa, ob)
    assert ob.step_count == 3
    c, oc = build(6)                                                     # a cold restart - weights only - does NOT continue the same way
    c.load_state_dict(ck['model'])
    inject(c, make_grads(c, 52)); oc.step()
    torch.cuda.synchronize()
    assert not torch.equal(c.store.flat, a.store.flat)


def test_fused_adam_state_loads_into_the_atan2_rule():
    from transfusion_pytorch_amd.optim import FusedAdam, FusedAdamAtan2
    a, b = small(7), small(8)
    oa = FusedAdam(a, lr=3e-4)
    for step in range(2):
        inject(a, make_grads(a, 60 + step)); oa.step()
    b.load_state_dict(a.state_dict())
    ob = FusedAdamAtan2(b, lr=2e-4)
    ob.load_state_dict(oa.state_dict())
    assert ob.step_count == 2 and ob.lr == 2e-4 and 'eps' not in ob.param_groups[0]
    assert torch.equal(ob.m, oa.m) and torch.equal(ob.v, oa.v) and float(ob.m.abs().sum()) > 0
    for p, q in zip(a.external_parameters(), b.external_parameters()):
        assert torch.equal(oa.ext_opt.state[p]['exp_avg'], ob.ext_opt.state[q]['exp_avg'])
    grads = make_grads(b, 62)                                            # and the loaded moments are what the next step uses
    inject(b, grads)
    before = snapshot(b, ob)
    ob.step()
    torch.cuda.synchronize()
    check_step(b, ob, before, 0.)


def test_muon_share_is_fused_muons_and_the_rest_follows_atan2(monkeypatch):
    from transfusion_pytorch_amd.optim import FusedMuon, FusedMuonAdamAtan2
    a, b = small(2), small(2)
    kw = dict(lr=1e-3, max_grad_norm=0.5, muon_lr=2e-3, muon_weight_decay=0.05)
    oa, ob = FusedMuonAdamAtan2(a, **kw), FusedMuon(b, **kw)
    assert oa.launches_per_step() == ob.launches_per_step()
    calls = []
    real_call, real_check = capi.call, capi.check
    monkeypatch.setattr(capi, 'call', lambda name, *r: (calls.append(name), real_call(name, *r))[1])
    monkeypatch.setattr(capi, 'check', lambda rc, what: (calls.append(what), real_check(rc, what))[1])
    seqs = []
    for model, opt in ((a, oa), (b, ob)):
        inject(model, make_grads(model, 30))
        if opt is oa:
            before = snapshot(model, opt)
        calls.clear()
        opt.step()
        seqs.append(list(calls))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seqs[0]) == len(seqs[1]) and seqs[0][:-1] == seqs[1][:-1]        # the same launches, in the same order ...
    assert (seqs[0][-1], seqs[1][-1]) == ('tfx_adam_atan2_step', 'tfx_adam_step')  # ... up to the one at the end of the chain
    for p, q in zip(a.muon_parameters(), b.muon_parameters()):
        assert torch.equal(p, q) and torch.equal(oa.momentum_buffer(p), ob.momentum_buffer(q))
    assert not torch.equal(a.store.flat, b.store.flat)
    check_step(a, oa, before, 0.5, skip=oa.adam_skip_table())                # every element Muon does not own


def test_example_image_flow_with_muon_and_atan2():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import image_flow_unet as ex
    losses, images = ex.main(steps=60, log=lambda *a: None, muon=True, atan2=True)
    assert all(l == l and abs(l) != float('inf') for l in losses)
    first, last = sum(losses[:10]) / 10, sum(losses[-10:]) / 10
    print(f'  loss: first 10 steps {first:.3f} -> last 10 steps {last:.3f}')
    assert last < 0.9 * first
    assert images.shape == (4, 1, 28, 28)
