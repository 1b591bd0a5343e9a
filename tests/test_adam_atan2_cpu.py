"""Host side of the Adam-atan2 rule (no GPU): the C ABI of tfx_adam_atan2_step, the fp64 reference and the per-element bound of
tests/_adam_atan2_cases.py (an fp32 emulation of the kernel's arithmetic stays inside the bound, every injected fault leaves it), the rule's
properties on the reference and on optim.AdamAtan2, and the constructors of FusedAdamAtan2 / FusedMuonAdamAtan2 on models left on the CPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _adam_atan2_cases as C
from transfusion_pytorch_amd import Transfusion, capi

GROUP_ARGS_FIELDS = ['p', 'g', 'm', 'v', 'n', 'lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'max_norm', 'grad_scale', 'step', 'sumsq', 'skip', 'nskip',
                     'decoupled', 'ranges', 'nrange', 'ngroup', 'group_lr', 'group_beta1', 'group_beta2', 'group_eps', 'group_weight_decay', 'group_decoupled']


def small():
    torch.manual_seed(0)
    return Transfusion(num_text_tokens=32, dim_latent=16, add_pos_emb=True, modality_num_dim=1, transformer=dict(dim=64, depth=2, heads=2, dim_head=8))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_of_the_atan2_launch():
    assert [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_args']] == GROUP_ARGS_FIELDS[:16]
    assert [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_group_args']] == GROUP_ARGS_FIELDS
    fields = [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_atan2_args']]
    assert fields == GROUP_ARGS_FIELDS + ['atan2_a', 'atan2_b']
    old, new = capi.STRUCTS['tfx_adam_group_args'], capi.STRUCTS['tfx_adam_atan2_args']
    for f in GROUP_ARGS_FIELDS:
        assert getattr(old, f).offset == getattr(new, f).offset and getattr(old, f).size == getattr(new, f).size, f
    assert new.atan2_a.size == new.atan2_b.size == 4 and new.atan2_b.offset == new.atan2_a.offset + 4
    assert new.atan2_a.offset == old.group_decoupled.offset + 4 * 8
    assert 'tfx_adam_atan2_step' in capi.FUNCTIONS and hasattr(capi.lib(), 'tfx_adam_atan2_step')
    op = capi.ENUMS['TFX_OP_ADAM_ATAN2_STEP']
    assert op < capi.ENUMS['TFX_OP_OUTPUT_TO_FLOW']                          # a struct entry point of the launch lists
    assert sum(1 for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_') and v == op) == 1
    assert b'atan2' in capi.lib().tfx_version()


def test_atan2_launch_refuses_bad_arguments_on_the_host():
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.addressof(buf) & ~15
    ok = dict(p=ptr, g=ptr, m=ptr, v=ptr, n=4, lr=1e-3, beta1=0.9, beta2=0.99, step=1, grad_scale=1., atan2_a=1.27, atan2_b=1.)
    call = lambda **kw: capi.lib().tfx_adam_atan2_step(ctypes.byref(capi.make_args('tfx_adam_atan2_args', **{**ok, **kw})), None)
    assert call(n=0) == 0                                                    # nothing to do
    assert call(atan2_a=0.) != 0 and call(atan2_a=-1.) != 0 and call(atan2_b=0.) != 0 and call(atan2_a=float('nan')) != 0
    assert call(n=0, atan2_a=0.) != 0
    assert call(p=ptr + 4) != 0 and call(v=ptr + 8) != 0                     # 16-byte alignment
    assert call(nrange=1, ngroup=1) != 0                                     # a count without a table
    assert call(nrange=1, ranges=ptr, ngroup=0) != 0 and call(nrange=1, ranges=ptr, ngroup=9) != 0 and call(nrange=-1) != 0
    assert call(nskip=2) != 0
    assert call(max_norm=0.5) != 0                                           # a clip without the sum of squares
    assert call(step=0) != 0


# ---------------------------------------------------------------------------------------------------------------- reference, bound, emulation
def layout(n, grouped):
    if not grouped:
        return [dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.)], None, None
    _, gidx = C.group_layout(n)
    return C.three_groups(), gidx, C.skip_layout(n)


@pytest.mark.parametrize('gscale', [1e-6, 1., 1e4])
@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('decay', [False, True])
def test_emulation_is_inside_the_bound(gscale, step, decay):
    """the fp32 emulation against ref64: no element of p, m, v over the bound, nothing left out"""
    n = 4099
    p, g, m, v = C.make_inputs(n, seed=step, gscale=gscale, state=step > 1)
    groups, gidx, skip = layout(n, decay)                                    # with decay: L2, decoupled and plain groups, a skip table
    kw = dict(step=step, groups=groups, gidx=gidx, coef=0.37 if decay else 1., b=0.5 if decay else 1., skip=skip)
    got = C.emulate(p, g, m, v, **kw)
    ref, bnd = C.ref64(p, g, m, v, **kw), C.bound(p, g, m, v, **kw)
    print(f'  worst |emulation - ref64| / bound = {C.worst(got, ref, bnd):.3f}')
    assert C.over(got, ref, bnd) == 0
    if skip:
        for t, t0 in zip(got, (p, m, v)):
            assert all(np.array_equal(t[s:e], t0[s:e]) for s, e in skip)


@pytest.mark.parametrize('fault', C.FAULTS)
def test_every_injected_fault_leaves_the_bound(fault):
    """one case on which every fault shows: step 2 (both bias corrections far from 1), three groups with their own lr over boundaries inside a block,
    a skip table, a = 1.27 and b = 0.5, gradients of 1e-6 (an eps of 1e-8 is 1 % of the denominator)"""
    n = 4099
    p, g, m, v = C.make_inputs(n, seed=7, gscale=1e-6)
    groups, gidx, skip = layout(n, True)
    kw = dict(step=2, groups=groups, gidx=gidx, coef=0.37, b=0.5, skip=skip)
    ref, bnd = C.ref64(p, g, m, v, **kw), C.bound(p, g, m, v, **kw)
    assert C.over(C.emulate(p, g, m, v, **kw), ref, bnd) == 0
    bad = C.over(C.emulate(p, g, m, v, fault=fault, **kw), ref, bnd)
    print(f'  {fault}: {bad} elements over the bound')
    assert bad >= 1


# ---------------------------------------------------------------------------------------------------------------- properties
def run_ref64(p, grads, groups, a=1.27, b=1.):
    m, v, out = np.zeros_like(p), np.zeros_like(p), []
    for t, g in enumerate(grads, 1):
        p, m, v = C.ref64(p, g, m, v, t, groups, a=a, b=b)
        p, m, v = (x.astype(np.float32) for x in (p, m, v))                  # ref64 takes fp32 inputs
        out.append(p)
    return out


def run_torch(opt_fn, p0, grads):
    p = torch.nn.Parameter(torch.tensor(p0))
    opt, out = opt_fn([p]), []
    for g in grads:
        p.grad = torch.tensor(g)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


def atan2_opt(**kw):
    from transfusion_pytorch_amd.optim import AdamAtan2
    return lambda ps: AdamAtan2(ps, **kw)


@pytest.mark.parametrize('decoupled', [False, True])
def test_step_is_bounded(decoupled):
    """|p_new - keep p| <= lr a pi / 2, whatever the gradient (here over 24 orders of magnitude, both signs, with decoupled decay)"""
    rng = np.random.default_rng(0)
    n, lr, a, wd = 2048, 1e-2, 1.27, 0.1 if decoupled else 0.
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10. ** rng.uniform(-12, 12, n)).astype(np.float32) for _ in range(3)]
    grp = dict(lr=lr, betas=(0.9, 0.99), weight_decay=wd, decoupled_weight_decay=decoupled)
    keep = 1. - C.f32(lr) * C.f32(wd)
    cap = C.f32(lr) * C.f32(a) * math.pi / 2
    for name, traj in (('ref64', run_ref64(p0, grads, [grp], a=a)), ('AdamAtan2', run_torch(atan2_opt(a=a, **grp), p0, grads))):
        prev = p0
        for p in traj:
            move = np.abs(p.astype(np.float64) - keep * prev.astype(np.float64))
            assert (move <= cap + 3 * C.U * np.abs(p) * C.SECOND_ORDER).all(), name   # keep rounded (1), keep p (1), the subtraction (1): fp32 results
            prev = p
        assert np.abs(traj[0].astype(np.float64) - keep * p0).max() > 0.49 * cap   # and the cap is not far: step 1 moves every element by lr a pi / 4


def test_zero_gradient_on_zero_state_moves_nothing():
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(1000).astype(np.float32)
    p0[:4] = [0., -0., 1e-40, -3e38]
    zero = [np.zeros_like(p0)] * 2
    grp = dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.)
    for traj in (run_ref64(p0, zero, [grp]), run_torch(atan2_opt(**grp), p0, zero)):
        for p in traj:
            assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(C.emulate(p0, zero[0], zero[0], zero[0], 1, [grp])[0].view(np.uint32), p0.view(np.uint32))


@pytest.mark.parametrize('k', [-8, 8])
def test_gradient_scale_does_not_change_the_trajectory_and_does_change_adams(k):
    """scaling every gradient of every step by 2^k (no clip, no L2 decay): the atan2 trajectories agree within the bound accumulated over the steps,
    plain Adam's (eps 1e-8, gradients of 1e-6) visibly do not - the test can tell the rules apart"""
    rng = np.random.default_rng(2)
    n, steps = 2048, 4
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 1e-6).astype(np.float32) for _ in range(steps)]
    scaled = [g * np.float32(2. ** k) for g in grads]
    grp = dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01, decoupled_weight_decay=True)
    # the bound of each step at the unscaled trajectory's state; a trajectory may be off by the sum so far, two of them by twice that
    m, v, p, budget, budgets = np.zeros_like(p0), np.zeros_like(p0), p0, np.zeros(n), []
    for t, g in enumerate(grads, 1):
        budget = budget + C.bound(p, g, m, v, t, [grp], form='torch')[0]     # AdamAtan2's operations: the larger count
        p, m, v = (x.astype(np.float32) for x in C.ref64(p, g, m, v, t, [grp]))
        budgets.append(budget)
    for name, run in (('ref64', lambda gs: run_ref64(p0, gs, [grp])), ('AdamAtan2', lambda gs: run_torch(atan2_opt(**grp), p0, gs))):
        for a_, b_, bud in zip(run(grads), run(scaled), budgets):
            assert (np.abs(a_.astype(np.float64) - b_) <= 2 * bud).all(), name
    adam = lambda ps: torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    a_, b_ = run_torch(adam, p0, grads)[-1], run_torch(adam, p0, scaled)[-1]
    off = np.abs(a_.astype(np.float64) - b_) > 2 * budgets[-1]
    print(f'  plain Adam, gradients x 2^{k}: {int(off.sum())} of {n} elements leave the budget')
    assert off.sum() > n // 2


def test_adam_atan2_optimizer_follows_the_reference_with_groups():
    """optim.AdamAtan2 (the external parameters' rule) against ref64: L2 and decoupled groups, three steps"""
    from transfusion_pytorch_amd.optim import AdamAtan2
    rng = np.random.default_rng(3)
    groups = C.three_groups()
    ps = [torch.nn.Parameter(torch.tensor(rng.standard_normal(500).astype(np.float32))) for _ in groups]
    opt = AdamAtan2([dict(params=[p], **g) for p, g in zip(ps, groups)], a=1.27, b=0.5)
    state = [(p.detach().numpy().copy(), np.zeros(500, np.float32), np.zeros(500, np.float32)) for p in ps]
    for t in (1, 2, 3):
        gs = [(rng.standard_normal(500) * 0.1).astype(np.float32) for _ in ps]
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g)
        opt.step()
        for i, (p, g, grp) in enumerate(zip(ps, gs, groups)):
            p0, m0, v0 = state[i]
            ref, bnd = C.ref64(p0, g, m0, v0, t, [grp], b=0.5), C.bound(p0, g, m0, v0, t, [grp], b=0.5, form='torch')
            got = (p.detach().numpy(), opt.state[p]['exp_avg'].numpy(), opt.state[p]['exp_avg_sq'].numpy())
            assert C.over(got, ref, bnd) == 0, (t, i)
            state[i] = tuple(x.copy() for x in got)
    assert set(opt.state[ps[0]]) == {'step', 'exp_avg', 'exp_avg_sq'} and float(opt.state[ps[0]]['step']) == 3.


# ---------------------------------------------------------------------------------------------------------------- constructors
def test_constructors_defaults_groups_and_errors():
    from torch.optim.lr_scheduler import LambdaLR
    from transfusion_pytorch_amd import FusedAdamAtan2, FusedMuonAdamAtan2
    from transfusion_pytorch_amd.optim import AdamAtan2, FusedAdam, FusedMuon, decay_groups
    model = small()
    opt = FusedAdamAtan2(model)
    assert isinstance(opt, FusedAdam) and isinstance(opt, torch.optim.Optimizer) and not isinstance(opt, FusedMuon)
    assert (opt.lr, opt.betas, opt.a, opt.b, opt.weight_decay, opt.max_grad_norm) == (1e-4, (0.9, 0.99), 1.27, 1., 0., None)
    assert set(opt.param_groups[0]) == {'params', 'lr', 'betas', 'weight_decay', 'decoupled_weight_decay'}       # no eps
    assert opt.param_groups[0]['decoupled_weight_decay'] is False
    with pytest.raises(AttributeError):
        opt.eps
    assert isinstance(opt.ext_opt, AdamAtan2) and len(opt.ext_params) > 0                                       # no user parameter stays on plain Adam
    assert {id(p) for g in opt.ext_opt.param_groups for p in g['params']} == {id(p) for p in opt.ext_params}
    assert opt.state_dict()['state'] == {}
    mu = FusedMuonAdamAtan2(model, lr=8e-4)
    assert isinstance(mu, FusedMuon) and isinstance(mu.ext_opt, AdamAtan2)
    assert (mu.lr, mu.betas, mu.a, mu.b, mu.muon_lr, mu.ns_steps) == (8e-4, (0.9, 0.99), 1.27, 1., 1e-3, 5)
    assert 'eps' not in mu.param_groups[0] and mu.param_groups[-1]['eps'] == 1e-7 == mu.muon_eps               # Muon's own eps stays
    assert mu.launches_per_step() == FusedMuon(model).launches_per_step()
    assert mu.state_dict()['state'] == {}
    for cls in (FusedAdamAtan2, FusedMuonAdamAtan2):
        grouped = cls(model, lr=1e-3, param_groups=decay_groups(model, 0.1))
        assert [g['weight_decay'] for g in grouped.param_groups[:2]] == [0.1, 0.] and all('eps' not in g for g in grouped.param_groups[:2])
        assert grouped.group_ranges() == (FusedMuon if cls is FusedMuonAdamAtan2 else FusedAdam)(model, param_groups=decay_groups(model, 0.1)).group_ranges()
        sched = LambdaLR(grouped, lambda s: 0.5 ** s)
        sched.step()
        assert grouped.lr == pytest.approx(5e-4) and grouped.ext_opt is not None
        grouped._sync_ext_opt()
        assert all(g['lr'] == pytest.approx(5e-4) and g['a'] == 1.27 for g in grouped.ext_opt.param_groups)
        some = list(model.parameters())
        for bad in (dict(eps=1e-8), dict(a=1.), dict(b=2.)):
            with pytest.raises(ValueError):
                cls(model, param_groups=[dict(params=[some[0]], **bad)])
        for bad in (dict(a=0.), dict(a=-1.), dict(b=0.)):
            with pytest.raises(ValueError):
                cls(model, **bad)
        with pytest.raises(ValueError):
            cls(model, param_groups=[dict(params=[some[i]]) for i in range(capi.ENUMS['TFX_ADAM_MAX_GROUPS'] + 1)])
        assert len(cls(model, param_groups=[dict(params=[some[i]]) for i in range(capi.ENUMS['TFX_ADAM_MAX_GROUPS'])])._adam_groups()) == 8
    opt.a = 2.                                                               # optimizer-wide, re-read at every step
    opt._sync_ext_opt()
    assert all(g['a'] == 2. for g in opt.ext_opt.param_groups)


def test_moments_load_across_the_rules_and_scalars_stay():
    """a torch.optim.Adam state dict loads into FusedAdamAtan2 (moments and step carry over, the groups keep the loading optimizer's scalars), and
    an Adam-atan2 one into FusedAdam"""
    from transfusion_pytorch_amd import FusedAdamAtan2
    from transfusion_pytorch_amd.optim import FusedAdam
    model = small()
    ref = torch.optim.Adam(model.parameters(), lr=3e-2, betas=(0.5, 0.6), eps=1e-3)
    for p in model.parameters():
        p.grad = torch.randn_like(p)
    ref.step(); ref.step()
    opt = FusedAdamAtan2(model, lr=2e-4)
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count == 2 and opt.lr == 2e-4 and opt.betas == (0.9, 0.99) and 'eps' not in opt.param_groups[0]
    sd = opt.state_dict()
    owned = set(opt._flat_offsets()) | {id(p) for p in opt.ext_params}
    assert len(owned) > 60 and any(id(p) in owned for p in opt.ext_params)
    for i, p in enumerate(model.parameters()):
        if id(p) not in owned:                                               # listed, never stepped, no state
            assert i not in sd['state']
            continue
        assert torch.equal(sd['state'][i]['exp_avg'], ref.state[p]['exp_avg']) and torch.equal(sd['state'][i]['exp_avg_sq'], ref.state[p]['exp_avg_sq'])
        assert set(sd['state'][i]) >= {'step', 'exp_avg', 'exp_avg_sq'}
    back = FusedAdam(model, lr=7e-4)
    back.load_state_dict(sd)
    assert back.step_count == 2 and back.lr == 7e-4 and back.eps == 1e-8
    assert torch.equal(back.m, opt.m) and torch.equal(back.v, opt.v)
    again = FusedAdamAtan2(model, lr=9e-4)                                    # its own rule's checkpoint brings the scalars, as torch's do
    again.load_state_dict(sd)
    assert again.lr == 2e-4
