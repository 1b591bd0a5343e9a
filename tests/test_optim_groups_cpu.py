"""Host side of the optimizer surface (no GPU): FusedAdam / FusedMuon as torch.optim.Optimizer subclasses under torch's LR schedulers, the
parameter groups and their range table, the C ABI of the grouped Adam launch, and the state dict before a step."""
import ctypes

import pytest
import torch

from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.optim import FusedAdam, FusedMuon, decay_groups

ADAM_FIELDS = ['p', 'g', 'm', 'v', 'n', 'lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'max_norm', 'grad_scale', 'step', 'sumsq', 'skip', 'nskip']
NEW_FIELDS = ['decoupled', 'ranges', 'nrange', 'ngroup', 'group_lr', 'group_beta1', 'group_beta2', 'group_eps', 'group_weight_decay', 'group_decoupled']


def small():
    torch.manual_seed(0)
    return Transfusion(num_text_tokens=32, dim_latent=16, add_pos_emb=True, modality_num_dim=1, transformer=dict(dim=64, depth=2, heads=2, dim_head=8))


# ---------------------------------------------------------------------------------------------------------------- 1. optimizer type and schedulers
@pytest.mark.parametrize('cls', [FusedAdam, FusedMuon])
def test_is_a_torch_optimizer_and_schedulers_drive_every_group(cls):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR
    model = small()
    opt = cls(model, lr=1e-3, param_groups=decay_groups(model, 0.1))
    assert isinstance(opt, torch.optim.Optimizer)
    base = [g['lr'] for g in opt.param_groups]
    assert len(base) == (3 if cls is FusedMuon else 2)
    sched = LambdaLR(opt, lambda s: 0.5 ** s)
    for k in (1, 2):
        sched.step()
        assert opt.lr == pytest.approx(1e-3 * 0.5 ** k)
        assert [g['lr'] for g in opt.param_groups] == pytest.approx([b * 0.5 ** k for b in base])
    if cls is FusedMuon:
        assert opt.muon_lr == opt.param_groups[-1]['lr'] == pytest.approx(1e-3 * 0.25)      # muon_lr 1e-3 by default: the scheduler scaled it too
    opt2 = cls(model, lr=2e-3)
    cos = CosineAnnealingLR(opt2, T_max=10)
    cos.step()
    assert opt2.lr == opt2.param_groups[0]['lr'] < 2e-3
    opt2.lr = 7e-4                                                   # code that does not use groups
    assert opt2.param_groups[0]['lr'] == 7e-4
    opt2.betas, opt2.eps, opt2.weight_decay = (0.8, 0.9), 1e-6, 0.2
    assert (opt2.param_groups[0]['betas'], opt2.param_groups[0]['eps'], opt2.param_groups[0]['weight_decay']) == ((0.8, 0.9), 1e-6, 0.2)


def test_muon_attributes_alias_the_last_group_under_torchs_keys():
    model = small()
    opt = FusedMuon(model, muon_lr=2e-3, muon_weight_decay=0.05, momentum=0.9, ns_steps=3)
    ref = torch.optim.Muon(model.muon_parameters())
    last = opt.param_groups[-1]
    assert set(last) == set(ref.param_groups[0])
    assert (last['lr'], last['weight_decay'], last['momentum'], last['ns_steps'], last['eps']) == (2e-3, 0.05, 0.9, 3, 1e-7)
    assert [id(p) for p in last['params']] == [id(p) for p in model.muon_parameters()] == [id(p) for p in opt.muon_params]
    opt.muon_lr, opt.nesterov = 5e-3, False
    assert last['lr'] == 5e-3 and last['nesterov'] is False
    last['momentum'] = 0.8
    assert opt.momentum == 0.8
    muon = {id(p) for p in model.muon_parameters()}
    assert not any(id(p) in muon for g in opt.param_groups[:-1] for p in g['params'])
    assert sum(len(g['params']) for g in opt.param_groups) == len(list(model.parameters()))


def test_owns_model_parameters_in_order():
    model = small()
    opt = FusedAdam(model)
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(p) for p in model.parameters()]
    assert len(opt.ext_params) == 6 and len(opt.ext_opt.param_groups) == 1


# ---------------------------------------------------------------------------------------------------------------- 2. group ranges
@pytest.mark.parametrize('cls', [FusedAdam, FusedMuon])
def test_group_ranges_cover_the_flat_buffer(cls):
    model = small()
    ps = model.store
    opt = cls(model, param_groups=decay_groups(model, 0.1))
    ranges = opt.group_ranges()
    assert ranges == sorted(ranges) and ranges[0][0] == 0 and ranges[-1][1] == ps.numel
    assert all(a < b and a % 4 == 0 and b % 4 == 0 and 0 <= k < 2 for a, b, k in ranges)
    assert all(r0[1] == r1[0] and r0[2] != r1[2] for r0, r1 in zip(ranges, ranges[1:]))      # disjoint, no hole, neighbours differ
    assert len(ranges) > 4
    # every Adam-owned flat parameter lies in a range of its own group
    muon = {id(p) for p in model.muon_parameters()} if cls is FusedMuon else set()
    group_of = {id(p): k for k, g in enumerate(opt.param_groups) for p in g['params']}
    for n, p in ps.params.items():
        if id(p) in muon:
            continue
        off = ps.offsets[n][0]
        hit = [k for a, b, k in ranges if a <= off and off + p.numel() <= b]
        assert hit == [group_of[id(p)]], n
    # the decaying group holds the matrices, the other gains, biases, layerscale and pseudo_queries
    names = {id(p): n for n, p in model.named_parameters()}
    decay, plain = decay_groups(model, 0.1)
    assert decay['weight_decay'] == 0.1 and plain['weight_decay'] == 0. and decay['decoupled_weight_decay'] is True
    assert all(p.ndim >= 2 for p in decay['params'])
    assert all(p.ndim < 2 or names[id(p)].endswith(('layerscale', 'pseudo_queries')) for p in plain['params'])
    assert {names[id(p)] for p in plain['params']} >= {'transformer.layers.0.1.layerscale', 'transformer.layers.0.3.pseudo_queries', 'transformer.norm.gamma',
                                                        'transformer.layers.0.2.fn.net.0.bias'}
    assert len(decay['params']) + len(plain['params']) == len(list(model.parameters()))
    assert FusedAdam(model).group_ranges() == [(0, ps.numel, 0)]


def test_groups_by_name_defaults_and_errors():
    model = small()
    gamma = 'transformer.layers.0.1.layernorm_gamma'
    opt = FusedAdam(model, lr=1e-3, weight_decay=0.1, param_groups=[dict(params=[]), dict(params=[gamma], eps=1e-6, weight_decay=0.)])
    assert [len(g['params']) for g in opt.param_groups] == [len(list(model.parameters())) - 1, 1]
    assert opt.param_groups[1]['params'][0] is model.store.params[gamma]
    assert opt.param_groups[1]['eps'] == 1e-6 and opt.param_groups[1]['lr'] == 1e-3 and opt.param_groups[0]['weight_decay'] == 0.1
    off = model.store.offsets[gamma][0]
    assert (off, off + 64, 1) in opt.group_ranges()
    p = model.store.params[gamma]
    with pytest.raises(ValueError):
        FusedAdam(model, param_groups=[dict(params=[p]), dict(params=[p])])                       # named in two groups
    with pytest.raises(ValueError):
        FusedAdam(model, param_groups=[dict(params=[torch.nn.Parameter(torch.zeros(4))])])        # not the model's
    with pytest.raises(ValueError):
        FusedAdam(model, param_groups=[dict(params=['no.such.parameter'])])
    some = list(model.store.params.values())
    with pytest.raises(ValueError):
        FusedAdam(model, param_groups=[dict(params=[some[i]]) for i in range(capi.ENUMS['TFX_ADAM_MAX_GROUPS'] + 1)])
    assert len(FusedAdam(model, param_groups=[dict(params=[some[i]]) for i in range(capi.ENUMS['TFX_ADAM_MAX_GROUPS'])]).param_groups) == 8


# ---------------------------------------------------------------------------------------------------------------- 3. ABI
def test_abi_of_the_grouped_adam_launch():
    """The grouped launch has a struct of its own, tfx_adam_group_args: tfx_adam_args' fields first, in its order and layout, the new fields at the
    end.  (tfx_adam_args itself cannot grow: tests/test_muon_cpu.py pins its exact field list.)"""
    assert [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_args']] == ADAM_FIELDS
    fields = [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_group_args']]
    assert fields[:len(ADAM_FIELDS)] == ADAM_FIELDS and fields[len(ADAM_FIELDS):] == NEW_FIELDS
    old, new = capi.STRUCTS['tfx_adam_args'], capi.STRUCTS['tfx_adam_group_args']
    for f in ADAM_FIELDS:
        assert getattr(old, f).offset == getattr(new, f).offset and getattr(old, f).size == getattr(new, f).size, f
    assert capi.ENUMS['TFX_ADAM_MAX_GROUPS'] == 8
    for f in NEW_FIELDS[4:]:
        assert getattr(new, f).size == 4 * 8
    assert getattr(new, 'decoupled').offset == getattr(old, 'nskip').offset + 4
    assert 'tfx_adam_step_groups' in capi.FUNCTIONS and hasattr(capi.lib(), 'tfx_adam_step_groups')
    a = capi.make_args('tfx_adam_group_args', group_lr=[1., 2.], group_decoupled=(1, 0, 1))
    assert list(a.group_lr) == [1., 2.] + [0.] * 6 and list(a.group_decoupled) == [1, 0, 1, 0, 0, 0, 0, 0]
    assert b'adamgroups' in capi.lib().tfx_version()


def test_grouped_launch_refuses_bad_arguments_on_the_host():
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.addressof(buf) & ~15
    ok = dict(p=ptr, g=ptr, m=ptr, v=ptr, n=4, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.)
    call = lambda **kw: capi.lib().tfx_adam_step_groups(ctypes.byref(capi.make_args('tfx_adam_group_args', **{**ok, **kw})), None)
    assert call(n=0, decoupled=1) == 0                                       # nothing to do
    assert call(decoupled=1, p=ptr + 4) != 0                                 # 16-byte alignment
    assert call(nrange=1, ngroup=1) != 0                                     # a count without a table
    assert call(nrange=-1) != 0
    assert call(nrange=1, ranges=ptr, ngroup=0) != 0 and call(nrange=1, ranges=ptr, ngroup=9) != 0
    assert call(decoupled=1, nskip=2) != 0
    assert call(decoupled=1, max_norm=0.5) != 0                              # a clip without the sum of squares


# ---------------------------------------------------------------------------------------------------------------- 4. state before a step
@pytest.mark.parametrize('cls', [FusedAdam, FusedMuon])
def test_state_dict_before_a_step(cls):
    model = small()
    opt = cls(model, param_groups=decay_groups(model, 0.1))
    sd = opt.state_dict()
    assert sd['state'] == {}
    ref = torch.optim.AdamW(model.parameters())
    for g in sd['param_groups'][:2]:
        assert {'params', 'lr', 'betas', 'eps', 'weight_decay', 'decoupled_weight_decay'} <= set(g) <= set(ref.state_dict()['param_groups'][0])
    flat = [i for g in sd['param_groups'] for i in g['params']]
    assert flat == list(range(len(list(model.parameters()))))               # indices run over the groups in order, as torch packs them
    if cls is FusedMuon:
        assert set(sd['param_groups'][-1]) == set(torch.optim.Muon(model.muon_parameters()).state_dict()['param_groups'][0])
    assert cls(small()).state_dict()['state'] == {}


def test_load_state_dict_on_the_host_and_its_errors():
    """torch.optim.Adam's state over model.parameters() loads (moments copied into m / v, the step count taken, the groups' scalars taken), and goes
    back into torch; count, shape and step mismatches raise"""
    model = small()
    ref = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.8, 0.9))
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        for p in model.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g) * 0.1
        ref.step()
    sd = ref.state_dict()
    opt = FusedAdam(model)
    opt.load_state_dict(sd)
    assert opt.step_count == 2 and opt.lr == 5e-4 and tuple(opt.betas) == (0.8, 0.9)
    ps = model.store
    for n, p in ps.params.items():
        off = ps.offsets[n][0]
        assert torch.equal(opt.m[off:off + p.numel()].view(p.shape), ref.state[p]['exp_avg']), n
        assert torch.equal(opt.v[off:off + p.numel()].view(p.shape), ref.state[p]['exp_avg_sq']), n
    for p in opt.ext_params:
        assert torch.equal(opt.ext_opt.state[p]['exp_avg'], ref.state[p]['exp_avg']) and float(opt.ext_opt.state[p]['step']) == 2.
    back = opt.state_dict()
    assert set(back['state']) == set(sd['state'])
    for k, e in sd['state'].items():
        assert float(back['state'][k]['step']) == 2. and torch.equal(back['state'][k]['exp_avg_sq'], e['exp_avg_sq'])
    torch.optim.Adam(model.parameters()).load_state_dict(back)
    # errors
    import copy
    bad = copy.deepcopy(sd); bad['param_groups'].append(dict(bad['param_groups'][0]))
    with pytest.raises(ValueError):
        FusedAdam(model).load_state_dict(bad)
    bad = copy.deepcopy(sd); bad['param_groups'][0]['params'] = bad['param_groups'][0]['params'][:-1]
    with pytest.raises(ValueError):
        FusedAdam(model).load_state_dict(bad)
    flat_idx = [i for i, p in enumerate(model.parameters()) if id(p) in {id(q) for q in ps.params.values()}]
    bad = copy.deepcopy(sd); bad['state'][flat_idx[0]]['exp_avg'] = torch.zeros(3)
    with pytest.raises(ValueError):
        FusedAdam(model).load_state_dict(bad)
    bad = copy.deepcopy(sd); bad['state'][flat_idx[1]]['step'] = torch.tensor(5.)
    with pytest.raises(ValueError):
        FusedAdam(model).load_state_dict(bad)
    # a missing entry means zeros
    part = copy.deepcopy(sd); del part['state'][flat_idx[0]]
    opt = FusedAdam(model); opt.load_state_dict(part)
    p0 = list(model.parameters())[flat_idx[0]]
    off = (p0.data_ptr() - ps.flat.data_ptr()) // 4
    assert not opt.m[off:off + p0.numel()].any() and opt.m.any() and opt.step_count == 2
