"""Host side of frozen parameters (`p.requires_grad_(False)` on native parameters; no GPU): `frozen_ranges()` against a brute-force walk of the
segment table, its merge with Muon's ranges into the Adam skip table, the C ABI (no struct grew; the version token), parameter groups with frozen
members, and that freezing changes neither `muon_parameters()` nor the `.grad` bookkeeping of the parameter store."""
import pytest
import torch

import _frozen_cases as F
from oracle.cases import CASES
from oracle.transfusion_oracle import OracleConfig
from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.optim import FusedAdam, FusedAdamAtan2, FusedMuon, FusedMuonAdamAtan2, decay_groups

NAMES = ('small2', 'head8')


def native(name):
    cfg = OracleConfig(**CASES[name][0])
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    return Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)


def test_every_set_freezes_something_and_the_sets_differ():
    model = native('small2')
    names = list(model.store.params)
    seen = set()
    for s in F.SETS:
        tr = tuple(F.trainable_names(names, model.md.depth, s))
        assert len(tr) < len(names) and tr not in seen, s
        assert (len(tr) == 0) == (s == 'all_frozen')
        seen.add(tr)
    assert F.trainable_names(names, 4, 'modality1') == ['latent_to_model_projs.1.weight', 'latent_to_model_projs.1.bias', 'model_to_latent_projs.1.weight']
    top = F.trainable_names(names, 4, 'top_half')
    assert 'transformer.layers.2.1.to_film.weight' in top and 'transformer.layers.1.2.fn.net.0.weight' not in top and 'text_embed.weight' not in top


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('set_name', list(F.SETS))
def test_frozen_ranges_equal_a_brute_force_walk(name, set_name):
    model = native(name)
    ps = model.store
    assert ps.frozen_ranges() == [] and ps.frozen_names() == frozenset()
    frozen, train = F.freeze(model, set_name)
    assert ps.frozen_names() == frozenset(frozen)
    got = FusedAdam(model).frozen_ranges()
    assert got == F.brute_force_ranges(ps, frozen)
    assert all(a % 4 == 0 and b % 4 == 0 and a < b for a, b in got) and all(b0 < a1 for (_, b0), (a1, _) in zip(got, got[1:]))
    if set_name == 'all_frozen':
        assert got == [(0, ps.numel)]
    F.unfreeze(model)
    assert ps.frozen_ranges() == [] and FusedAdam(model).skip_table() == []


@pytest.mark.parametrize('cls', [FusedMuon, FusedMuonAdamAtan2])
@pytest.mark.parametrize('set_name', list(F.SETS))
def test_skip_table_is_the_merge_of_muons_ranges_and_the_frozen_ones(cls, set_name):
    model = native('small2')
    ps = model.store
    opt = cls(model)
    muon_only = opt.skip_table()
    assert muon_only == opt.adam_skip_table()                          # nothing frozen: the table FusedMuon always built
    all_segments = opt.muon_segments()
    frozen, _ = F.freeze(model, set_name)
    tab = opt.skip_table()
    assert all(a % 4 == 0 and b % 4 == 0 and a < b for a, b in tab) and all(b0 < a1 for (_, b0), (a1, _) in zip(tab, tab[1:]))   # sorted, disjoint, not touching
    mask = torch.zeros(ps.numel, dtype=torch.bool)
    for a, b in tab:
        mask[a:b] = True
    want = torch.zeros(ps.numel, dtype=torch.bool)
    for a, b in muon_only + F.brute_force_ranges(ps, frozen):
        want[a:b] = True
    assert torch.equal(mask, want)
    # a frozen matrix leaves the Muon tables; the full list and the reference's muon_parameters() do not change
    assert opt.muon_segments() == all_segments
    frozen_off = {ps.offsets[n][0] for n in frozen}
    assert [m['off'] for m in opt.host_tables()['mats']] == [o for o, _, _ in all_segments if o not in frozen_off]


@pytest.mark.parametrize('name', NAMES)
def test_muon_parameters_do_not_change_with_freezing(name):
    model = native(name)
    before = [id(p) for p in model.muon_parameters()]
    for s in F.SETS:
        F.freeze(model, s)
        assert [id(p) for p in model.muon_parameters()] == before, s


def test_abi_no_struct_grew_and_the_version_token_is_last():
    count = {k: len(capi.STRUCT_FIELDS[k]) for k in ('tfx_adaln_pre_args', 'tfx_adaln_post_args', 'tfx_rmsnorm_args', 'tfx_attnres_args', 'tfx_attnres_src',
                                                     'tfx_attnres_pull_args', 'tfx_adam_args')}
    assert count == {'tfx_adaln_pre_args': 18, 'tfx_adaln_post_args': 17, 'tfx_rmsnorm_args': 8, 'tfx_attnres_args': 17, 'tfx_attnres_src': 11,
                     'tfx_attnres_pull_args': 15, 'tfx_adam_args': 16}
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and v.endswith(b'-frozen') and v.index(b'ablate') < v.index(b'frozen')


def test_parameter_groups_may_hold_frozen_parameters():
    model = native('small2')
    frozen, train = F.freeze(model, 'bias_gain')
    for cls in (FusedAdam, FusedAdamAtan2, FusedMuon, FusedMuonAdamAtan2):
        opt = cls(model, param_groups=decay_groups(model, 0.1))
        listed = [p for g in opt.param_groups for p in g['params']]
        assert len(listed) == len(list(model.parameters())) and len({id(p) for p in listed}) == len(listed)
        assert opt.state_dict()['state'] == {}
    # a group of frozen parameters only is legal, and so are names
    opt = FusedAdam(model, param_groups=[dict(params=[]), dict(params=frozen[:3], lr=1e-2)])
    assert [len(g['params']) for g in opt.param_groups] == [len(list(model.parameters())) - 3, 3]
    a = opt.group_ranges()
    F.unfreeze(model)
    assert opt.group_ranges() == a                                     # the group table does not depend on what is frozen: the skip table does


def test_store_attaches_no_grad_view_to_frozen_parameters():
    model = native('head8')
    ps = model.store
    ps.grad = torch.zeros(ps.numel)                                    # (the host bookkeeping of `ensure_grad_views`; on the GPU `.cuda()` creates the buffer)
    ps.ensure_grad_views()
    assert all(p.grad is not None for p in ps.params.values())
    ps.grad.fill_(1.)                                                  # "a backward wrote everywhere"
    frozen, train = F.freeze(model, 'v_only')
    ps.ensure_grad_views(ps.frozen_names())
    for n, p in ps.params.items():
        assert (p.grad is None) == (n in frozen), n
        assert bool((ps.grad_view(n) == 0).all()) == (n in frozen), n   # a frozen segment is cleared, an accumulating one is kept
    for p in ps.params.values():
        p.grad = None
    ps.ensure_grad_views(ps.frozen_names())
    assert not ps.grad.any() and all((p.grad is None) == (n in frozen) for n, p in ps.params.items())
