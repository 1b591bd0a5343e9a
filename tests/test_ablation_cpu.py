"""The two attention ablations - Transformer(qk_rmsnorm=False) (reference T:948-952) and Transformer(attn_kwargs=dict(gate_values=False)) (T:901-904,
T:1026-1027): what can be checked without a GPU - the constructor, the parameter layout, the state_dict against the reference's, the library's
version token and the committed fixtures (tools/make_golden_ablation.py)."""
import os

import pytest
import torch

from _ablation_cases import BOTH, FIXTURES, LASER_FIXTURES, NOGATE, NOQK, TRAIN_FIXTURES, has_gates, strip_state, transformer_kwargs
from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.params import head_phys_to_ref_rows
from transfusion_pytorch_amd.transfusion import Transformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _golden(name):
    return torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)


def _native(cfg, **switches):
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    return Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, transformer=transformer_kwargs(cfg, **switches), prob_uncond=0.)


def test_constructor_accepts_qk_rmsnorm():
    assert Transformer(dim=128, depth=2).qk_rmsnorm is True and Transformer(dim=128, depth=2, qk_rmsnorm=False).qk_rmsnorm is False
    mk = lambda **sw: Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2, **sw))
    on, off, both = mk(), mk(**NOQK), mk(**BOTH)
    assert on.md.qk_norm is True and off.md.qk_norm is False and both.md.qk_norm is False and both.md.gates is False and off.md.gates is True
    # the reference keeps its q_norm / k_norm modules (T:893-894): the same parameters, the same sizes
    assert sorted(on.state_dict()) == sorted(off.state_dict()) and (off.md.nq, off.md.nqk, off.md.ldq) == (on.md.nq, on.md.nqk, on.md.ldq)
    off.load_state_dict(on.state_dict(), strict=True)


def test_constructor_accepts_gate_values():
    assert Transformer(dim=128, depth=2).gate_values is True
    assert Transformer(dim=128, depth=2, attn_kwargs=dict(gate_values=True)).gate_values is True
    t = Transformer(dim=128, depth=2, dim_head=64, heads=2, attn_laser=True, attn_kwargs=dict(gate_values=False, laser_softclamp_value=7.5))
    assert t.gate_values is False and t.attn_laser and t.laser_softclamp_value == 7.5
    m = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2, attn_kwargs=dict(gate_values=False)))
    assert m.md.gates is False
    assert Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2)).md.gates is True
    with pytest.raises(ValueError):
        Transformer(dim=128, depth=2, attn_kwargs=dict(gate_values=0))


def test_constructor_still_refuses_the_rest():
    for kw in (dict(attn_kwargs=dict(gate_values=False, dropout=0.1)), dict(attn_kwargs=dict(gate_values=False, softcap_value=30.)),
               dict(attn_kwargs=dict(gate_values=True, learned_value_residual_mix=True)), dict(unet_skips=False), dict(dropout=0.1),
               dict(use_value_residual=True), dict(ff_kwargs=dict(dropout=0.1)), dict(qk_rmsnorm=False, unet_skips=False), dict(dim_head=128)):
        with pytest.raises(NotImplementedError):
            Transformer(dim=128, depth=2, **kw)


@pytest.mark.parametrize('heads,dim_head', [(2, 64), (8, 64), (4, 8), (3, 32)])
def test_projection_sizes_for_both_gate_settings(heads, dim_head):
    mk = lambda **sw: Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=dim_head, heads=heads, **sw)).md
    on, off = mk(), mk(**NOGATE)
    assert on.nq == 3 * heads * dim_head + heads and off.nq == 3 * heads * dim_head
    assert on.nqk == 3 * heads * 64 + heads and off.nqk == 3 * heads * 64
    assert on.ldq == (on.nqk + 63) // 64 * 64 and off.ldq == 3 * heads * 64          # no padding columns behind d q | d k | d v without gates
    rows_on, rows_off = head_phys_to_ref_rows(heads, dim_head), head_phys_to_ref_rows(heads, dim_head, gates=False)
    assert len(rows_on) == on.nqk and len(rows_off) == off.nqk
    assert (rows_on[:off.nqk] == rows_off).all() and rows_off.max() == off.nq - 1 and rows_on.max() == on.nq - 1


@pytest.mark.parametrize('name', FIXTURES)
def test_state_dict_keys_equal_the_references(name):
    """without value gating the reference has no `to_gates` module: the key sets match, and a reference-shaped state_dict loads strictly"""
    g = _golden(name)
    if g['base_case'] == 'sampling':
        from oracle.make_golden_sampling import sampling_case
        cfg, sd = sampling_case(False)[:2]
    elif g['base_case'] == 'text1':
        from oracle.cases import build_text_case
        cfg, sd = build_text_case('text1')[:2]
    else:
        from oracle.cases import build_case
        cfg, sd = build_case(g['base_case'])[:2]
    sw = FIXTURES[name]
    assert g['switches'] == sw
    m = _native(cfg, **sw)
    assert sorted(m.state_dict()) == g['state_keys']
    assert any('.to_gates.' in k for k in g['state_keys']) == has_gates(sw) and any('.q_norm.gamma' in k for k in g['state_keys'])
    m.load_state_dict(strip_state(sd, sw), strict=True)
    for k, v in strip_state(sd, sw).items():
        assert torch.equal(m.state_dict()[k], v), k
    if not has_gates(sw):
        with pytest.raises(RuntimeError):
            m.load_state_dict(sd, strict=True)                   # the gated model's state_dict carries keys this model does not have
        plain = _native(cfg)
        assert sorted(set(plain.state_dict()) - set(m.state_dict())) == [f'transformer.layers.{i}.1.fn.to_gates.0.weight' for i in range(cfg.depth)]


def test_the_reference_leaves_only_the_unread_gammas_without_a_gradient():
    """training steps: without QK-RMSNorm q_norm / k_norm are never called (T:950), their gammas get no gradient; everything else does"""
    for name, sw in {**TRAIN_FIXTURES, **LASER_FIXTURES}.items():
        g = _golden(name)
        depth = 1 + max(int(k.split('.')[2]) for k in g['state_keys'] if k.startswith('transformer.layers.'))
        want = [] if sw.get('qk_rmsnorm', True) else sorted(f'transformer.layers.{i}.1.fn.{n}_norm.gamma' for i in range(depth) for n in 'qk')
        assert g['grad_none'] == want, name


def test_muon_parameters_do_not_depend_on_the_switch():
    names = {}
    for key, sw in (('on', {}), ('off', NOGATE), ('noqk', NOQK), ('both', BOTH)):
        m = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=3, dim_head=32, heads=2, **sw))
        by_id = {id(p): k for k, p in m.named_parameters()}
        names[key] = [by_id[id(p)] for p in m.muon_parameters()]
        for p, k in zip(m.muon_parameters(), names[key]):
            assert p.data_ptr() == m.store.view(k).data_ptr()     # views into the flat buffer, as before
    assert names['on'] == names['off'] == names['noqk'] == names['both'] and len(names['on']) == 12


def test_clones_carry_the_switch():
    import copy
    m = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2, **BOTH))
    for c in (m._clone_architecture(), copy.deepcopy(m)):
        assert c.md.gates is False and c.md.qk_norm is False and sorted(c.state_dict()) == sorted(m.state_dict())


def test_version_token():
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'ablate' in v


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_was_made_with_the_switch(name):
    g = _golden(name)
    assert g['switches'] == FIXTURES[name]
    assert abs(float(g['loss']) - float(g['plain_loss'])) > 1e-3, 'the fixture was not made with its switches'
    assert 0. < g['bf16_logits_rel'] < 5e-2
    assert os.path.getsize(os.path.join(GOLDEN, f'{name}.pt')) < 1 << 20


def test_greedy_fixtures_are_decisive():
    """tools/make_golden_ablation.py asserts it while writing: at least three quarters of the greedy steps have a top-2 margin above NEAR_TIE"""
    g = _golden('ablate_both_text1')
    assert float((g['gen_margin'] > 0.05).float().mean()) >= 0.75
    for run, per_sample in _golden('ablate_both_sampling')['margins'].items():
        ms = [v for mg in per_sample for _, _, v in mg]
        assert sum(v > 0.05 for v in ms) >= 0.75 * len(ms), run


def test_fixtures_regenerate_bit_for_bit():
    from oracle.ref_runner import reference_available
    if not reference_available():
        pytest.skip('the reference is not present on this machine')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_ablation', os.path.join(ROOT, 'tools', 'make_golden_ablation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in FIXTURES:
        new, old = mod.make(name), _golden(name)
        assert set(new) == set(old), name
        for k in ('loss', 'logits', 'plain_loss', 'kv_head', 'gen_tokens', 'gen_margin'):
            if k in old:
                assert torch.equal(torch.as_tensor(new[k]), torch.as_tensor(old[k])), (name, k)
        assert new['state_keys'] == old['state_keys'] and new.get('grad_none') == old.get('grad_none')
        for k, v in old.get('grad_head', {}).items():
            assert torch.equal(new['grad_head'][k], v), (name, k)
        for run, samples in old.get('runs', {}).items():            # sampling: every part of every sample, and the recorded margins
            assert new['margins'][run] == old['margins'][run], (name, run)
            for a, b in zip(new['runs'][run], samples):
                assert len(a) == len(b), (name, run)
                for pa, pb in zip(a, b):
                    assert pa[0] == pb[0] and torch.equal(pa[-1], pb[-1]), (name, run)
