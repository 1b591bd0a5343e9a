"""LASER attention (Transformer(attn_laser=True), reference T:979-983, T:1019-1022): what can be checked without a GPU - the constructor,
the C ABI the ctypes layer reads from include/tfx.h, and the committed fixtures (tools/make_golden_laser.py)."""
import os

import pytest
import torch

from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.transfusion import Transformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
LASER_GOLDENS = ['laser_small2', 'laser_head8', 'laser_text1', 'laser_sampling']


def test_constructor_accepts_laser_and_its_softclamp_value():
    t = Transformer(dim=128, depth=2, dim_head=64, heads=2, attn_laser=True)
    assert t.attn_laser and t.laser_softclamp_value == 15.
    t = Transformer(dim=128, depth=2, dim_head=64, heads=2, attn_laser=True, attn_kwargs=dict(laser_softclamp_value=7.5))
    assert t.laser_softclamp_value == 7.5
    m = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2, attn_laser=True))
    assert m.md.laser == 15.
    assert Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2)).md.laser == 0.
    # the option adds no parameters: a laser model loads a plain model's state_dict strictly
    plain = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=2, dim_head=32, heads=2))
    m.load_state_dict(plain.state_dict(), strict=True)


def test_constructor_still_refuses_other_attention_options():
    with pytest.raises(NotImplementedError):
        Transformer(dim=128, depth=2, attn_laser=True, attn_kwargs=dict(laser_softclamp_value=15., dropout=0.1))
    with pytest.raises(NotImplementedError):
        Transformer(dim=128, depth=2, attn_kwargs=dict(softcap_value=30.))
    with pytest.raises(NotImplementedError):
        Transformer(dim=128, depth=2, use_value_residual=True)
    with pytest.raises(ValueError):
        Transformer(dim=128, depth=2, attn_laser=True, attn_kwargs=dict(laser_softclamp_value=0.))


def test_abi_has_the_laser_field_and_the_value_transform_entry_points():
    fields = [f for f, _ in capi.STRUCT_FIELDS['tfx_attn_args']]
    assert fields[-1] == 'laser', 'the laser field is appended at the END of tfx_attn_args'
    assert [f for f, _ in capi.STRUCT_FIELDS['tfx_laser_v_args']] == ['T', 'H', 'v', 'ld_v', 'vl', 'ld_vl', 'rowmap', 'c', 'dvl', 'ld_dvl', 'dv', 'ld_dv']
    for fn in ('tfx_laser_v_fwd', 'tfx_laser_v_bwd'):
        assert fn in capi.FUNCTIONS
        assert hasattr(capi.lib(), fn)
    assert capi.ENUMS['TFX_OP_LASER_V_FWD'] == 24 and capi.ENUMS['TFX_OP_LASER_V_BWD'] == 25
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'laser' in v


@pytest.mark.parametrize('name', LASER_GOLDENS)
def test_laser_golden_differs_from_the_plain_loss(name):
    g = torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    assert abs(float(g['loss']) - float(g['plain_loss'])) > 1e-3, 'the fixture was not made with attn_laser=True'
    assert 0. < g['bf16_logits_rel'] < 5e-2
    assert os.path.getsize(os.path.join(GOLDEN, f'{name}.pt')) < 1 << 20


def test_laser_goldens_regenerate_bit_for_bit():
    from oracle.ref_runner import reference_available
    if not reference_available():
        pytest.skip('the reference is not present on this machine')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_laser', os.path.join(ROOT, 'tools', 'make_golden_laser.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in LASER_GOLDENS:
        new, old = mod.make(name), torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
        assert set(new) == set(old), name
        for k in ('loss', 'logits', 'plain_loss'):
            if k in old:
                assert torch.equal(torch.as_tensor(new[k]), torch.as_tensor(old[k])), (name, k)
        for k, v in old.get('grad_head', {}).items():
            assert torch.equal(new['grad_head'][k], v), (name, k)
        for run, samples in old.get('runs', {}).items():            # sampling: every part of every sample, and the recorded margins
            assert new['margins'][run] == old['margins'][run], (name, run)
            for a, b in zip(new['runs'][run], samples):
                assert len(a) == len(b), (name, run)
                for pa, pb in zip(a, b):
                    assert pa[0] == pb[0] and torch.equal(pa[-1], pb[-1]), (name, run)
