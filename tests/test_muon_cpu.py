"""Host side of Muon (no GPU): Transfusion.muon_parameters() against the reference's names, the C ABI of csrc/muon.hip, the host logic of the
problem tables (orientation, padding, tile counts, launches per step) and the Adam skip table of optim.FusedMuon."""
import ctypes
import json
import os

import pytest
import torch

from oracle.cases import CASES
from oracle.transfusion_oracle import OracleConfig
from transfusion_pytorch_amd import Transfusion, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'muon_names.json')
NAMES = ('small2', 'head8', 'canon512')


def native(name):
    cfg = OracleConfig(**CASES[name][0])
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    return Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)


@pytest.mark.parametrize('name', NAMES)
def test_muon_parameters_are_the_references_in_its_order(name):
    want = json.load(open(GOLDEN))[name]
    model = native(name)
    named = dict(model.named_parameters())
    by_id = {id(p): n for n, p in named.items()}
    got = model.muon_parameters()
    assert [by_id[id(p)] for p in got] == want                      # the very objects named_parameters() yields, under the reference's names
    assert len(want) == 4 * OracleConfig(**CASES[name][0]).depth
    base = model.store.flat.data_ptr()
    for p, n in zip(got, want):
        assert p is named[n] and p.ndim == 2
        assert p.data_ptr() == base + 4 * model.store.offsets[n][0], 'a view into the flat buffer'


def test_muon_names_fixture_regenerates_identically():
    from oracle.ref_runner import reference_available
    if not reference_available():
        pytest.skip('the reference is not present on this machine')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_muon', os.path.join(ROOT, 'tools', 'make_golden_muon.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make_all() == json.load(open(GOLDEN))
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_abi_has_the_muon_entry_points_and_adam_grew_at_its_end():
    fields = [f for f, _ in capi.STRUCT_FIELDS['tfx_adam_args']]
    assert fields == ['p', 'g', 'm', 'v', 'n', 'lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'max_norm', 'grad_scale', 'step', 'sumsq', 'skip', 'nskip']
    for s in ('tfx_muon_mat', 'tfx_muon_prep_args', 'tfx_muon_gemm_problem', 'tfx_muon_apply_args'):
        assert s in capi.STRUCT_FIELDS
    for fn in ('tfx_muon_plan', 'tfx_muon_step_launches', 'tfx_muon_prep', 'tfx_muon_norm', 'tfx_muon_gemm', 'tfx_muon_apply', 'tfx_sumsq_det'):
        assert fn in capi.FUNCTIONS and hasattr(capi.lib(), fn)
    assert capi.ENUMS['TFX_OP_ADAM_STEP'] == 22 and capi.ENUMS['TFX_OP_LASER_V_BWD'] == 25
    v = capi.lib().tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'laser' in v and b'muon' in v


@pytest.mark.parametrize('rows,cols,want', [
    # flip, m, n, m_pad, n_pad, gram tiles (m_pad / 128)^2, update tiles (n_pad / 128)(m_pad / 128), 64 x 64 prep blocks
    (512, 512, (0, 512, 512, 512, 512, 16, 16, 64)),
    (2730, 512, (1, 512, 2730, 512, 2816, 16, 88, 43 * 8)),
    (512, 1365, (0, 512, 1365, 512, 1408, 16, 44, 8 * 22)),
    (32, 128, (0, 32, 128, 128, 128, 1, 1, 2)),
    (128, 32, (1, 32, 128, 128, 128, 1, 1, 2)),
])
def test_problem_plan_orientation_padding_and_tiles(rows, cols, want):
    from transfusion_pytorch_amd.optim import FusedMuon
    pl = FusedMuon.plan(rows, cols)
    assert tuple(pl[k] for k in ('flip', 'm', 'n', 'm_pad', 'n_pad', 'gram_tiles', 'update_tiles', 'prep_blocks')) == want
    assert pl['m'] <= pl['n'] and pl['m_pad'] % 128 == 0 and pl['n_pad'] % 128 == 0
    assert capi.lib().tfx_muon_plan(0, 4, *[None] * 8) != 0
    out = ctypes.c_int32()                                           # any output may be NULL
    assert capi.lib().tfx_muon_plan(rows, cols, None, None, None, None, ctypes.byref(out), None, None, None) == 0 and out.value == want[4]


@pytest.mark.parametrize('fn', [None, 'original', 'match_rms_adamw'])
@pytest.mark.parametrize('rows,cols', [(512, 512), (2730, 512), (512, 1365), (32, 128), (128, 32)])
def test_lr_ratio_is_torchs_adjust_lr(fn, rows, cols):
    """the per-matrix learning-rate factor against torch/optim/_muon.py `_adjust_lr`, and the same figure in the descriptor table the kernels read"""
    from torch.optim._muon import _adjust_lr
    from transfusion_pytorch_amd.optim import FusedMuon, _muon_host_tables
    want = _adjust_lr(1., fn, torch.Size((rows, cols)))
    assert FusedMuon._lr_ratio(fn, rows, cols) == pytest.approx(want, rel=1e-12)
    assert _muon_host_tables([(0, rows, cols)], fn)['mats'][0]['lr_ratio'] == pytest.approx(want, rel=1e-12)
    if fn != 'match_rms_adamw':
        assert want == pytest.approx(max(1., rows / cols) ** 0.5)            # 2730 x 512 -> 2.31, never below 1
    else:
        assert want == pytest.approx(0.2 * max(rows, cols) ** 0.5)


def test_model_tables_carry_torchs_lr_ratio():
    from torch.optim._muon import _adjust_lr
    from transfusion_pytorch_amd.optim import FusedMuon
    for fn in (None, 'original', 'match_rms_adamw'):
        opt = FusedMuon(native('head8'), adjust_lr_fn=fn)
        for m in opt.host_tables()['mats']:
            assert m['lr_ratio'] == pytest.approx(_adjust_lr(1., fn, torch.Size((m['rows'], m['cols']))), rel=1e-12)


def test_launches_per_step_do_not_depend_on_depth():
    """host side only: the reported count and the structure of the tables (one grid per product kind over all matrices).  The calls a step really
    makes are counted at the library boundary in tests/test_muon_gpu.py::test_entry_point_calls_of_a_step_do_not_depend_on_depth"""
    from transfusion_pytorch_amd.optim import FusedMuon
    mk = lambda depth: Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=64, depth=depth, dim_head=64, heads=1))
    shallow, deep = FusedMuon(mk(2)), FusedMuon(mk(24))
    assert len(shallow.muon_params) == 8 and len(deep.muon_params) == 96
    assert shallow.launches_per_step() == deep.launches_per_step() == 2 + 1 + 1 + 3 * 5 + 1 + 1
    deep.ns_steps = 3
    assert deep.launches_per_step() == 2 + 1 + 1 + 3 * 3 + 1 + 1
    # one grid per product kind: the tiles of all matrices, each tile pointing at its problem, every problem's tiles contiguous from its tile0
    H = deep.host_tables()
    assert len(H['mats']) == 96
    for key, tile0, count in (('sq_prob', 'sq_tile0', 'gram_tiles'), ('up_prob', 'up_tile0', 'update_tiles')):
        assert len(H[key]) == sum(m[count] for m in H['mats'])
        for i, m in enumerate(H['mats']):
            assert H[key][m[tile0]:m[tile0] + m[count]] == [i] * m[count]


@pytest.mark.parametrize('name', ['head8', 'small2'])
def test_skip_table_covers_exactly_the_muon_segments(name):
    from transfusion_pytorch_amd.optim import FusedMuon
    model = native(name)
    ps = model.store
    opt = FusedMuon(model)
    ranges = opt.skip_ranges()
    assert ranges == sorted(ranges) and all(a < b for a, b in ranges) and all(r0[1] < r1[0] for r0, r1 in zip(ranges, ranges[1:]))
    got = torch.zeros(ps.numel, dtype=torch.bool)
    for a, b in ranges:
        got[a:b] = True
    want = torch.zeros(ps.numel, dtype=torch.bool)
    muon = {id(p) for p in model.muon_parameters()}
    for n, p in ps.params.items():
        if id(p) in muon:
            o, shape = ps.offsets[n]
            want[o:o + int(torch.Size(shape).numel())] = True
    assert torch.equal(got, want)
    assert 0 < int(want.sum()) < ps.numel
    assert opt.adam_skip_table() == ranges and all(a % 4 == 0 and b % 4 == 0 for a, b in ranges)      # what the Adam kernel gets: whole groups of 4
    # workspace: every matrix has its own, non-overlapping, tile-padded X / X^T / A / B regions
    H = opt.host_tables()
    x_regions = sorted((m[k], m[k] + m['m_pad'] * m['n_pad']) for m in H['mats'] for k in ('x_off', 'xt_off'))
    ab_regions = sorted((m[k], m[k] + m['m_pad'] ** 2) for m in H['mats'] for k in ('a_off', 'b_off'))
    for regions, total in ((x_regions, H['x_elems']), (ab_regions, H['ab_elems'])):
        assert regions[0][0] == 0 and regions[-1][1] == total and all(r0[1] == r1[0] for r0, r1 in zip(regions, regions[1:]))


def test_explicit_muon_params_and_bad_ones():
    from transfusion_pytorch_amd.optim import FusedMuon
    model = native('head8')
    two = model.muon_parameters()[:2]
    opt = FusedMuon(model, muon_params=two, muon_lr=2e-3)
    assert len(opt.skip_ranges()) == 2 and opt.muon_lr == 2e-3
    with pytest.raises(ValueError):
        FusedMuon(model, muon_params=[model.store.params['transformer.norm.gamma']])          # not a matrix
    with pytest.raises(ValueError):
        FusedMuon(model, muon_params=[torch.nn.Parameter(torch.zeros(4, 4))]).skip_ranges()   # not in the flat buffer
    with pytest.raises(ValueError):
        FusedMuon(model, adjust_lr_fn='nope').host_tables()
