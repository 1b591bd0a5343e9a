"""SelfMaskedRepTraining / hidden taps: everything that needs no GPU - the public surface, the C ABI of the fused cosine loss, the fixtures."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _self_flow_cases as SF                                      # noqa: E402
from transfusion_pytorch_amd import capi                            # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
FIXTURES = [*SF.WRAPPER_CASES, SF.TAPS_FIXTURE]


def _model(dim=64, depth=2):
    from transfusion_pytorch_amd import Transfusion
    return Transfusion(num_text_tokens=32, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=dim, depth=depth))


def test_export_and_constructor_surface():
    import transfusion_pytorch_amd as tp
    from transfusion_pytorch_amd import SelfMaskedRepTraining, default_rep_loss_fn
    assert 'SelfMaskedRepTraining' in tp.__all__ and 'default_rep_loss_fn' in tp.__all__
    sig = inspect.signature(SelfMaskedRepTraining.__init__)
    defaults = {k: v.default for k, v in sig.parameters.items() if k not in ('self', 'net')}
    assert defaults == dict(ema_beta=0.999, rep_loss_weight=0.1, student_layer=-3, teacher_layer=-1, loss_fn=default_rep_loss_fn,
                            use_asymmetric_dropout=True, student_dropout_rate=0.1, teacher_dropout_rate=0.)
    assert list(defaults) == ['ema_beta', 'rep_loss_weight', 'student_layer', 'teacher_layer', 'loss_fn', 'use_asymmetric_dropout',
                              'student_dropout_rate', 'teacher_dropout_rate']
    p, t = torch.randn(2, 5, 8), torch.randn(2, 5, 8)
    assert torch.allclose(default_rep_loss_fn(p, t), 1 - torch.nn.functional.cosine_similarity(p, t, dim=-1).mean())


def test_asymmetric_dropout_raises_and_names_the_supported_mode():
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    with pytest.raises(NotImplementedError, match='use_asymmetric_dropout=False'):
        SelfMaskedRepTraining(_model())
    with pytest.raises(AssertionError):                             # the reference's own check comes first (T:3473)
        SelfMaskedRepTraining(_model(), student_dropout_rate=0., teacher_dropout_rate=0.1)


def test_head_parameters_names_shapes_and_parameter_order():
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    dim = 128
    net = _model(dim=dim)
    w = SelfMaskedRepTraining(net, use_asymmetric_dropout=False)
    di = int(dim * 8 / 3)
    assert di == int(dim * 4 * 2 / 3)
    shapes = {k: tuple(v.shape) for k, v in w.student_predict_head.named_parameters()}
    assert shapes == {'0.gamma': (dim,), '1.net.0.weight': (2 * di, dim), '1.net.0.bias': (2 * di,), '1.net.3.weight': (dim, di), '1.net.3.bias': (dim,)}
    sd = w.state_dict()
    for k in shapes:
        assert f'student_predict_head.{k}' in sd
    assert 'zero' in sd and float(w.zero) == 0.
    assert all(p.dtype == torch.float32 for p in w.student_predict_head.parameters())
    w.student_predict_head.load_state_dict(SF.head_state(dim), strict=True)          # a reference wrapper's head entries load
    ps = list(w.parameters())
    want = list(net.parameters()) + list(w.student_predict_head.parameters())
    assert len(ps) == len(want) and all(a is b for a, b in zip(ps, want))
    assert w.student is net and w.teacher.ema_model is not net and w.has_ssl_loss
    assert [id(p) for p in w.muon_parameters()] == [id(p) for p in net.muon_parameters()]
    assert not SelfMaskedRepTraining(_model(), use_asymmetric_dropout=False, rep_loss_weight=0.).has_ssl_loss


def test_push_form_models_raise_at_construction():
    """hidden taps ride on the pull-form AttentionResidual backward (depth <= 32, dim <= 1024): elsewhere the wrapper says so before any step"""
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    with pytest.raises(NotImplementedError, match='depth <= 32'):
        SelfMaskedRepTraining(_model(dim=64, depth=33), use_asymmetric_dropout=False)
    SelfMaskedRepTraining(_model(dim=64, depth=33), use_asymmetric_dropout=False, rep_loss_weight=0.)      # no taps without the loss


def test_tensor_inputs_raise():
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    w = SelfMaskedRepTraining(_model(), use_asymmetric_dropout=False)
    with pytest.raises(NotImplementedError):
        w(torch.randint(0, 32, (2, 16)))
    with pytest.raises(NotImplementedError):
        w(torch.randn(2, 4, 16))


def test_cosine_abi():
    fields = [f for f, _ in capi.STRUCT_FIELDS['tfx_cosine_args']]
    assert fields == ['T', 'd', 'pred', 'ld_pred', 'target', 'ld_target', 'n_pad', 'n_valid', 'grad_scale', 'dpred', 'ld_d', 'acc']
    assert 'tfx_cosine_fwd_bwd' in capi.FUNCTIONS
    op = capi.ENUMS['TFX_OP_COSINE_FWD_BWD']
    assert sum(1 for k, v in capi.ENUMS.items() if k.startswith('TFX_OP_') and v == op) == 1
    lib = capi.lib()
    assert hasattr(lib, 'tfx_cosine_fwd_bwd')
    v = lib.tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'laser' in v and b'muon' in v and b'selfflow' in v
    # argument checks run on the host, before any launch
    bad = capi.make_args('tfx_cosine_args', T=4, d=48, ld_pred=48, ld_target=48, ld_d=48)
    assert lib.tfx_cosine_fwd_bwd(__import__('ctypes').byref(bad), None) != 0


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_sanity(name):
    path = os.path.join(GOLDEN, f'{name}.pt')
    assert os.path.getsize(path) < (1 << 20)
    g = torch.load(path, weights_only=False)
    if name == SF.TAPS_FIXTURE:
        assert sorted(g['taps']) == sorted(SF.tap_indices(4))
        for k, t in g['taps'].items():
            assert 0.1 <= t['share_fraction'] <= 0.5 and t['floor_mean'] > 0 and t['floor_worst'] >= t['floor_mean'] and t['w'] > 0
        return
    rep = float(g['rep_loss'])
    assert abs(rep) > 1e-3 and abs(rep - 1.) > 1e-3
    assert abs(float(g['total_loss']) - float(g['student_loss']) - g['rep_loss_weight'] * rep) < 1e-5
    assert abs(float(g['student_loss']) - float(g['plain_loss'])) < 1e-6
    assert g['share_fraction'] >= 0.05
    assert all(v > 0 for v in g['floors'].values())
    assert set(g['head_grad_norms']) == set(SF.head_state(8))


@pytest.mark.parametrize('name', FIXTURES)
def test_selfflow_goldens_regenerate_bit_for_bit(name):
    from oracle.ref_runner import reference_available
    if not reference_available():
        pytest.skip('the reference is not present')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_golden_selfflow as G
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                     # as the generator's main: the sums of a CPU GEMM depend on the thread count
    try:
        new, old = G.make(name), torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    finally:
        torch.set_num_threads(threads)

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], f'{path}.{k}')
        elif torch.is_tensor(a):
            assert torch.equal(a, b), path
        elif isinstance(a, (list, tuple)):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f'{path}[{i}]')
        else:
            assert a == b, (path, a, b)
    same(new, old, name)
