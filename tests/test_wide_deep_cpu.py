"""The wide / deep model cases (tests/_wide_deep_cases.py) without a GPU: the oracle runs on each, every parameter's oracle gradient is above the floor
under which the GPU comparison (tests/test_push_form_gpu.py) would skip it, and the host code gives each case the plan form its table claims -
engine.pull_form_ok, Plan._side_stream, engine.skip_sources.  pull_form_ok is the ONE definition of the pull limits: the checks that refuse
hidden taps on a push-form model call it."""
import inspect
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _wide_deep_cases as WD                                      # noqa: E402


@pytest.mark.parametrize('name', list(WD.CASES))
def test_oracle_runs_and_every_gradient_is_above_the_comparison_floor(name):
    ref = WD.oracle_step(name)
    cfg = WD.config(name)
    assert math.isfinite(ref.loss) and ref.loss > 0
    assert ref.logits.shape[0] == 3 and ref.logits.shape[-1] == cfg.vocab
    assert set(ref.grads) == set(ref.trainable), 'a trainable parameter without an oracle gradient'
    norms = {k: float(g.double().norm()) for k, g in ref.grads.items()}
    low = {k: v for k, v in norms.items() if not v >= WD.NORM_FLOOR}
    k_min = min(norms, key=norms.get)
    print(f'  [{name}] oracle loss {ref.loss:.6f}; {len(norms)} gradients, smallest norm {norms[k_min]:.3e} ({k_min})')
    assert not low, f'the GPU comparison would skip {sorted(low)}'


@pytest.mark.parametrize('name', list(WD.CASES))
def test_plan_form_of_every_case(name, monkeypatch):
    from transfusion_pytorch_amd import engine
    monkeypatch.delenv('TFX_SIDE_STREAM', raising=False)
    c, md = WD.CASES[name], WD.dims(name)
    assert (md.dim, md.depth) == (c.dim, c.depth)
    assert engine.pull_form_ok(md) is c.pull
    assert engine.Plan._side_stream(md) is c.side
    src = engine.skip_sources(md)
    assert src == c.skips and len(src) == WD.N_SKIP[name]
    assert [i for i in range(md.depth) if md.has_skip(i)] == sorted(src)
    pushed = set(src.values())
    assert (0 in pushed) == (md.depth >= 2)                          # x_0's U-Net share: the `dskip[0]` term of the push form's dx0
    g2 = [i for i in range(md.depth) if (i + 1) in pushed]           # layers whose push sweep takes a skip share as `g2`
    assert len(g2) == len(src) - 1
    if name == 'd33':
        assert len(g2) == 15
    if name == 'w1088x3':
        assert not md.has_skip(1) and 1 not in pushed                # the middle layer of an odd depth


def test_the_limits_are_defined_once():
    from transfusion_pytorch_amd import engine
    from transfusion_pytorch_amd.params import ModelDims
    assert (engine.PULL_MAX_DEPTH, engine.PULL_MAX_DIM) == (32, 1024)
    md = lambda dim, depth: ModelDims(num_text_tokens=96, dim=dim, depth=depth, heads=1, dim_head=64, dim_latents=(16,))
    for dim, depth, ok in [(1024, 32, True), (1088, 32, False), (1024, 33, False), (64, 1, True), (1088, 33, False)]:
        assert engine.pull_form_ok(md(dim, depth)) is ok
    assert 'depth <= 32' in engine.PULL_LIMITS and 'dim <= 1024' in engine.PULL_LIMITS


def _model(dim=64, depth=2):
    from transfusion_pytorch_amd import Transfusion
    return Transfusion(num_text_tokens=32, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=dim, depth=depth))


def test_the_refusals_of_the_push_form_ask_pull_form_ok(monkeypatch):
    """what tests/test_push_form_gpu.py patches to force the push form on a pull-eligible model is what decides every refusal"""
    from transfusion_pytorch_amd import SelfMaskedRepTraining, engine, self_flow, transfusion
    assert self_flow.engine is engine and transfusion._engine is engine
    with pytest.raises(NotImplementedError, match='depth <= 32'):
        SelfMaskedRepTraining(_model(depth=33), use_asymmetric_dropout=False)
    SelfMaskedRepTraining(_model(depth=2), use_asymmetric_dropout=False)
    with monkeypatch.context() as m:
        m.setattr(engine, 'pull_form_ok', lambda md: False)
        with pytest.raises(NotImplementedError, match='pull-form'):
            SelfMaskedRepTraining(_model(depth=2), use_asymmetric_dropout=False)
    with monkeypatch.context() as m:
        m.setattr(engine, 'pull_form_ok', lambda md: True)
        SelfMaskedRepTraining(_model(depth=33), use_asymmetric_dropout=False)
    # the hidden-tap check of Transfusion's training forward needs a plan (a GPU: tests/test_push_form_gpu.py runs it); here: it reads the same function,
    # looked up in the engine module at call time, and Plan.__init__ does too
    fwd = inspect.getsource(transfusion.Transfusion)
    assert '_engine.pull_form_ok(self.md)' in fwd and 'NotImplementedError' in fwd
    assert 'pull_form_ok(md)' in inspect.getsource(engine.Plan.__init__)
    for mod in (engine, transfusion, self_flow):
        assert 'TFX_ATTNRES_PULL' not in inspect.getsource(mod)          # (a switch nothing reads: DESIGN.md lists it among the removed ones)
