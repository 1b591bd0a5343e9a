"""examples/dpo_toy_text_latent.py runs: the DPO loss falls from log 2 (policy == reference at step 0) and the reference model's weights do not move by a bit"""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu


def test_dpo_example_loss_falls_and_the_reference_stays():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'dpo_toy_text_latent.py')
    spec = importlib.util.spec_from_file_location('dpo_toy_text_latent', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = []
    losses, moved = mod.main(steps=30, log=lines.append)
    print('\n'.join(lines))
    assert abs(losses[0] - math.log(2.)) <= 1e-3, 'the adapters start at zero: margin 0, loss log 2'
    assert all(math.isfinite(v) for v in losses) and sum(losses[-5:]) / 5 < 0.8 * losses[0], (losses[0], losses[-5:])
    assert moved == [], 'the reference model\'s weights must not move by a bit'
