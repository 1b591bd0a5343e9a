"""Shared by tools/make_golden_selfflow.py and tests/test_self_flow_*.py: the Self-Flow parity cases and the closed-form weights of the
prediction head (values written out here, so no fixture stores weights).  TEST INFRASTRUCTURE ONLY."""
import math

import torch

# fixture name -> (oracle/cases.py case, student_layer, teacher_layer); all at rep_loss_weight = 1.0
WRAPPER_CASES = {
    'selfflow_small2_m3_m1': ('small2', -3, -1),
    'selfflow_small2_m1_m1': ('small2', -1, -1),
    'selfflow_head8_1_2': ('head8', 1, 2),
    'selfflow_head8_m1_m1': ('head8', -1, -1),
}
REP_LOSS_WEIGHT = 1.0
TEACHER_SCALE = 0.9                  # teacher weights = the case's state_dict, every learnable parameter times this
TAPS_FIXTURE, TAPS_CASE = 'selfflow_taps_small2', 'small2'
TAP_SHARE = 0.3                      # the generator picks w_k so that the tap's share is this fraction of the plain gradient's norm (named parameters)
SAMPLE_ROWS, SAMPLE_COLS = 3, 64     # samples of (b, n, d) tensors: every third position (padding positions included), the first 64 features
FROZEN = ('rotary_emb.freqs', 'transformer.to_time_cond.0.weights')


def sample(x):
    return x.detach().float()[:, ::SAMPLE_ROWS, :SAMPLE_COLS].contiguous().clone()


def head_state(dim):
    """the five parameters of student_predict_head under the reference's names (relative to the head): the hash-based deterministic uniform
    numbers of oracle/detdata.py (exact integer arithmetic, a pure function of the key), matrices within +- 1.5 / sqrt(fan_in)"""
    from oracle import detdata as D
    di = int(dim * 4 * 2 / 3)
    u = lambda key, shape, a: D.det_uniform(f'selfflow/head/{dim}/{key}', shape, -a, a).float()
    return {
        '0.gamma': u('gamma', (dim,), 0.1),
        '1.net.0.weight': u('w1', (2 * di, dim), 1.5 / math.sqrt(dim)),
        '1.net.0.bias': u('b1', (2 * di,), 0.02),
        '1.net.3.weight': u('w2', (dim, di), 1.5 / math.sqrt(di)),
        '1.net.3.bias': u('b2', (dim,), 0.02),
    }


def teacher_state(sd):
    return {k: (v.clone() if k in FROZEN else v * TEACHER_SCALE) for k, v in sd.items()}


def tap_parameter_names(depth):
    """the parameters the taps fixture holds gradients of"""
    names = ['text_embed.weight', 'transformer.layers.0.1.fn.to_qk.0.weight', 'transformer.norm.gamma', 'latent_to_model_projs.0.weight']
    for i in range(depth):
        names += [f'transformer.layers.{i}.2.fn.net.0.weight', f'transformer.layers.{i}.2.fn.net.3.weight']
    return names


def tap_indices(depth):
    return (0, 1, depth, depth + 1)
