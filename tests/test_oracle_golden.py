"""The oracle restatement vs the golden vectors the UNMODIFIED reference produced
(oracle/make_golden.py)."""
import os

import pytest
import torch

from oracle.cases import CASES, build_case, input_checksum, with_grad
from oracle.transfusion_oracle import forward_train, naive_mask

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
FAST = ['tiny1', 'small2', 'mid2', 'head8']


def load_golden(name):
    return torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)


@pytest.mark.parametrize('name', FAST + ['canon512', 'cfg4_768'])
def test_oracle_matches_reference_golden(name):
    g = load_golden(name)
    cfg, sd, batch, times, noise = build_case(name)
    assert abs(input_checksum(sd, batch, times, noise) - g['input_checksum']) <= 1e-6 * abs(g['input_checksum']), \
        'deterministic input factory drifted from the one that made the golden vectors'
    sdg = with_grad(sd)
    out = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    # fp32 CPU vs fp32 CPU, different op order only: tight tolerances
    assert abs(float(out['loss']) - float(g['loss'])) < 2e-5
    assert abs(float(out['text_loss']) - float(g['text_loss'])) < 2e-5
    for a, b in zip(out['flow_losses'], g['flow_losses']):
        assert abs(float(a) - float(b)) < 2e-5
    rs = g['row_step']
    assert (out['logits'][:, ::rs] - g['logits']).abs().max() < 2e-4
    assert (out['embed'][:, ::rs] - g['embed']).abs().max() < 2e-4
    out['loss'].backward()
    for k, gn in g['grad_norms'].items():
        go = sdg[k].grad
        assert go is not None, k
        assert abs(float(go.double().norm()) - gn) <= 1e-4 * gn + 1e-9, k
        head = g['grad_head'][k]
        assert (go.reshape(-1)[:head.numel()] - head).abs().max() <= 1e-4 * head.abs().max() + 1e-8, k
    if 'grads' in g:
        for k, gr in g['grads'].items():
            assert (sdg[k].grad - gr).norm() <= 1e-5 * gr.norm() + 1e-9, k
    # the prefix-extension mask equals the reference's naive mask (T:452-470)
    P = out['packed']
    b, n = out['kv_end'].shape
    assert torch.equal(naive_mask(P.positions, b, n), torch.arange(n)[None, None, :] < out['kv_end'][:, :, None])


def test_default_times_and_cfg_drop_match_reference_golden():
    """tests/golden/cfg1.pt: the reference's DEFAULT training call (no `times=`, CFG drop active) with its three uniform draws replaced
    by the deterministic vectors of oracle/make_golden_cfg.py.  The restatement of `default_modality_length_to_time_fn` (T:186-200)
    must give the reference's times exactly, and the drop (T:3027-3043) + null-label masking (T:3322-3323) its loss / gradients."""
    from oracle.make_golden_cfg import cfg_case
    from oracle.transfusion_oracle import default_times
    from oracle.detdata import count_instances
    g = load_golden('cfg1')
    cfg, sd, batch, noise, draws = cfg_case()
    times = default_times(torch.tensor(count_instances(batch)), draws['u_k'], draws['u_t'])
    assert torch.equal(times, g['times'])
    rows = set((draws['u_cfg'] < g['prob_uncond']).nonzero().flatten().tolist())
    assert rows == set(g['dropped_rows'].nonzero().flatten().tolist()) and len(rows) >= 2
    sdg = with_grad(sd)
    out = forward_train(sdg, cfg, batch, times, noise, return_all=True, uncond_rows=rows)
    assert abs(float(out['loss']) - float(g['loss'])) < 2e-5 and abs(float(out['text_loss']) - float(g['text_loss'])) < 2e-5
    for a, b in zip(out['flow_losses'], g['flow_losses']):
        assert abs(float(a) - float(b)) < 2e-5
    out['loss'].backward()
    for k, gn in g['grad_norms'].items():
        assert abs(float(sdg[k].grad.double().norm()) - gn) <= 1e-4 * gn + 1e-9, k
    # without the drop the loss differs: the fixture really exercises the branch
    plain = forward_train(sd, cfg, batch, times, noise)
    assert abs(float(plain) - float(g['loss'])) > 1e-2


def test_packed_layout_known_answers():
    """canonical sample packs to 1025 tokens, first instance at offset 28, stride 32."""
    cfg, sd, batch, times, noise = build_case('canon512')
    from oracle.transfusion_oracle import pack_batch
    P = pack_batch(cfg, batch)
    assert P.text.shape == (2, 1025)
    assert P.positions[0][:3] == [(0, 28, 4), (0, 60, 4), (0, 92, 4)]
    assert P.total_tokens == 2 * 1025
    cfg, sd, batch, times, noise = build_case('mid2')
    P = pack_batch(cfg, batch)
    assert P.text.shape == (2, 1025)
    assert P.positions[0][:3] == [(0, 29, 4), (1, 62, 2), (0, 93, 4)]


@pytest.mark.parametrize('name', ['tiny1'])
def test_oracle_matches_live_reference(name):
    """the reference's complete outputs of a small case - every logit and every gradient, as oracle/make_golden.py stored them from
    `ref_runner.reference_forward_backward` - held to the tolerances of a same-process comparison with the live reference"""
    ref = load_golden(name)
    assert ref['row_step'] == 1 and 'grads' in ref, 'needs the full logits and gradients of the case'
    cfg, sd, batch, times, noise = build_case(name)
    assert abs(input_checksum(sd, batch, times, noise) - ref['input_checksum']) <= 1e-6 * abs(ref['input_checksum'])
    sdg = with_grad(sd)
    out = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    out['loss'].backward()
    assert abs(float(out['loss']) - float(ref['loss'])) < 1e-5
    assert (out['logits'] - ref['logits']).abs().max() < 1e-4
    for k, gr in ref['grads'].items():
        assert (sdg[k].grad - gr).norm() <= 1e-5 * gr.norm() + 1e-9, k


def test_forward_text_restatement_matches_reference_golden():
    """pure-text path (T:2586-2664): restatement vs the reference's golden (oracle/make_golden_text.py)"""
    from oracle.cases import build_text_case, with_grad
    from oracle.transfusion_oracle import forward_text
    cfg, sd, text = build_text_case('text1')
    g = torch.load(os.path.join(GOLDEN, 'text1.pt'))
    sdg = with_grad(sd)
    out = forward_text(sdg, cfg, text, return_all=True)
    out['loss'].backward()
    assert abs(float(out['loss'].detach()) - float(g['loss'])) < 2e-5
    assert float((out['logits'].detach() - g['logits']).abs().max()) < 2e-4
    for k, v in g['grad_norms'].items():
        gn = float(sdg[k].grad.double().norm())
        assert abs(gn - v) <= 1e-4 * max(v, 1e-6), k


def test_forward_modality_restatement_matches_reference_golden():
    """pure flow path (T:2710-2869): restatement vs the reference's golden (oracle/make_golden_modality.py)"""
    from oracle.cases import build_modality_case, with_grad
    from oracle.transfusion_oracle import forward_modality
    cfg, sd, x, times, noise, ty = build_modality_case('flow1')
    g = torch.load(os.path.join(GOLDEN, 'flow1.pt'))
    sdg = with_grad(sd)
    loss = forward_modality(sdg, cfg, x, times, noise, ty)
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 2e-5
    for k, v in g['grad_norms'].items():
        gn = float(sdg[k].grad.double().norm())
        assert abs(gn - v) <= 1e-4 * max(v, 1e-6), k
    with torch.no_grad():
        pred = forward_modality(sd, cfg, x, times, None, ty)
    assert float((pred - g['pred_noloss']).abs().max()) < 2e-4


def test_velocity_consistency_restatement_matches_reference_golden():
    """velocity-consistency term (T:3084-3088, T:3378-3418): restatement vs the reference's golden (oracle/make_golden_velocity.py)"""
    from oracle.cases import with_grad
    from oracle.make_golden_velocity import DELTA, velocity_case
    from oracle.transfusion_oracle import forward_velocity
    cfg, sd, sd_t, batch, times, noise, noise_t = velocity_case()
    g = torch.load(os.path.join(GOLDEN, 'velocity1.pt'))
    sdg = with_grad(sd)
    out = forward_velocity(sdg, sd_t, cfg, batch, times, noise, noise_t, delta=DELTA, return_all=True)
    out['loss'].backward()
    assert abs(float(out['loss'].detach()) - float(g['loss'])) < 2e-5
    for a, r in zip(out['velocity'], g['velocity_losses']):
        assert abs(float(a.detach()) - float(r)) < 2e-5
    for k, v in g['grad_norms'].items():
        gn = float(sdg[k].grad.double().norm())
        assert abs(gn - v) <= 1e-4 * max(v, 1e-6), k


def test_model_output_clean_restatement_matches_reference_golden():
    """model_output_clean (T:1297, MP:100-126, MP:786-792): interleaved step (model-space conversion) and forward_modality
    (latent-space conversion, eps floor active for one instance) vs the reference's golden (oracle/make_golden_clean.py)"""
    from oracle.cases import with_grad
    from oracle.make_golden_clean import clean_case
    from oracle.transfusion_oracle import forward_modality
    cfg, sd, batch, times, noise, xm, tm, nm = clean_case()
    g = torch.load(os.path.join(GOLDEN, 'clean1.pt'))
    sdg = with_grad(sd)
    loss = forward_train(sdg, cfg, batch, times, noise)
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 2e-5 * max(1., float(g['loss']))
    for k, v in g['grad_norms'].items():
        assert abs(float(sdg[k].grad.double().norm()) - v) <= 1e-4 * max(v, 1e-6), k
    sdg = with_grad(sd)
    lm = forward_modality(sdg, cfg, xm, tm, nm, 1)
    lm.backward()
    assert abs(float(lm.detach()) - float(g['mod_loss'])) < 2e-5 * max(1., float(g['mod_loss']))
    for k, v in g['mod_grad_norms'].items():
        assert abs(float(sdg[k].grad.double().norm()) - v) <= 1e-4 * max(v, 1e-6), k
