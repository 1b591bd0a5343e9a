"""Per-token losses end to end on the GPU (Transfusion.forward / forward_text / forward_modality under `model.set_token_losses_()`), on the small fixtures (small2,
head8, text1, flow1) with the gates of tests/test_loss_weights_gpu.py / tests/test_text_head_gpu.py:
  recomposition      loss rebuilt from TokenLosses by the stated identity, to 1e-5 max(1, |loss|)
  only `loss` used   loss and gradients against the plain step (TH._assert_gap); neither fused loss kernel in the plan
  coefficients       backward() of a fixed linear function of the row values = the parent's `loss_weights` step with those coefficients (TH.GRAD_EQ)
  live oracle        per-sample means of `text`, per-instance means of `flow` (2e-3 max(1, |want|)); a DPO-shaped loss through TT._compare_with_oracle; per token
                     1.5 x the oracle's own bf16-autocast deviation (the project's parity rule), worst element and root mean square
  text_loss_weight   0 with a gradient through TokenLosses.text alone = 1 through the recomposed text term
  composition        chunking with a ragged last chunk, checkpointing, LoRA on a frozen trunk, loss_weights, graph replay, a ragged two-batch sequence on one
                     bucketed plan - each against the un-composed token-loss step (TH.GAP)
  no_grad            the same bits without a graph;  a second and a stale backward() raise as they always did."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case, build_modality_case, build_text_case, with_grad          # noqa: E402

import test_loss_weights_gpu as LW                                     # noqa: E402  (_random_weights, _oracle_grid, _weighted, _model)
import test_model_gpu as TM                                            # noqa: E402
import test_text_head_gpu as TH                                        # noqa: E402
import test_text_loss_terms_gpu as TT                                  # noqa: E402  (_compare_with_oracle, _per_param_worst)

GAP, GAP_TEXT, GRAD_EQ = TH.GAP, TH.GAP_TEXT, TH.GRAD_EQ
rel, sync, _model, _n = TM.rel, TH.sync, LW._model, LW._n
F = torch.nn.functional
FUSED = {'tfx_ce_fwd_bwd', 'tfx_ce_reg_fwd_bwd', 'tfx_ce_w_fwd_bwd', 'tfx_mse_fwd_bwd'}


def _recompose(m, S, tok):
    """the stated identity: text_loss_weight text.sum() / total_tokens + sum_t flow_loss_weight (flow[t].sum() / (R_t dim_latent_t)) w_t, w_t = (tokens of
    the type) / total_tokens (what `_losses` calls w)"""
    total = float(S['P'].total_tokens)
    out = m.text_loss_weight * tok.text.sum() / total
    for t, fl in zip(sorted(S['R']), tok.flow):
        out = out + m.flow_loss_weight * (fl.sum() / (fl.numel() * m.dim_latents[t])) * (float(S['tm'].is_type[t]) / total)
    return out


def _structure(m):
    """the structure of the model's latest interleaved forward (what `_recompose` reads total_tokens and the types from)"""
    return m._live[0].loaded_structure


@functools.lru_cache(maxsize=None)
def _tl(name):
    """the un-composed token-loss step of a fixture with only `loss` used: (snapshot, TokenLosses detached, structure)"""
    m, batch, times = _model(name)
    loss, tok = m.set_token_losses_()(batch, times=times)
    loss.backward()
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.token_losses and plan.chunk is None and not plan.ckpt
    return s, tok._replace(text=tok.text.detach().clone(), flow=[f.detach().clone() for f in tok.flow]), _structure(m)


# ================================================================================================ recomposition, only `loss` used
@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_loss_recomposes_from_the_row_values_and_equals_the_plain_step(name):
    s, tok, S = _tl(name)
    m, batch, times = _model(name)
    loss, bd, tok2 = m.set_token_losses_()(batch, times=times, return_breakdown=True)
    plan = m._live[0]
    b, n = len(batch), S['n_true']
    assert tok2.text.shape == tok2.text_weight.shape == (b, n) and tok2.text.dtype == torch.float32 and tok2.text.requires_grad and not tok2.text_weight.requires_grad
    assert len(tok2.flow) == len(tok2.flow_index) == len(S['R']) and all(f.shape == (S['R'][t],) and i.shape == (S['R'][t], 2) and i.dtype == torch.int64
                                                                           for t, f, i in zip(sorted(S['R']), tok2.flow, tok2.flow_index))
    want = float(loss.detach())
    got = float(_recompose(m, S, tok2).detach())
    print(f'  {name}: loss {want:.7f} recomposed {got:.7f}')
    assert abs(got - want) <= 1e-5 * max(1., abs(want))
    # text_weight is the valid mask; ignored positions are exactly 0; the breakdown's text entry is the mean over it
    lab = plan.labels.view(b, plan.n)[:, :n]
    assert torch.equal(tok2.text_weight, (lab >= 0).float()) and not bool(tok2.text[lab < 0].any()) and bool((tok2.text[lab >= 0] > 0).all())
    assert abs(float(tok2.text.sum() / tok2.text_weight.sum()) - float(bd.text)) <= 1e-5 * float(bd.text)
    assert not FUSED & {_n(i) for L in (plan.fwd, plan.bwd, plan.seed) for i in L}, 'neither fused loss kernel in the plan'
    plain, _ = TH._plain(name)
    TH._assert_gap(s, plain, f'{name}: the token-loss step with only `loss` used against the plain step')
    assert torch.is_tensor(m.set_token_losses_(False)(batch, times=times)) and not m._live[0].token_losses and not m._live[0].weighted, 'off is the plain step on the plain plan'


def test_forward_text_and_forward_modality():
    cfg, sd, text = build_text_case('text1')
    m = TH._native(cfg, sd)
    loss, tok = m.set_token_losses_().forward_text(text)
    loss.backward()
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.token_losses and tok.text.shape == (text.shape[0], text.shape[1] - 1) and tok.flow == [] and tok.flow_index == []
    want = float(loss.detach())
    assert abs(float(tok.text.sum() / tok.text_weight.sum()) - want) <= 1e-5 * max(1., want)
    assert torch.equal(tok.text_weight.cpu(), (text[:, 1:] != -1).float()) and not FUSED & {_n(i) for L in (plan.fwd, plan.bwd, plan.seed) for i in L}
    plain, _ = TH._plain('text1')
    TH._assert_gap(s, plain, 'forward_text: token losses with only `loss` used against the plain step', GAP_TEXT)
    # a gradient through the rows alone: sum(text) / count is the loss itself
    m2 = TH._native(cfg, sd)
    _, tok2 = m2.set_token_losses_().forward_text(text)
    (tok2.text.sum() / tok2.text_weight.sum()).backward()
    TH._assert_gap(TH._snap(m2, loss), s, 'forward_text: backward through the row values against backward through the loss', GAP_TEXT)

    cfg, sd, x, times, noise, ty = build_modality_case('flow1')
    res = {}
    for kind in ('plain', 'loss', 'rows'):
        m = TM.build_native(cfg, sd).train()
        m._noise_override = {ty: noise.cuda()}
        if kind == 'plain':
            loss = m.forward_modality(x, times=times, modality_type=ty)
            loss.backward()
        else:
            loss, bd, tok = m.set_token_losses_().forward_modality(x, times=times, modality_type=ty, return_loss_breakdown=True)
            rows = x.shape[0] * x[0, ..., 0].numel()
            assert m._live[0].token_losses and tok.flow[0].shape == (rows,) and tok.flow_index[0].shape == (rows, 2) and tok.text.shape == (x.shape[0], 0)
            assert tok.flow_index[0][:, 0].tolist() == [i for i in range(x.shape[0]) for _ in range(rows // x.shape[0])] and not bool(tok.flow_index[0][:, 1].any())
            re = tok.flow[0].sum() / (rows * cfg.dim_latents[ty])
            assert abs(float(re.detach()) - float(loss.detach())) <= 1e-5 * max(1., float(loss.detach()))
            (loss if kind == 'loss' else re).backward()
        res[kind] = TH._snap(m, loss)
    # (the token-loss call keeps its divisor on the device and rounds its seeds once; the plain call rounds 2 / (rows dl) on the host: two independently
    # rounded steps, held to the model's own per-parameter gate as in tests/test_loss_weights_gpu.py)
    for kind in ('loss', 'rows'):
        assert abs(res[kind]['loss'] - res['plain']['loss']) <= 1e-5 * abs(res['plain']['loss'])
        worst = TT._per_param_worst(res[kind]['grads'], res['plain']['grads'])
        print(f'  forward_modality {kind}: worst gradient {worst[0]:.3e} ({worst[1]})')
        assert worst[0] <= TM.GRAD_TOL
    assert rel(res['rows']['flat'], res['loss']['flat']) <= GRAD_EQ


# ================================================================================================ against the loss_weights step of the parent
def _coefficients(batch, lw, tok, S):
    """the coefficients of `lw` (forward()'s loss_weights) on the row values: (b, n) for `text`, per type (R_t,) for `flow`"""
    grid, w_inst = LW._oracle_grid(batch, lw)
    n = S['n_true']
    first = [0]
    for sample in batch:
        first.append(first[-1] + sum(LW._is_mod(p) for p in sample))
    first = torch.tensor(first)
    return grid[:, 1:n + 1].cuda(), [w_inst[first[ix[:, 0].cpu()] + ix[:, 1].cpu()].cuda() for ix in tok.flow_index]


def _objective(m, S, tok, ct, cf):
    total = float(S['P'].total_tokens)
    out = m.text_loss_weight * (ct * tok.text).sum()
    for t, fl, c in zip(sorted(S['R']), tok.flow, cf):
        out = out + m.flow_loss_weight * (c * fl).sum() / m.dim_latents[t]
    return out / total


@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_backward_through_fixed_coefficients_is_the_loss_weights_step(name):
    (want, _, _) = LW._weighted(name)
    m, batch, times = _model(name)
    lw = LW._random_weights(batch, 5)
    loss, tok = m.set_token_losses_()(batch, times=times)
    S = _structure(m)
    ct, cf = _coefficients(batch, lw, tok, S)
    obj = _objective(m, S, tok, ct, cf)
    obj.backward()
    s = TH._snap(m, obj)
    g = TH._gap(s, want)
    print(f'  {name}: objective {s["loss"]:.6f} weighted loss {want["loss"]:.6f}; flat gradient {g[1]:.3e} head {g[2]:.3e}')
    assert g[0] <= 1e-5 and g[1] <= GRAD_EQ and g[2] <= GRAD_EQ
    worst = TT._per_param_worst(s['grads'], want['grads'])
    print(f'  {name}: worst parameter {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= TM.GRAD_TOL


# ================================================================================================ the live oracle
@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_row_values_and_a_dpo_shaped_loss_match_the_live_oracle(name):
    from oracle.transfusion_oracle import forward_train
    cfg, sd, batch, times, noise = build_case(name)
    sdg = with_grad(sd)
    ref = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        low = forward_train(sd, cfg, batch, times, noise, return_all=True)
    P, lab = ref['packed'], ref['labels']
    b = lab.shape[0]
    per_tok = lambda r: F.cross_entropy(r['logits'].float().reshape(lab.numel(), -1), lab.reshape(-1), ignore_index=cfg.ignore_index, reduction='none').view(b, -1)
    per_row = lambda r, t: ((r['pred_flows'][t].float() - r['flows'][t].float()) ** 2).sum(dim=1)
    want_text, low_text = per_tok(ref), per_tok(low)
    valid = (lab != cfg.ignore_index).float()

    m, _, _ = _model(name)
    loss, tok = m.set_token_losses_()(batch, times=times)
    n = tok.text.shape[1]
    assert n == lab.shape[1] and torch.equal(tok.text_weight.cpu(), valid)
    text = tok.text.detach().cpu()
    # per sample, per instance: the breakdown gate
    for got, want in zip(text.sum(1) / valid.sum(1), want_text.detach().sum(1) / valid.sum(1)):
        assert abs(float(got) - float(want)) <= 2e-3 * max(1., abs(float(want))), ('text mean of a sample', float(got), float(want))
    types = sorted(ref['pred_flows'])
    first = torch.tensor([0] + [sum(LW._is_mod(p) for s in batch[:i + 1] for p in s) for i in range(b)])
    lines = []
    for t, fl, ix in zip(types, tok.flow, tok.flow_index):
        gi = first[ix[:, 0].cpu()] + ix[:, 1].cpu()
        assert torch.equal(gi, P.inst_of_row[t]), 'flow_index names the oracle\'s instance of every row'
        want_rows = per_row(ref, t).detach()
        for k in gi.unique().tolist():
            a, w = float(fl.detach().cpu()[gi == k].mean()), float(want_rows[gi == k].mean())
            assert abs(a - w) <= 2e-3 * max(1., abs(w)), ('flow mean of an instance', t, k, a, w)
        dev_o, dev_n = (per_row(low, t) - want_rows).abs(), (fl.detach().cpu() - want_rows).abs()
        lines.append((f'flow[{t}]', dev_n, dev_o))
    lines.append(('text', ((text - want_text.detach()) * valid).abs(), ((low_text - want_text.detach()) * valid).abs()))
    # per token: 1.5 x the oracle's own bf16-autocast deviation, worst element and root mean square
    for what, dn, do in lines:
        r_max, r_rms = float(dn.max() / do.max()), float(dn.square().mean().sqrt() / do.square().mean().sqrt())
        print(f'  TOKENBOUND {name} {what}: native worst {float(dn.max()):.3e} rms {float(dn.square().mean().sqrt()):.3e}; oracle bf16 worst {float(do.max()):.3e} '
              f'rms {float(do.square().mean().sqrt()):.3e}; ratios {r_max:.3f} {r_rms:.3f}')
        assert r_max <= 1.5 and r_rms <= 1.5, (what, r_max, r_rms)
    # a DPO-shaped loss over the two halves of the batch: -logsigmoid(beta (sum of one half - sum of the other)) plus a flow term per type
    beta, h = 0.1, b // 2

    def dpo(text_rows, flows):
        per = text_rows.sum(dim=1)
        out = -F.logsigmoid(beta * (per[h:2 * h].sum() - per[:h].sum()))
        for fl in flows:
            out = out + 1e-3 * (fl.sum() / fl.numel()).sqrt()
        return out
    ref_loss = dpo(want_text * valid, [per_row(ref, t) for t in types])
    ref_loss.backward()
    obj = dpo(tok.text, tok.flow)
    obj.backward(); sync()
    TT._compare_with_oracle(m, obj, ref_loss, sdg)


def test_gradient_through_text_rows_does_not_depend_on_text_loss_weight():
    s1, _, S = _tl('small2')
    res = []
    for tlw in (0.0, 1.0):
        m, batch, times = _model('small2')
        m.text_loss_weight = tlw
        loss, tok = m.set_token_losses_()(batch, times=times)
        (tok.text.sum() / float(S['P'].total_tokens)).backward()
        res.append(TH._snap(m, tok.text.sum()))
    g = TH._gap(res[0], res[1])
    print(f'  text_loss_weight 0 against 1, gradient through TokenLosses.text alone: flat {g[1]:.3e} head {g[2]:.3e}')
    assert g[1] <= GRAD_EQ and g[2] <= GRAD_EQ and float(res[0]['flat'].norm()) > 0
    # ... and it is the text part of the loss' own gradient: with flow_loss_weight 0 the whole step
    m, batch, times = _model('small2')
    m.flow_loss_weight = 0.0
    loss, _ = m.set_token_losses_()(batch, times=times)
    loss.backward()
    assert rel(res[0]['flat'], TH._snap(m, loss)['flat']) <= GRAD_EQ


# ================================================================================================ composition
def _tl_step(m, batch, times, **kw):
    loss, tok = m.set_token_losses_()(batch, times=times, **kw)
    loss.backward()
    return loss, tok


@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_chunked_with_a_ragged_last_chunk(name):
    on, tok0, _ = _tl(name)
    rows = TH._ragged_rows(TH._plain(name)[1])
    m, batch, times = _model(name, rows)
    loss, tok = _tl_step(m, batch, times)
    plan = m._live[0]
    assert plan.token_losses and plan.chunk == rows and len(plan._chunks()) >= 2 and plan.T % rows
    assert [_n(i) for i in plan.seed] == ['tfx_mse_w_fwd_bwd'] * len([t for t in plan.R if t not in plan.ext])
    TH._assert_gap(TH._snap(m, loss), on, f'{name} rows {rows}, token losses')
    assert float((tok.text.detach() - tok0.text).abs().max()) <= 1e-5 * float(tok0.text.max())


def test_checkpointing_and_text_loss_terms():
    m, batch, times = _model('small2')
    m.set_text_loss_terms_(*TT.TERMS)
    loss, tok = _tl_step(m, batch, times)
    on = TH._snap(m, loss)
    S = _structure(m)
    assert abs(float(_recompose(m, S, tok).detach()) - on['loss']) <= 1e-5 * max(1., on['loss']) and m._live[0].reg == TT.TERMS
    assert float(tok.text.sum()) > float(_tl('small2')[1].text.sum()), 'the row values carry the terms'
    m2, _, _ = _model('small2', 64)
    m2.set_text_loss_terms_(*TT.TERMS).set_activation_checkpointing_(True)
    loss2, _ = _tl_step(m2, batch, times)
    plan = m2._live[0]
    assert plan.token_losses and plan.ckpt and plan.chunk == 64 and plan.reg == TT.TERMS and plan._recompute
    TH._assert_gap(TH._snap(m2, loss2), on, 'token losses + terms + chunking + checkpointing')
    m3, _, _ = _model('small2')
    m3.set_activation_checkpointing_(True)
    loss3, _ = _tl_step(m3, batch, times)
    assert m3._live[0].ckpt and m3._live[0].token_losses
    TH._assert_gap(TH._snap(m3, loss3), _tl('small2')[0], 'token losses + checkpointing')


def test_lora_on_a_frozen_trunk():
    from transfusion_pytorch_amd.lora import add_lora_, lora_parameters
    on, _, S = _tl('small2')
    res = {}
    for kind in ('plain', 'loss', 'rows'):
        m, batch, times = _model('small2')
        torch.manual_seed(11)
        add_lora_(m, rank=8)
        if kind == 'plain':
            loss = m(batch, times=times)
            loss.backward()
        else:
            loss, tok = m.set_token_losses_()(batch, times=times)
            (loss if kind == 'loss' else _recompose(m, S, tok)).backward()
        sync()
        assert m._live[0].token_losses == (kind != 'plain') and all(p.grad is None for p in m.store.params.values())
        res[kind] = (float(loss.detach()), [p.grad.detach().float().clone() for p in lora_parameters(m) if p.grad is not None])
    assert abs(res['loss'][0] - on['loss']) <= 1e-6 * abs(on['loss']), 'adapters start at zero: the loss of the base model'
    assert res['plain'][1] and len(res['plain'][1]) == len(res['loss'][1]) == len(res['rows'][1])
    for a, b, c in zip(res['loss'][1], res['rows'][1], res['plain'][1]):
        if float(c.norm()) > 1e-7:
            assert rel(a, c) <= GRAD_EQ and rel(b, c) <= GRAD_EQ


@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_with_loss_weights(name):
    on, tok0, S = _tl(name)
    m, batch, times = _model(name)
    loss, tok = _tl_step(m, batch, times, loss_weights=LW._random_weights(batch, 0, ones=True))
    assert m._live[0].token_losses
    TH._assert_gap(TH._snap(m, loss), on, f'{name}: token losses + all-ones loss weights')
    # random weights: the parent's weighted step, and the row values are w x (the unweighted ones)
    want, _, _ = LW._weighted(name)
    lw = LW._random_weights(batch, 5)
    m, batch, times = _model(name)
    loss, tok = _tl_step(m, batch, times, loss_weights=lw)
    TH._assert_gap(TH._snap(m, loss), want, f'{name}: token losses + random loss weights against the weighted step')
    ct, cf = _coefficients(batch, lw, tok, S)
    assert torch.equal(tok.text_weight, ct * tok0.text_weight)
    assert float((tok.text.detach() - ct * tok0.text).abs().max()) <= 1e-5 * float(tok0.text.max()) and not bool(tok.text[ct == 0].any())
    for fl, f0, c in zip(tok.flow, tok0.flow, cf):
        assert float((fl.detach() - c * f0).abs().max()) <= 1e-5 * float(f0.max()) and not bool(fl[c == 0].any())
    assert abs(float(_recompose(m, S, tok).detach()) - want['loss']) <= 1e-5 * max(1., want['loss'])


def test_accumulation_and_graph_replay(monkeypatch):
    from transfusion_pytorch_amd import engine
    from transfusion_pytorch_amd.optim import FusedAdam
    on, _, _ = _tl('small2')
    m, batch, times = _model('small2')
    opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
    with opt.no_sync():
        _tl_step(m, batch, times)
    _tl_step(m, batch, times)
    sync()
    assert rel(m.store.grad.clone(), 2. * on['flat']) <= GRAD_EQ
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    m, batch, times = _model('small2')
    for k in range(4):
        TH._clear(m)
        loss, tok = m.set_token_losses_()(batch, times=times)
        # from the third step on both lists replay as graphs; the row gradient of the last step is new device data behind fixed pointers
        (loss if k < 3 else loss + 0.5 * tok.text.sum() / tok.text_weight.sum()).backward(); sync()
        plan = m._live[0]
        if k >= 2:
            assert plan.fwd._auto[(0, len(plan.fwd))][1] and plan.bwd._auto[(0, len(plan.bwd))][1]
        if k < 3:
            TH._assert_gap(TH._snap(m, loss), on, f'TFX_TRAIN_GRAPH token-loss step {k}')
    assert rel(TH._snap(m, loss)['flat'], on['flat']) > 10 * GRAD_EQ, 'the row gradient reached the replayed backward'


def test_ragged_batches_share_one_bucketed_plan(monkeypatch):
    from oracle import detdata as D
    cfg, sd, batch, times, noise = build_case('small2')
    short = [list(s) for s in batch]
    short[2] = short[2][:-2]
    noise_s = D.det_noise('lossw/ragged', short, cfg.num_modalities)
    m = TH._native(cfg, sd)
    m._noise_override = {t: v.cuda() for t, v in noise.items()}
    _tl_step(m, batch, times); sync()
    first = m._live[0]
    TH._clear(m)
    m._noise_override = {t: v.cuda() for t, v in noise_s.items()}
    loss, tok = _tl_step(m, short, times)
    shared = TH._snap(m, loss)
    plan = m._live[0]
    real = {t: noise_s[t].shape[0] for t in noise_s}
    assert plan is first and plan.token_losses and all(plan.R[t] > real[t] for t in real), 'one bucketed plan for both batches'
    assert [f.numel() for f in tok.flow] == [real[t] for t in sorted(real)] and all(not bool(plan.lat[t]['row_sse'][real[t]:].any()) for t in real)
    monkeypatch.setenv('TFX_PLAN_BUCKETS', '0')
    e = TH._native(cfg, sd)
    e._noise_override = {t: v.cuda() for t, v in noise_s.items()}
    loss_e, tok_e = _tl_step(e, short, times)
    assert e._live[0].R == real
    TH._assert_gap(shared, TH._snap(e, loss_e), 'the short batch on the shared bucketed plan against its exact plan')
    assert all(float((a.detach() - b.detach()).abs().max()) <= 1e-5 * float(b.detach().max()) for a, b in zip([tok.text] + tok.flow, [tok_e.text] + tok_e.flow))


# ================================================================================================ no_grad, the backward rules
def test_no_grad_returns_the_same_bits_without_a_graph():
    _, tok0, _ = _tl('small2')
    m, batch, times = _model('small2')
    with torch.no_grad():
        loss, tok = m.set_token_losses_()(batch, times=times)
    assert not loss.requires_grad and not tok.text.requires_grad and all(not f.requires_grad for f in tok.flow)
    assert torch.equal(tok.text, tok0.text) and all(torch.equal(a, b) for a, b in zip(tok.flow, tok0.flow)) and torch.equal(tok.text_weight, tok0.text_weight)
    # (the scalar is formed from `acc`, which the blocks of a launch reach with fp32 atomics in the order they arrive: two launches on the same input may differ
    # in its last place, with or without a graph - measured 5.0449357 against 5.0449362 here; the row values have no such freedom)
    assert abs(float(loss) - _tl('small2')[0]['loss']) <= 1e-6 * _tl('small2')[0]['loss']
    assert all(torch.equal(a, b) for a, b in zip(tok.flow_index, tok0.flow_index))


def test_second_and_stale_backward_raise():
    m, batch, times = _model('small2')
    loss, tok = m.set_token_losses_()(batch, times=times)
    obj = loss + tok.text.sum() * 1e-3
    obj.backward()
    with pytest.raises(RuntimeError):
        (tok.text.sum() + tok.flow[0].sum()).backward()
    loss1, tok1 = m.set_token_losses_()(batch, times=times)
    loss2, tok2 = m.set_token_losses_()(batch, times=times)
    with pytest.raises(RuntimeError, match='stale'):
        tok1.text.sum().backward()
    tok2.flow[0].sum().backward()                                    # the latest forward's rows alone: fine, and the loss itself seeded nothing
    sync()
    assert bool(torch.isfinite(m.store.grad).all())
    with pytest.raises(ValueError):
        m.set_token_losses_()(batch, times=times, return_loss=False)
    with pytest.raises(NotImplementedError):
        m.set_token_losses_()(torch.randint(0, 256, (2, 33)))
