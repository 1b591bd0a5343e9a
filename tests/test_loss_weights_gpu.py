"""Per-token loss weights end to end on the GPU (Transfusion.forward / forward_text / forward_modality with `loss_weights`), on the small fixtures (small2, text1,
head8) with the gates of tests/test_text_loss_terms_gpu.py / tests/test_model_gpu.py: all-ones weights against the unweighted step, random weights against the live
oracle with the weights applied in PyTorch to its per-token cross entropy and per-row squared errors, forward_text with {0, 1} weights against ignored labels,
forward_modality with a zero-weight entry against the call without it, the weighted step under chunking / checkpointing / LoRA / graph replay, and a ragged
two-batch sequence on one bucketed plan.  The oracle's token-grid weights are laid out by `_oracle_grid` below, written from the packing contract alone."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case, build_modality_case, build_text_case, with_grad          # noqa: E402

import test_model_gpu as TM                                            # noqa: E402
import test_text_head_gpu as TH                                        # noqa: E402
import test_text_loss_terms_gpu as TT                                  # noqa: E402  (_compare_with_oracle, _per_param_worst)

GAP, GAP_TEXT, GRAD_EQ = TH.GAP, TH.GAP_TEXT, TH.GRAD_EQ
rel, sync = TM.rel, TH.sync
F = torch.nn.functional


def _is_mod(p):
    return isinstance(p, tuple) or p.is_floating_point()


def _random_weights(batch, seed, ones=False):
    """forward()'s `loss_weights` for a batch: per text part a 1-D tensor on [0, 2] with zeros, a scalar or None in turn; per modality part a scalar (zeros among them)"""
    g = torch.Generator().manual_seed(seed)
    out, k = [], 0
    for sample in batch:
        ws = []
        for p in sample:
            k += 1
            if ones:
                ws.append([None, 1.0, torch.tensor(1.0)][k % 3] if _is_mod(p) or k % 2 else torch.ones(p.numel()))
            elif _is_mod(p):
                ws.append([0.0, 1.5, torch.tensor(0.5), None][k % 4])
            elif k % 3 == 0:
                ws.append([0.0, 0.75][k % 2])
            else:
                w = 2. * torch.rand(p.numel(), generator=g)
                w[torch.rand(p.numel(), generator=g) < 0.3] = 0.
                ws.append(w)
        out.append(ws)
    return out


def _oracle_grid(batch, lw):
    """(grid (b, n_full) with element [i, j] the weight of predicting token j of row i, instance weights in scan order), from the packing contract: per sample
    [sos] parts [eos]; an instance is [meta] chars(shape string) [som] L slots [eom]"""
    rows, w_inst = [], []
    for sample, ws in zip(batch, lw):
        row, last = [0.0], 1.0
        for p, w in zip(sample, ws if ws is not None else [None] * len(sample)):
            w = 1.0 if w is None else w
            if _is_mod(p):
                x = p[1] if isinstance(p, tuple) else p
                s = float(w)
                n_ins = 1 + len(','.join(map(str, x.shape[:-1]))) + 1
                row += [s] * (n_ins + x[..., 0].numel() + 1)
                w_inst.append(s); last = s
            elif torch.is_tensor(w) and w.ndim == 1:
                row += w.tolist(); last = float(w[-1]) if w.numel() else last
            else:
                row += [float(w)] * p.numel(); last = float(w)
        rows.append(row + [last])
    n = max(map(len, rows))
    return torch.tensor([r + [0.0] * (n - len(r)) for r in rows]), torch.tensor(w_inst)


def _oracle_weighted(cfg, sdg, batch, times, noise, lw):
    """the oracle's step with the weights applied in PyTorch: (loss, text mean, flow means per type present)"""
    from oracle.transfusion_oracle import forward_train
    ref = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    P, lab = ref['packed'], ref['labels']
    grid, w_inst = _oracle_grid(batch, lw)
    assert grid.shape[1] == lab.shape[1] + 1
    wl = grid[:, 1:].reshape(-1)
    per = F.cross_entropy(ref['logits'].reshape(lab.numel(), -1), lab.reshape(-1), ignore_index=cfg.ignore_index, reduction='none')
    valid = (lab.reshape(-1) != cfg.ignore_index).float()
    total = float(P.total_tokens)
    loss = cfg.text_loss_weight * (wl * per).sum() / total
    text = (wl * per).sum() / (wl * valid).sum()
    flows = []
    for t in sorted(ref['pred_flows']):
        wr = w_inst[P.inst_of_row[t]]
        sse = (wr[:, None] * (ref['pred_flows'][t] - ref['flows'][t]) ** 2).sum() / cfg.dim_latents[t]
        loss = loss + cfg.flow_loss_weight * sse / total
        flows.append(sse / wr.sum() if float(wr.sum()) > 0 else torch.zeros(()))
    return loss, text, flows


def _model(name, rows=None):
    cfg, sd, batch, times, noise = build_case(name)
    m = TH._native(cfg, sd, rows)
    m._noise_override = {t: v.cuda() for t, v in noise.items()}
    return m, batch, times


def _step(m, batch, times, lw):
    loss, bd = m(batch, times=times, return_breakdown=True, loss_weights=lw)
    loss.backward()
    return loss, bd


@functools.lru_cache(maxsize=None)
def _weighted(name):
    """the plain weighted step of a fixture under its random weights: (snapshot, breakdown text, flows)"""
    m, batch, times = _model(name)
    loss, bd = _step(m, batch, times, _random_weights(batch, 5))
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.weighted and plan.chunk is None and not plan.ckpt
    return s, float(bd.text), [float(f) for f in bd.flow]


# ================================================================================================ all ones, the oracle
@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_all_ones_reproduce_the_unweighted_step(name):
    plain, _ = TH._plain(name)
    m, batch, times = _model(name)
    loss0, bd0 = m(batch, times=times, return_breakdown=True)
    loss, bd = _step(m, batch, times, _random_weights(batch, 0, ones=True))
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.weighted and all(_n(i) != 'tfx_ce_fwd_bwd' and _n(i) != 'tfx_mse_fwd_bwd' for i in plan.fwd)
    TH._assert_gap(s, plain, f'{name}: all-ones weights against the unweighted step')
    for a, b in zip([bd.text] + list(bd.flow), [bd0.text] + list(bd0.flow)):
        assert abs(float(a) - float(b)) <= 1e-5 * max(1., abs(float(b)))
    assert m(batch, times=times, loss_weights=None) is not None and not m._live[0].weighted, 'None is the unweighted step, on the unweighted plan'


def _n(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


@pytest.mark.parametrize('name', ['small2', 'head8'])
def test_random_weights_match_the_live_oracle(name):
    cfg, sd, batch, times, noise = build_case(name)
    lw = _random_weights(batch, 5)
    sdg = with_grad(sd)
    ref_loss, ref_text, ref_flows = _oracle_weighted(cfg, sdg, batch, times, noise, lw)
    ref_loss.backward()
    (s, text, flows) = _weighted(name)
    m, _, _ = _model(name)
    loss, bd = _step(m, batch, times, [[w.cuda() if torch.is_tensor(w) else w for w in ws] for ws in lw])      # weights already on the device: same step
    sync()
    assert abs(float(loss.detach()) - s['loss']) <= 1e-6 * abs(s['loss'])
    TT._compare_with_oracle(m, loss, ref_loss, sdg)
    for got, want in zip([bd.text] + list(bd.flow), [ref_text] + ref_flows):
        print(f'  breakdown native {float(got):.6f} oracle {float(want):.6f}')
        assert abs(float(got) - float(want.detach())) <= 2e-3 * max(1., abs(float(want.detach())))
    plain, _ = TH._plain(name)
    assert abs(s['loss'] - plain['loss']) > 1e-3 * abs(plain['loss']), 'the weighted step is another step'


def test_forward_refusals_on_the_device():
    m, batch, times = _model('small2')
    lw = _random_weights(batch, 5)
    with pytest.raises(ValueError):
        m(batch, times=times, return_loss=False, loss_weights=lw)
    with pytest.raises(ValueError):
        m(batch, times=times, loss_weights=lw[:-1])
    bad = [list(ws) for ws in lw]
    bad[0][0] = torch.full((batch[0][0].numel(),), -1.0, device='cuda')
    with pytest.raises(ValueError):
        m(batch, times=times, loss_weights=bad)
    with pytest.raises(NotImplementedError):
        m(torch.randint(0, 256, (2, 33)), loss_weights=lw)
    with pytest.raises(TypeError):
        m(batch, times, None, None, None, None, None, None, 1e-3, False, True, False, False, False, False, False, None, None, lw)      # keyword-only
    cfg, sd, _, _, _ = build_case('small2')
    from transfusion_pytorch_amd import Transfusion
    r = TM.build_native(cfg, sd).train()
    r.reconstruction_loss_weight, r.has_recon_loss = 0.1, True
    with pytest.raises(NotImplementedError):
        r(batch, times=times, loss_weights=lw)
    with pytest.raises(NotImplementedError):
        r.forward_modality(torch.randn(2, 4, 32), modality_type=0, loss_weights=[1.0, 1.0])


# ================================================================================================ forward_text, forward_modality
@pytest.mark.parametrize('rows', [None, 64], ids=['whole_head', 'rows64'])
def test_forward_text_binary_weights_equal_ignored_labels(rows):
    """(a) zero weights on a suffix of every row against forward_text on that suffix set to ignore_index: under the causal mask a dropped suffix is seen by no
    kept label, so the two calls are the same step; (b) random {0, 1} weights against the live oracle's logits with the zero-weight labels set to ignore_index"""
    from oracle.transfusion_oracle import forward_text
    cfg, sd, text = build_text_case('text1')
    b, n1 = text.shape
    cut = [60, 40, 97]
    W = torch.ones(b, n1)
    masked = text.clone()
    for i, c in enumerate(cut):
        W[i, c:] = 0.; masked[i, c:] = -1
    res = []
    for kind in ('weights', 'labels'):
        m = TH._native(cfg, sd, rows)
        loss = m.forward_text(text, loss_weights=W.cuda()) if kind == 'weights' else m.forward_text(masked)
        loss.backward()
        res.append(TH._snap(m, loss))
        assert m._live[0].weighted == (kind == 'weights') and m._live[0].chunk == rows
        if kind == 'weights':
            assert float(m._live[0].acc[1]) == float(((text[:, 1:] != -1) & (W[:, 1:] != 0)).sum()), 'acc[1] is the count'
    TH._assert_gap(res[0], res[1], f'forward_text suffix weights against ignored labels, rows {rows}', GAP_TEXT)
    plain, _ = TH._plain('text1')
    assert abs(res[0]['loss'] - plain['loss']) > 1e-4 * abs(plain['loss'])
    W = (torch.rand(text.shape, generator=torch.Generator().manual_seed(3)) < 0.6).float()
    sdg = with_grad(sd)
    ref = forward_text(sdg, cfg, text, return_all=True)
    lab = torch.where(W[:, 1:] == 0, torch.full_like(text[:, 1:], cfg.ignore_index), text[:, 1:]).reshape(-1)
    ref_loss = F.cross_entropy(ref['logits'][..., :cfg.num_text_tokens].reshape(lab.numel(), -1), lab, ignore_index=cfg.ignore_index)
    ref_loss.backward()
    m = TH._native(cfg, sd, rows)
    loss = m.forward_text(text, loss_weights=W)
    loss.backward(); sync()
    TT._compare_with_oracle(m, loss, ref_loss, sdg)


def test_forward_modality_zero_weight_entry_equals_the_call_without_it():
    cfg, sd, x, times, noise, ty = build_modality_case('flow1')
    res = []
    for kind in ('weights', 'without'):
        m = TM.build_native(cfg, sd).train()
        if kind == 'weights':
            m._noise_override = {ty: noise.cuda()}
            loss, bd = m.forward_modality(x, times=times, modality_type=ty, loss_weights=torch.tensor([1.0, 0.0, 1.0]), return_loss_breakdown=True)
        else:
            m._noise_override = {ty: noise[[0, 2]].cuda()}
            loss, bd = m.forward_modality(x[[0, 2]], times=times[[0, 2]], modality_type=ty, return_loss_breakdown=True)
        loss.backward()
        res.append(TH._snap(m, loss))
        assert abs(float(bd[0]) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
        assert m._live[0].weighted == (kind == 'weights')
    print(f'  loss with a zero-weight entry {res[0]["loss"]:.6f}, without the entry {res[1]["loss"]:.6f}')
    assert abs(res[0]['loss'] - res[1]['loss']) <= 1e-5 * abs(res[1]['loss'])
    worst = TT._per_param_worst(res[0]['grads'], res[1]['grads'])
    # the two calls run other row counts (3 x 35 against 2 x 35 tokens): other GEMM tiles, split sums and bf16 roundings, not the same launches in another
    # atomic order - so the gate is the model's own per-parameter figure for two independently rounded steps (tests/test_model_gpu.py GRAD_TOL, and
    # GRAD_MEAN_TOL norm-weighted), not GRAD_EQ
    mean = sum(rel(res[0]['grads'][k], v) * float(v.norm()) for k, v in res[1]['grads'].items()) / sum(float(v.norm()) for v in res[1]['grads'].values())
    print(f'  gradients: worst {worst[0]:.3e} ({worst[1]}), norm-weighted mean {mean:.3e}')
    assert worst[0] <= TM.GRAD_TOL and mean <= TM.GRAD_MEAN_TOL
    m = TM.build_native(cfg, sd).train()
    m._noise_override = {ty: noise.cuda()}
    w = torch.tensor([0.5, 2.0, 0.0])
    loss = m.forward_modality(x, times=times, modality_type=ty, loss_weights=w)
    from oracle.transfusion_oracle import forward_modality
    ref = forward_modality(sd, cfg, x, times, noise, modality_type=ty, return_all=True)
    err = ((ref['pred_flow'] - ref['flow']) ** 2).reshape(3, -1)
    want = (w[:, None] * err).sum() / (w.sum() * err.shape[1])
    assert abs(float(loss.detach()) - float(want)) <= 2e-3 * max(1., abs(float(want))), (float(loss.detach()), float(want))


# ================================================================================================ the weighted step under the plan features
@pytest.mark.parametrize('name,rows', [('small2', 64), ('head8', 64)])
def test_chunked_weighted_step_equals_the_plain_weighted_step(name, rows):
    on, text, _ = _weighted(name)
    m, batch, times = _model(name, rows)
    loss, bd = _step(m, batch, times, _random_weights(batch, 5))
    plan = m._live[0]
    assert plan.weighted and plan.chunk == rows and len(plan._chunks()) >= 2
    TH._assert_gap(TH._snap(m, loss), on, f'{name} rows {rows}, weighted')
    assert abs(float(bd.text) - text) <= 1e-5 * abs(text)


def test_weighted_step_with_text_loss_terms_and_checkpointing():
    m, batch, times = _model('small2')
    m.set_text_loss_terms_(*TT.TERMS)
    lw = _random_weights(batch, 5)
    loss, bd = _step(m, batch, times, lw)
    on = TH._snap(m, loss)
    plan = m._live[0]
    t = m.text_loss_terms()
    assert plan.weighted and plan.reg == TT.TERMS and float(t.text) == float(bd.text) == float(plan.acc[0] / plan.acc[1]) and float(t.ce) < float(t.text)
    assert abs(float(t.ce) - _weighted('small2')[1]) <= 2e-3 * _weighted('small2')[1], 'ce is the weighted mean of the plain cross entropy'
    m2, _, _ = _model('small2', 64)
    m2.set_text_loss_terms_(*TT.TERMS).set_activation_checkpointing_(True)
    loss2, _ = _step(m2, batch, times, lw)
    plan = m2._live[0]
    assert plan.weighted and plan.ckpt and plan.chunk == 64 and plan.reg == TT.TERMS and plan._recompute
    TH._assert_gap(TH._snap(m2, loss2), on, 'weights + terms + chunking + checkpointing')


def test_weighted_step_with_lora_and_a_frozen_base():
    from transfusion_pytorch_amd.lora import add_lora_, lora_parameters
    on, _, _ = _weighted('small2')
    res = {}
    for kind in ('random', 'ones', 'none'):
        m, batch, times = _model('small2')
        torch.manual_seed(11)                                               # (the adapters' A is drawn at random: the same draw for the three models)
        add_lora_(m, rank=8)
        lw = None if kind == 'none' else _random_weights(batch, 5, ones=kind == 'ones')
        loss = m(batch, times=times, loss_weights=lw)
        loss.backward(); sync()
        assert m._live[0].weighted == (kind != 'none') and all(p.grad is None for p in m.store.params.values())
        res[kind] = (float(loss.detach()), [p.grad.detach().float().clone() for p in lora_parameters(m) if p.grad is not None])
    assert abs(res['random'][0] - on['loss']) <= 1e-6 * abs(on['loss']), 'adapters start at zero: the weighted loss of the base model'
    assert res['ones'][1] and len(res['ones'][1]) == len(res['none'][1]) == len(res['random'][1])
    for a, b, c in zip(res['ones'][1], res['none'][1], res['random'][1]):
        if float(b.norm()) > 1e-7:
            assert rel(a, b) <= GRAD_EQ and rel(c, b) > 10 * GRAD_EQ and bool(torch.isfinite(c).all())


def test_weighted_step_accumulates():
    from transfusion_pytorch_amd.optim import FusedAdam
    on, _, _ = _weighted('small2')
    m, batch, times = _model('small2')
    lw = _random_weights(batch, 5)
    opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
    with opt.no_sync():
        m(batch, times=times, loss_weights=lw).backward()
    m(batch, times=times, loss_weights=lw).backward()
    sync()
    g = m.store.grad.clone()
    opt.step(); sync()
    assert rel(g, 2. * on['flat']) <= GRAD_EQ and bool(torch.isfinite(m.store.flat).all())


def test_weighted_training_graph_replay(monkeypatch):
    """TFX_TRAIN_GRAPH: the weights are device data behind fixed pointers, so from the third identical step both lists replay as graphs - with NEW weight values
    in the same buffers from the fourth step on, which a capture must not freeze"""
    from transfusion_pytorch_amd import engine
    on, _, _ = _weighted('small2')
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    m, batch, times = _model('small2')
    other = None
    for k in range(5):
        TH._clear(m)
        loss, _ = _step(m, batch, times, _random_weights(batch, 5 if k != 3 else 6)); sync()
        plan = m._live[0]
        if k >= 2:
            assert plan.fwd._auto[(0, len(plan.fwd))][1] and plan.bwd._auto[(0, len(plan.bwd))][1], 'from the third identical step both lists replay as graphs'
        if k == 3:
            other = float(loss.detach())
        else:
            TH._assert_gap(TH._snap(m, loss), on, f'TFX_TRAIN_GRAPH weighted step {k}')
    assert plan.weighted and abs(other - on['loss']) > 1e-4 * abs(on['loss']), 'new weights under the captured graph give another loss'


# ================================================================================================ bucketed plans
def test_ragged_batches_share_one_bucketed_plan_and_padding_adds_nothing(monkeypatch):
    from oracle import detdata as D
    cfg, sd, batch, times, noise = build_case('small2')
    short = [list(s) for s in batch]
    assert sum(_is_mod(p) for p in short[2]) == 3
    short[2] = short[2][:-2]                                                  # drops sample 2's last instance and the text behind it: fewer instances, fewer rows
    noise_s = D.det_noise('lossw/ragged', short, cfg.num_modalities)
    times_s = times
    lw, lw_s = _random_weights(batch, 5), _random_weights(short, 7)
    m = TH._native(cfg, sd)
    m._noise_override = {t: v.cuda() for t, v in noise.items()}
    _step(m, batch, times, lw); sync()
    first = m._live[0]
    TH._clear(m)
    m._noise_override = {t: v.cuda() for t, v in noise_s.items()}
    loss, bd = _step(m, short, times_s, lw_s)
    shared = TH._snap(m, loss)
    plan = m._live[0]
    assert plan is first and plan.weighted and plan.I > 5 and all(plan.R[t] > noise_s[t].shape[0] for t in noise_s), 'one bucketed plan for both batches'
    real = {t: noise_s[t].shape[0] for t in noise_s}
    assert all(not bool(plan.lat[t]['w_row'][real[t]:].any()) for t in real) and not bool(plan.w_inst[5:].any()), 'padding rows and instances take weight 0'
    monkeypatch.setenv('TFX_PLAN_BUCKETS', '0')
    e = TH._native(cfg, sd)
    e._noise_override = {t: v.cuda() for t, v in noise_s.items()}
    loss_e, bd_e = _step(e, short, times_s, lw_s)
    exact = TH._snap(e, loss_e)
    assert e._live[0].I == 5 and e._live[0].R == real
    TH._assert_gap(shared, exact, 'the short batch on the shared bucketed plan against its exact plan')
    assert abs(float(bd.text) - float(bd_e.text)) <= 1e-6 * abs(float(bd_e.text)) and all(abs(float(a) - float(b)) <= 1e-5 * max(abs(float(b)), 1e-3) for a, b in zip(bd.flow, bd_e.flow))


# ================================================================================================ velocity consistency under weights
def _scaled(batch, c):
    """every weight of the batch equal to c, in the three forms a part weight takes"""
    out, k = [], 0
    for sample in batch:
        ws = []
        for p in sample:
            k += 1
            ws.append([c, torch.tensor(c)][k % 2] if _is_mod(p) or k % 3 else torch.full((p.numel(),), c))
        out.append(ws)
    return out


def test_forward_with_a_teacher_all_ones_and_uniform_scale():
    """forward(..., velocity_consistency_ema_model=teacher) under weights: all ones reproduce the unweighted step - loss, every breakdown entry, gradients -;
    every weight 0.5 halves the loss and the gradients (each token adds weight x loss / total) and leaves the weighted means of the breakdown where they were"""
    from oracle.make_golden_velocity import DELTA, velocity_case
    cfg, sd, sd_t, batch, times, noise, noise_t = velocity_case()
    res = {}
    for kind, lw in (('none', None), ('ones', _scaled(batch, 1.0)), ('half', _scaled(batch, 0.5))):
        student, teacher = TM.build_native(cfg, sd).train(), TM.build_native(cfg, sd_t).eval()
        student._noise_override = {t: v.cuda() for t, v in noise.items()}
        teacher._noise_override = {t: v.cuda() for t, v in noise_t.items()}
        loss, bd = student(batch, times=times, velocity_consistency_ema_model=teacher, velocity_consistency_delta_time=DELTA, return_breakdown=True, loss_weights=lw)
        loss.backward()
        res[kind] = (TH._snap(student, loss), [float(bd.text)] + [float(v) for v in bd.flow] + [float(v) for v in bd.velocity])
        plan = student._live[0]
        assert plan.weighted == (lw is not None) and len(bd.velocity) == len(bd.flow) and all(v > 0 for v in res[kind][1])
        if lw is not None:
            assert all(_n(i) == 'tfx_mse_w_fwd_bwd' for i in plan.vel) and len(plan.vel)
    TH._assert_gap(res['ones'][0], res['none'][0], 'teacher + all-ones weights against the unweighted step')
    half = dict(res['half'][0], loss=2. * res['half'][0]['loss'], flat=2. * res['half'][0]['flat'], head=2. * res['half'][0]['head'])
    # (halved seeds round to bf16 exactly like the whole ones: a power of two)
    TH._assert_gap(half, res['none'][0], 'teacher + every weight 0.5, doubled, against the unweighted step')
    for kind in ('ones', 'half'):
        for a, b in zip(res[kind][1], res['none'][1]):
            assert abs(a - b) <= 1e-5 * max(1., abs(b)), (kind, res[kind][1], res['none'][1])


def test_forward_modality_with_a_teacher_under_weights():
    """forward_modality's velocity term is mse(flow target, teacher flow), sample by sample: all-ones weights reproduce the unweighted call, and with a zero-weight
    entry the weighted means are those of the call without the entry"""
    from oracle import detdata as D
    cfg, sd, x, times, noise, ty = build_modality_case('flow1')
    sd_t = D.det_state_dict(cfg.state_dict_shapes(), tag='flow1/teacher')
    keep = [0, 2]

    def run(sel, w):
        m, teacher = TM.build_native(cfg, sd).train(), TM.build_native(cfg, sd_t).eval()
        m._noise_override = {ty: noise[sel].cuda()}
        loss, (fl, vel, _) = m.forward_modality(x[sel], times=times[sel], modality_type=ty, velocity_consistency_ema_model=teacher, return_loss_breakdown=True, loss_weights=w)
        loss.backward(); sync()
        assert m._live[0].weighted == (w is not None)
        return float(loss.detach()), float(fl), float(vel), TH._grads(m)
    all3 = [0, 1, 2]
    none, ones = run(all3, None), run(all3, torch.ones(3))
    zero, without = run(all3, torch.tensor([1.0, 0.0, 1.0]).cuda()), run(keep, None)
    print(f'  loss / flow / velocity: unweighted {none[:3]} all ones {ones[:3]}; zero-weight entry {zero[:3]} without it {without[:3]}')
    assert none[2] > 0 and abs(none[2] - without[2]) > 1e-3 * none[2], 'the dropped entry matters to the velocity term'
    for a, b in ((ones, none), (zero, without)):
        assert all(abs(p - q) <= 1e-5 * max(1., abs(q)) for p, q in zip(a[:3], b[:3]))
    # The weighted call keeps its divisor on the device: the seeds are written at 2 / dl and scaled by 1 / (rows' weight) in a second pass, so every seed is
    # rounded to bf16 twice where the unweighted call (2 / (rows dl) on the host) rounds once - as forward_text's seeds are against a host-side count.  The two
    # steps are therefore independently rounded ones, not the same launches in another atomic order: the gate is the model's own for such a pair
    # (tests/test_model_gpu.py GRAD_TOL per parameter, GRAD_MEAN_TOL norm-weighted), for both comparisons; the losses above agree to 1e-5.
    for a, b, what in ((ones, none, 'all ones | unweighted'), (zero, without, 'zero-weight entry | without it')):
        worst = TT._per_param_worst(a[3], b[3])
        mean = sum(rel(a[3][k], v) * float(v.norm()) for k, v in b[3].items()) / sum(float(v.norm()) for v in b[3].values())
        print(f'  gradients {what}: worst {worst[0]:.3e} ({worst[1]}), norm-weighted mean {mean:.3e}')
        assert worst[0] <= TM.GRAD_TOL and mean <= TM.GRAD_MEAN_TOL


# ================================================================================================ types whose encoder / decoder are user modules
def _unet_model():
    from oracle.make_golden_f4b import unet_case, unet_modules
    import os
    from transfusion_pytorch_amd import Transfusion
    g = torch.load(os.path.join(TM.GOLDEN, 'f4b_unet.pt'), weights_only=False)
    cfg, sd, batch, times, noises, xm, nm, tm, _ = unet_case()
    enc, dec = unet_modules(cfg.dim)
    model = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=4, modality_default_shape=(8, 8), channel_first_latent=True,
                        pre_post_transformer_enc_dec=(enc, dec), add_pos_emb=True, modality_num_dim=2, prob_uncond=0.,
                        transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads))
    model.load_state_dict({**sd, **g['ext_sd']}, strict=True)
    model = model.cuda().train()
    model._noise_override = {0: [n.cuda() for n in noises]}
    batch = [[(p[0], p[1].cuda()) if isinstance(p, tuple) else p.cuda() for p in s] for s in batch]
    return model, batch, times, (xm, nm, tm)


def _all_grads(m):
    return {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}


def test_user_encoder_decoder_type_takes_its_weights_in_pytorch():
    """a `pre_post_transformer_enc_dec` type (a stride-2 conv pair around the transformer): its flow loss is formed in PyTorch, so are its weights.
      all ones      the unweighted step (the one the reference golden of tests/test_f4b_gpu.py holds): loss, breakdown, every gradient - the conv pair's too
      breakdown     bd.flow = sum_i w_i sse_i / sum_i w_i n_i with the per-instance sse read off the model's own predictions (captured at _ext_flow_loss)
      linearity     every token adds weight x loss / total, so at fixed times and noise loss(a W1 + b W2) = a loss(W1) + b loss(W2), and the gradients alike;
                    with the all-ones point and the per-instance breakdown this fixes where each weight lands.  The three steps round their seeds and every
                    bf16 intermediate of the backward separately, so the gradients are held to the model's own gate for two independently rounded steps
                    (tests/test_model_gpu.py: GRAD_TOL per parameter, GRAD_MEAN_TOL norm-weighted), as in the zero-weight-entry test above; the loss,
                    a few hundred fp32 terms, to 1e-5."""
    res = {}
    W1 = [[torch.tensor([0.0, 1.0, 0.5, 2.0, 0.0]), 0.5, None], [2.0, torch.tensor([1.0, 0.0, 0.25, 1.5]), 0.0]]
    W2 = [[0.25, 0.0, torch.tensor([1.0, 0.0, 2.0])], [torch.tensor(0.5), 1.0, 1.5]]
    a, b = 0.5, 2.0
    val = lambda w, p: torch.ones(p.numel()) if w is None else (w if torch.is_tensor(w) and w.ndim == 1 else torch.full((p.numel(),), float(w)))
    for kind in ('none', 'ones', 'W1', 'W2', 'mix'):
        m, batch, times, _ = _unet_model()
        if kind == 'mix':
            lw = [[a * float(1.0 if w1 is None else w1) + b * float(1.0 if w2 is None else w2) if _is_mod(p) else a * val(w1, p) + b * val(w2, p)
                   for p, w1, w2 in zip(s, s1, s2)] for s, s1, s2 in zip(batch, W1, W2)]
        else:
            lw = dict(none=None, ones=_scaled(batch, 1.0), W1=W1, W2=W2)[kind]
        seen = {}
        real = m._ext_flow_loss

        def capture(t, preds, ctx, wi=None, real=real, seen=seen):
            seen.update(preds=[p.detach() for p in preds], flow=[f.detach() for f in ctx['flow']], wi=None if wi is None else wi.detach().clone())
            return real(t, preds, ctx, wi)
        m._ext_flow_loss = capture
        loss, bd = m(batch, times=times, return_breakdown=True, loss_weights=lw)
        loss.backward(); sync()
        assert m._live[0].weighted == (lw is not None) and 0 in m._live[0].ext
        res[kind] = dict(loss=float(loss.detach()), text=float(bd.text), flow=float(bd.flow[0]), grads=_all_grads(m), seen=seen)
    assert any('latent_to_model_projs' in k for k in res['none']['grads']) and any('model_to_latent_projs' in k for k in res['none']['grads'])
    # all ones
    for f in ('loss', 'text', 'flow'):
        assert abs(res['ones'][f] - res['none'][f]) <= 1e-5 * max(1., abs(res['none'][f])), f
    worst = TT._per_param_worst(res['ones']['grads'], res['none']['grads'])
    print(f'  all ones against unweighted: worst gradient {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= GRAD_EQ
    # breakdown and the instance weights that reached the PyTorch side: scan order 0.5 | 2.0, 0.0
    s = res['W1']['seen']
    assert s['wi'].tolist() == [0.5, 2.0, 0.0] and res['none']['seen']['wi'] is None
    sse = torch.stack([(p - f).square().sum() for p, f in zip(s['preds'], s['flow'])]).double().cpu()
    n = torch.tensor([p.numel() for p in s['preds']]).double()
    wi = torch.tensor([0.5, 2.0, 0.0]).double()
    want = float((wi * sse).sum() / (wi * n).sum())
    assert abs(res['W1']['flow'] - want) <= 1e-5 * want and abs(want - res['none']['flow']) > 1e-3 * want
    # linearity
    lin = a * res['W1']['loss'] + b * res['W2']['loss']
    print(f'  loss(a W1 + b W2) {res["mix"]["loss"]:.6f}, a loss(W1) + b loss(W2) {lin:.6f}')
    assert abs(res['mix']['loss'] - lin) <= 1e-5 * abs(lin) and abs(res['W1']['loss'] - res['W2']['loss']) > 1e-3 * abs(lin)
    comb = {k: a * res['W1']['grads'][k] + b * res['W2']['grads'][k] for k in res['mix']['grads']}
    worst = TT._per_param_worst(comb, res['mix']['grads'])
    ref = res['mix']['grads']
    mean = sum(rel(comb[k], v) * float(v.norm()) for k, v in ref.items()) / sum(float(v.norm()) for v in ref.values())
    print(f'  gradient linearity: worst {worst[0]:.3e} ({worst[1]}), norm-weighted mean {mean:.3e}')
    assert worst[0] <= TM.GRAD_TOL and mean <= TM.GRAD_MEAN_TOL
    # forward_modality: the weighted mean over the batch entries, in PyTorch on the unweighted plan
    m, _, _, (xm, nm, tm) = _unet_model()
    m._noise_override = {0: nm.cuda()}
    l0 = float(m.forward_modality(xm.cuda(), times=tm).detach())
    m._noise_override = {0: nm.cuda()}
    l1 = float(m.forward_modality(xm.cuda(), times=tm, loss_weights=[1.0, 1.0]).detach())
    m._noise_override = {0: nm[:1].cuda()}
    only0 = float(m.forward_modality(xm[:1].cuda(), times=tm[:1]).detach())
    m._noise_override = {0: nm.cuda()}
    lz = m.forward_modality(xm.cuda(), times=tm, loss_weights=torch.tensor([3.0, 0.0]))
    lz.backward(); sync()
    assert not m._live[0].weighted
    assert abs(l1 - l0) <= 1e-6 * abs(l0) and abs(float(lz.detach()) - only0) <= 2e-3 * abs(only0) and abs(only0 - l0) > 1e-3 * abs(l0)
