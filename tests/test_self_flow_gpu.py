"""SelfMaskedRepTraining (Self-Flow, reference T:3452-3569) and the hidden taps of the fused training step, on the MI355X.

Fixtures: tools/make_golden_selfflow.py (the unmodified reference on the CPU).  Tolerances: the project's own (tests/test_laser_gpu.py: loss 1e-3,
gradient norm 4e-2, norm-weighted mean 1.2e-2, worst head 8e-2) for everything the reference suite already pins; the two new quantities - the
representation loss and the representation share of the gradient g_total - g_plain - are held to 1.5 x the reference's own bf16-autocast deviation
from its fp32 value, recorded per fixture (README: the factor used for logits and gradients), the loss to 1e-3 where that is the looser bound.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _self_flow_cases as SF                                      # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, 'golden')
LOSS_TOL, GRAD_TOL, GRAD_MEAN_TOL, GRAD_HEAD_TOL = 1e-3, 4e-2, 1.2e-2, 8e-2
FLOOR_FACTOR = 1.5
SAMPLE_TOL = 2e-2                                                  # bf16 activations against fp32 ones (the kernel tests' bound for a bf16 row)
# every sampled position on its own, those behind a shorter sample's end included (the reference's mean counts them): a position that holds something
# else than the reference computes there is off by O(1); bf16 rounding (2^-8 per element, through depth + head layers) stays an order below this
ROW_TOL = 1e-1


def row_rel_max(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-30)).max())


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _build(cfg, sd):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _grads_match(named, norms, heads, what='gradients', tols=(GRAD_TOL, GRAD_MEAN_TOL, GRAD_HEAD_TOL)):
    """the rule of tests/test_laser_gpu.py::_grads_match: every norm within tols[0], heads norm-weighted mean within tols[1], worst within tols[2]"""
    worst, wsum, nsum = 0., 0., 0.
    for k, grad in named:
        if k not in norms or norms[k] < 1e-7:
            continue
        assert grad is not None, k
        r = rel(grad.float().reshape(-1)[:1024], heads[k])
        gn = float(grad.double().norm())
        assert abs(gn - norms[k]) <= tols[0] * norms[k], (k, gn, norms[k])
        worst = max(worst, r); wsum += r * norms[k]; nsum += norms[k]
    print(f'  {what}: worst head rel {worst:.3e}, norm-weighted mean {wsum / nsum:.3e}')
    assert worst <= tols[2] and wsum / nsum <= tols[1], (what, worst, wsum / nsum, tols)


def _share_match(share, norms, heads, floor_mean, floor_worst, what):
    """g_total - g_plain against the reference's same difference: norm-weighted mean and worst relative deviation of the heads within
    FLOOR_FACTOR x the reference's bf16-autocast deviation (over the parameters the generator's floor covers: share norm above 1e-6 of the largest)"""
    top = max(norms.values())
    worst, wsum, nsum, wk = 0., 0., 0., None
    for k, s in share.items():
        if k not in norms or norms[k] < 1e-6 * top or norms[k] < 1e-7:
            continue
        r = rel(s.float().reshape(-1)[:1024], heads[k])
        if r > worst:
            worst, wk = r, k
        wsum += r * norms[k]; nsum += norms[k]
    mean = wsum / nsum
    print(f'  {what}: share rel worst {worst:.3e} ({wk}; floor {floor_worst:.3e}, ratio {worst / floor_worst:.2f}), '
          f'norm-weighted mean {mean:.3e} (floor {floor_mean:.3e}, ratio {mean / floor_mean:.2f})')
    assert mean <= FLOOR_FACTOR * floor_mean and worst <= FLOOR_FACTOR * floor_worst, (what, mean, floor_mean, worst, floor_worst)


def _wrapper(g, loss_fn=None, weight=None):
    from oracle.cases import build_case
    from transfusion_pytorch_amd import SelfMaskedRepTraining
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    kw = dict(loss_fn=loss_fn) if loss_fn is not None else {}
    w = SelfMaskedRepTraining(_build(cfg, sd), rep_loss_weight=g['rep_loss_weight'] if weight is None else weight, student_layer=g['student_layer'],
                              teacher_layer=g['teacher_layer'], use_asymmetric_dropout=False, **kw).cuda()
    w.teacher.ema_model.load_state_dict(SF.teacher_state(sd), strict=True)
    w.student_predict_head.load_state_dict(SF.head_state(cfg.dim), strict=True)
    ov = {t: v.cuda() for t, v in noise.items()}
    w.student._noise_override = ov
    w.teacher.ema_model._noise_override = ov
    return w, cfg, batch, times


def _student_grads(w):
    return {k: p.grad.detach().clone() for k, p in w.student.named_parameters() if p.grad is not None}


def _plain_grads(model, batch, times):
    model.zero_grad()
    loss = model(batch, times=times)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------------------------------------ 1. parity with every fixture
@pytest.mark.parametrize('name', list(SF.WRAPPER_CASES))
def test_self_flow_matches_reference_golden(name):
    g = torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    w, cfg, batch, times = _wrapper(g)
    total, (student_loss, rep) = w(batch, num_modalities_to_times_fn=lambda n: times.cuda())
    head = w._head
    splan = w.student._live[0]
    nt, b, n = w.student._live_n_true, splan.b, splan.n
    nh = cfg.depth + 2
    ks, kt = g['student_layer'] % nh, g['teacher_layer'] % nh
    pred = head.bufs[b * n]['pred'].view(b, n, -1)[:, :nt].float()
    hidden = (splan.embed if ks == nh - 1 else splan.hid[ks]).view(b, n, -1)[:, :nt].float()
    tplan = w._teacher_plan
    target = (tplan.embed if kt == nh - 1 else tplan.hid[kt]).view(b, n, -1)[:, :nt].float()
    total.backward()
    torch.cuda.synchronize()
    f = g['floors']
    print(f'  {name}: total {float(total):.6f} / {float(g["total_loss"]):.6f}  student {float(student_loss):.6f} / {float(g["student_loss"]):.6f}  '
          f'rep {float(rep):.6f} / {float(g["rep_loss"]):.6f} (reference bf16 floor {f["rep"]:.1e})')
    assert tuple(pred.shape) == tuple(g['shape'])
    for nm, got in (('hidden', hidden), ('target', target), ('pred', pred)):
        e = rel(SF.sample(got), g[nm])
        print(f'  {nm} sample rel {e:.3e} (reference bf16 floor {f[nm]:.2e})')
        assert e <= max(SAMPLE_TOL, FLOOR_FACTOR * f[nm]), (nm, e)
        rmax = row_rel_max(SF.sample(got), g[nm])
        print(f'  {nm} worst single position rel {rmax:.3e} (bound {ROW_TOL})')
        assert rmax <= ROW_TOL, (nm, rmax)
    assert abs(float(total) - float(g['total_loss'])) <= LOSS_TOL * max(1., abs(float(g['total_loss'])))
    assert abs(float(student_loss) - float(g['student_loss'])) <= LOSS_TOL * max(1., abs(float(g['student_loss'])))
    assert abs(float(rep) - float(g['rep_loss'])) <= max(LOSS_TOL, FLOOR_FACTOR * f['rep'])
    gt = _student_grads(w)
    _grads_match(gt.items(), g['grad_norms'], g['grad_head'], 'total gradients')
    hg = {k: p.grad for k, p in w.student_predict_head.named_parameters()}
    _grads_match(hg.items(), g['head_grad_norms'], g['head_grad_head'], 'head gradients')
    # the representation share: two native steps on the same inputs
    _, gp = _plain_grads(w.student, batch, times)
    _grads_match(gp.items(), g['plain_norms'], g['plain_head'], 'plain gradients')
    share = {k: gt[k].float() - gp[k].float() for k in gp}
    _share_match(share, g['share_norms'], g['share_head'], f['share_mean'], f['share_worst'], name)


# ------------------------------------------------------------------------------------------------ 2. taps alone
def test_hidden_taps_match_reference_golden():
    from oracle.cases import build_case
    g = torch.load(os.path.join(GOLDEN, f'{SF.TAPS_FIXTURE}.pt'), weights_only=False)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    model = _build(cfg, sd)
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    _, gp = _plain_grads(model, batch, times)
    for k in SF.tap_indices(cfg.depth):
        t = g['taps'][k]
        model.zero_grad()
        loss, hiddens, tm = model(batch, times=times, return_hiddens=True, return_times=True)
        assert len(hiddens) == cfg.depth + 2 == t['n_hiddens']
        assert all(tuple(h.shape) == tuple(t['shape']) for h in hiddens)
        assert torch.equal(tm.cpu(), times.float())
        (loss + t['w'] * hiddens[k].pow(2).mean()).backward()
        torch.cuda.synchronize()
        named = dict(model.named_parameters())
        share = {nm: named[nm].grad.float() - gp[nm].float() for nm in g['names']}
        _share_match(share, t['share_norms'], t['share_head'], t['floor_mean'], t['floor_worst'], f'tap {k} (w {t["w"]})')
    # under no_grad the same call is a teacher's pass
    with torch.no_grad():
        loss2, hiddens2 = model(batch, times=times, return_hiddens=True)
    assert len(hiddens2) == cfg.depth + 2 and not hiddens2[0].requires_grad and abs(float(loss2) - float(loss)) <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. custom loss_fn
def test_custom_loss_fn_takes_the_autograd_route_and_matches_the_default():
    g = torch.load(os.path.join(GOLDEN, 'selfflow_small2_m3_m1.pt'), weights_only=False)
    outs = []
    for fn in (None, lambda p, t: 1 - F.cosine_similarity(p, t, dim=-1).mean()):
        w, cfg, batch, times = _wrapper(g, loss_fn=fn)
        total, (_, rep) = w(batch, num_modalities_to_times_fn=lambda n: times.cuda())
        total.backward()
        torch.cuda.synchronize()
        outs.append((float(total), float(rep), _student_grads(w), {k: p.grad.clone() for k, p in w.student_predict_head.named_parameters()}))
    (t0, r0, g0, h0), (t1, r1, g1, h1) = outs
    print(f'  default total {t0:.6f} rep {r0:.6f}; custom total {t1:.6f} rep {r1:.6f}')
    assert abs(t0 - t1) <= LOSS_TOL * max(1., abs(t0)) and abs(r0 - r1) <= LOSS_TOL
    _grads_match(g1.items(), {k: float(v.double().norm()) for k, v in g0.items()}, {k: v.reshape(-1)[:1024] for k, v in g0.items()}, 'custom vs default')
    _grads_match(h1.items(), {k: float(v.double().norm()) for k, v in h0.items()}, {k: v.reshape(-1)[:1024] for k, v in h0.items()}, 'custom vs default (head)')
    _grads_match(g1.items(), g['grad_norms'], g['grad_head'], 'custom vs reference')


# ------------------------------------------------------------------------------------------------ 4. no stale tap
def test_no_stale_tap_and_zero_weight():
    g = torch.load(os.path.join(GOLDEN, 'selfflow_small2_m1_m1.pt'), weights_only=False)
    w, cfg, batch, times = _wrapper(g)
    total, _ = w(batch, num_modalities_to_times_fn=lambda n: times.cuda())
    total.backward()
    model = w.student
    loss, gp = _plain_grads(model, batch, times)
    assert abs(loss - float(g['plain_loss'])) <= LOSS_TOL * max(1., abs(loss))
    _grads_match(gp.items(), g['plain_norms'], g['plain_head'], 'plain step after a tapped step')
    # a tapped forward whose backward never ran leaves nothing behind either
    w(batch, num_modalities_to_times_fn=lambda n: times.cuda())
    _, gp = _plain_grads(model, batch, times)
    _grads_match(gp.items(), g['plain_norms'], g['plain_head'], 'plain step after a tapped forward')
    w0, cfg, batch, times = _wrapper(g, weight=0.)
    total, (student_loss, rep) = w0(batch, num_modalities_to_times_fn=lambda n: times.cuda())
    assert total is student_loss and rep is w0.zero and float(rep) == 0.
    assert len(w0.teacher.ema_model._plans) == 0, 'rep_loss_weight = 0 must not run the teacher'
    total.backward()


# ------------------------------------------------------------------------------------------------ 5. it trains
def _load_example():
    import importlib.util
    path = os.path.join(os.path.dirname(HERE), 'examples', 'self_flow_label_image.py')
    spec = importlib.util.spec_from_file_location('self_flow_label_image', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('opt_kind,steps', [('fused', 40), ('torch', 10)])
def test_self_flow_trains(opt_kind, steps):
    from transfusion_pytorch_amd.optim import FusedAdam
    ex = _load_example()
    torch.manual_seed(0)
    wrapper = ex.build_wrapper()
    head0 = [p.detach().clone() for p in wrapper.student_predict_head.parameters()]
    teacher0 = wrapper.teacher.ema_model.store.flat.clone()
    opt = FusedAdam(wrapper, lr=3e-4, max_grad_norm=0.5) if opt_kind == 'fused' else torch.optim.Adam(wrapper.parameters(), lr=3e-4)
    log = ex.train(wrapper, opt, steps=steps, quiet=True)
    reps = [r for _, _, r in log]
    print(f'  {opt_kind}: rep loss first five {sum(reps[:5]) / 5:.4f} last five {sum(reps[-5:]) / 5:.4f}')
    assert all(torch.isfinite(torch.tensor([x for row in log for x in row])))
    assert sum(reps[-5:]) / 5 < sum(reps[:5]) / 5
    assert not torch.equal(teacher0, wrapper.teacher.ema_model.store.flat)
    assert all(not torch.equal(a, p.detach()) for a, p in zip(head0, wrapper.student_predict_head.parameters()))


# ------------------------------------------------------------------------------------------------ 6. the reference's two tests, restated
def cu(x):
    return x.cuda() if torch.is_tensor(x) else x


def test_self_flow():                                               # tests/test_transfusion.py:418-450 (dim 64, use_asymmetric_dropout=False)
    from torch import randint, randn
    from transfusion_pytorch_amd import SelfMaskedRepTraining, Transfusion, exists
    model = Transfusion(num_text_tokens=256, dim_latent=16, modality_default_shape=(), transformer=dict(dim=64, depth=1)).cuda()
    self_flow_wrapper = SelfMaskedRepTraining(model, use_asymmetric_dropout=False, student_dropout_rate=0.1, teacher_dropout_rate=0., rep_loss_weight=0.1,
                                              student_layer=-1, teacher_layer=-1).cuda()
    text_and_embeds = [
        [randint(0, 256, (16,)), randn(16), randint(0, 256, (8,)), randn(16)],
        [randint(0, 256, (16,)), randn(16), randint(0, 256, (5,)), randn(16), randint(0, 256, (9,))]
    ]
    text_and_embeds = [[cu(x) for x in s] for s in text_and_embeds]
    total_loss, (student_loss, self_flow_loss) = self_flow_wrapper(text_and_embeds)
    total_loss.backward()
    self_flow_wrapper.update_teacher()
    assert exists(self_flow_loss) and exists(student_loss)
    assert total_loss.shape == ()
    assert all(p.grad is not None for p in self_flow_wrapper.student_predict_head.parameters())


def test_e2e_self_flow_with_cfg():                                  # tests/test_transfusion.py:527-557 (dim 64, use_asymmetric_dropout=False)
    from torch import randint, randn
    from transfusion_pytorch_amd import SelfMaskedRepTraining, Transfusion
    model = Transfusion(num_text_tokens=32, dim_latent=16, prob_uncond=0.1, modality_default_shape=(4,), transformer=dict(dim=64, depth=1)).cuda()
    wrapper = SelfMaskedRepTraining(model, use_asymmetric_dropout=False, student_dropout_rate=0.1, teacher_dropout_rate=0., rep_loss_weight=0.1,
                                    student_layer=-1, teacher_layer=-1).cuda()
    data = [
        [randint(0, 32, (12,)), randn(4, 16), randint(0, 32, (6,))]
    ]
    data = [[cu(x) for x in s] for s in data]
    total_loss, (student_loss, self_flow_loss) = wrapper(data)
    total_loss.backward()
    wrapper.update_teacher()
    assert total_loss.ndim == 0


# ------------------------------------------------------------------------------------------------ the kernel alone, the plans, the optimizers
@pytest.mark.parametrize('d,ld,n_pad,n_valid', [(64, 64, 0, 0), (512, 512, 16, 11), (576, 640, 16, 16), (1024, 1024, 8, 5), (1088, 1152, 0, 0), (2048, 2048, 16, 9)])
def test_cosine_kernel_matches_torch(d, ld, n_pad, n_valid):
    """tfx_cosine_fwd_bwd alone against fp32 autograd of F.cosine_similarity on the same bf16 rows: every register width (d <= 512, <= 1024, <= 2048),
    leading dimensions above d, every row counting (n_pad = 0) or a prefix of each group, a zero row (norm under eps) and a tiny one.  Bounds: the sum is
    fp32 over fp32 dot products (1e-5 relative to the row count), d pred is rounded to bf16 once (2^-9 relative per element: 4e-3 norm-relative)."""
    from transfusion_pytorch_amd import capi
    torch.manual_seed(d + n_pad)
    T = 48
    pred = torch.zeros(T, ld, device='cuda', dtype=torch.bfloat16); target = torch.zeros(T, ld, device='cuda', dtype=torch.bfloat16)
    pred[:, :d] = torch.randn(T, d, device='cuda'); target[:, :d] = torch.randn(T, d, device='cuda') * 3
    pred[:, d:] = 7.; target[:, d:] = -5.                            # columns past d must not be read
    pred[3, :d] = 0.; pred[5, :d] = 1e-12
    dpred = torch.full((T, ld), 9., device='cuda', dtype=torch.bfloat16)
    acc = torch.zeros(1, device='cuda')
    scale = 0.37
    a = capi.make_args('tfx_cosine_args', T=T, d=d, pred=pred, ld_pred=ld, target=target, ld_target=ld, n_pad=n_pad, n_valid=n_valid, grad_scale=scale,
                       dpred=dpred, ld_d=ld, acc=acc)
    capi.call('tfx_cosine_fwd_bwd', a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = pred[:, :d].float().requires_grad_(True)
    y = target[:, :d].float()
    counts = torch.ones(T, dtype=torch.bool, device='cuda') if n_pad == 0 else (torch.arange(T, device='cuda') % n_pad) < n_valid
    # the sum by the stated formula (rows under eps included); the gradient against autograd on the ordinary rows (at |x| <= eps the clamp's
    # derivative is a convention: those two rows are held to "finite" below)
    c = (x.detach().double() * y.double()).sum(-1) / (x.detach().double().norm(dim=-1).clamp(min=1e-8) * y.double().norm(dim=-1).clamp(min=1e-8))
    want_sum = float(c[counts].sum())
    ordinary = counts.clone(); ordinary[3] = ordinary[5] = False
    (-scale * F.cosine_similarity(x, y, dim=-1)[ordinary].sum()).backward()
    e = rel(dpred[ordinary][:, :d], x.grad[ordinary])
    print(f'  d {d}: sum {float(acc[0]):.6f} / {want_sum:.6f}; d pred rel {e:.3e}')
    assert abs(float(acc[0]) - want_sum) <= 1e-5 * T
    assert e <= 4e-3
    if (~counts).any():
        assert float(dpred[~counts][:, :d].abs().max()) == 0.
    assert torch.isfinite(dpred.float()).all()
    if ld > d:
        assert float((dpred[:, d:].float() - 9.).abs().max()) == 0., 'columns past d were written'


def _small_wrapper(**kw):
    from transfusion_pytorch_amd import SelfMaskedRepTraining, Transfusion
    model = Transfusion(num_text_tokens=32, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=64, depth=3)).cuda()
    return SelfMaskedRepTraining(model, use_asymmetric_dropout=False, rep_loss_weight=0.5, student_layer=-3, teacher_layer=-1, **kw).cuda()


def _ragged(n_mod, seed):
    g = torch.Generator().manual_seed(seed)
    sample = []
    for i in range(n_mod):
        sample += [torch.randint(0, 32, (5 + i,), generator=g).cuda(), torch.randn(4, 16, generator=g).cuda()]
    return [sample, sample[:2] + [torch.randint(0, 32, (3,), generator=g).cuda()]]


def test_ragged_batches_share_the_teachers_plan():
    """the teacher's hiddens-only plan is bucketed like the student's training plan: batches with different instance and latent-row counts reuse it"""
    w = _small_wrapper()
    for n_mod, seed in ((2, 0), (3, 1), (4, 2)):
        total, _ = w(_ragged(n_mod, seed))
        total.backward()
        assert torch.isfinite(total)
    ema = w.teacher.ema_model
    print(f'  plans: student {len(w.student._plans)}, teacher {len(ema._plans)}')
    assert len(ema._plans) == 1 and len(w.student._plans) == 1
    assert not next(iter(ema._plans.values())).pull, 'the teacher runs on a plan without backward state'
    # and the full training plan gives the same target
    w.teacher_hiddens_only = False
    torch.manual_seed(3); w(_ragged(3, 1)); a = w._teacher_plan.embed.clone()
    w.teacher_hiddens_only = True
    torch.manual_seed(3); w(_ragged(3, 1)); b = w._teacher_plan.embed
    assert torch.equal(a, b)


def test_fused_muon_steps_the_wrapper():
    from transfusion_pytorch_amd.optim import FusedMuon
    w = _small_wrapper()
    opt = FusedMuon(w, lr=3e-4, muon_lr=1e-3, max_grad_norm=0.5)
    head0 = [p.detach().clone() for p in w.student_predict_head.parameters()]
    flat0 = w.student.store.flat.clone()
    for step in range(2):
        total, _ = w(_ragged(2, step))
        total.backward()
        opt.step(); opt.zero_grad()
        w.update_teacher()
    assert torch.isfinite(total)
    assert not torch.equal(flat0, w.student.store.flat)
    assert all(not torch.equal(a, p.detach()) for a, p in zip(head0, w.student_predict_head.parameters()))
