"""Generate the Self-Flow fixtures tests/golden/selfflow_*.pt from the UNMODIFIED reference (only where the reference is present).

    python tools/make_golden_selfflow.py                 # all five
    python tools/make_golden_selfflow.py selfflow_head8_1_2

TEST INFRASTRUCTURE ONLY.  The reference's `SelfMaskedRepTraining(use_asymmetric_dropout=False, rep_loss_weight=1)` on the deterministic inputs and
state_dict of oracle/cases.py; teacher = that state_dict times 0.9; head weights from tests/_self_flow_cases.py; times injected through
`num_modalities_to_times_fn`, noise through oracle.ref_runner.inject_noise (student and teacher see the same noise).  Every fixture records the
reference's fp32 values and the deviation of its own bf16-autocast run from them (the floors the GPU tolerances are multiples of).
`selfflow_taps_small2.pt` has no wrapper in it: gradients of loss + w_k * hiddens[k].pow(2).mean() minus the plain gradient.
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import _self_flow_cases as SF                                                            # noqa: E402
from oracle.cases import build_case, default_shapes, input_checksum                     # noqa: E402
from oracle.ref_runner import import_reference, inject_noise                            # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
HEAD = 1024


def _model(cfg, sd):
    tp = import_reference()
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    torch.manual_seed(0)
    m = tp.Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, modality_default_shape=default_shapes(cfg),
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads),
                       modality_processing='flat', prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m.train()


def _grads(named):
    return {k: p.grad.detach().clone() for k, p in named if p.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _pack(grads):
    return ({k: float(v.double().norm()) for k, v in grads.items()}, {k: v.reshape(-1)[:HEAD].clone() for k, v in grads.items()})


def _dev(got, ref):
    """(norm-weighted mean, worst) relative deviation of the gradient heads, over the parameters whose reference norm is not negligible"""
    worst, wsum, nsum = 0., 0., 0.
    top = max(float(v.double().norm()) for v in ref.values())
    for k, r in ref.items():
        n = float(r.double().norm())
        if n < 1e-6 * top or n < 1e-7:
            continue
        e = _rel(got[k].reshape(-1)[:HEAD], r.reshape(-1)[:HEAD])
        worst = max(worst, e); wsum += e * n; nsum += n
    return wsum / nsum, worst


def _plain(cfg, sd, batch, times, noise, autocast):
    m = _model(cfg, sd)
    with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        loss = m(batch, times=times)
    loss.backward()
    return loss.detach().double(), _grads(m.named_parameters())


def _wrapper_run(cfg, sd, batch, times, noise, ks, kt, autocast):
    tp = import_reference()
    cap = {}

    def loss_fn(pred, target):
        cap['pred'], cap['target'] = pred.detach().float(), target.detach().float()
        return tp.transfusion.default_rep_loss_fn(pred, target)
    w = tp.SelfMaskedRepTraining(_model(cfg, sd), rep_loss_weight=SF.REP_LOSS_WEIGHT, student_layer=ks, teacher_layer=kt, loss_fn=loss_fn,
                                 use_asymmetric_dropout=False)
    w.teacher.ema_model.load_state_dict(SF.teacher_state(sd), strict=True)
    w.student_predict_head.load_state_dict(SF.head_state(cfg.dim), strict=True)
    hk = w.student_predict_head.register_forward_pre_hook(lambda m, i: cap.__setitem__('hidden', i[0].detach().float()))
    with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        total, (student_loss, rep) = w(batch, num_modalities_to_times_fn=lambda n: times)
    hk.remove()
    total.backward()
    out = dict(total=total.detach().double(), student=student_loss.detach().double(), rep=rep.detach().double(),
               grads=_grads(w.student.named_parameters()), head_grads=_grads(w.student_predict_head.named_parameters()), **cap)
    return out


def make_wrapper(name):
    base, ks, kt = SF.WRAPPER_CASES[name]
    cfg, sd, batch, times, noise = build_case(base)
    r32 = _wrapper_run(cfg, sd, batch, times, noise, ks, kt, False)
    r16 = _wrapper_run(cfg, sd, batch, times, noise, ks, kt, True)
    pl32, gp32 = _plain(cfg, sd, batch, times, noise, False)
    pl16, gp16 = _plain(cfg, sd, batch, times, noise, True)
    share32 = {k: r32['grads'][k] - gp32[k] for k in gp32}
    share16 = {k: r16['grads'][k].float() - gp16[k].float() for k in gp16}
    gn, gh = _pack(r32['grads']); sn, sh = _pack(share32); pn, ph = _pack(gp32); hn, hh = _pack(r32['head_grads'])
    pnorm = sum(v ** 2 for v in pn.values()) ** 0.5
    floors = dict(rep=abs(float(r16['rep']) - float(r32['rep'])), total=abs(float(r16['total']) - float(r32['total'])),
                  pred=_rel(r16['pred'], r32['pred']), hidden=_rel(r16['hidden'], r32['hidden']), target=_rel(r16['target'], r32['target']))
    floors['grad_mean'], floors['grad_worst'] = _dev(r16['grads'], r32['grads'])
    floors['share_mean'], floors['share_worst'] = _dev(share16, share32)
    floors['head_mean'], floors['head_worst'] = _dev(r16['head_grads'], r32['head_grads'])
    return dict(case=name, base_case=base, student_layer=ks, teacher_layer=kt, rep_loss_weight=SF.REP_LOSS_WEIGHT,
                reference='lucidrains/transfusion-pytorch v0.19.4 SelfMaskedRepTraining(use_asymmetric_dropout=False), modality_processing=flat, fp32, CPU',
                input_checksum=input_checksum(sd, batch, times, noise),
                total_loss=r32['total'], student_loss=r32['student'], rep_loss=r32['rep'], loss=r32['total'], plain_loss=pl32,
                grad_norms=gn, grad_head=gh, share_norms=sn, share_head=sh, plain_norms=pn, plain_head=ph, head_grad_norms=hn, head_grad_head=hh,
                share_fraction=sum(v ** 2 for v in sn.values()) ** 0.5 / pnorm,
                shape=tuple(r32['pred'].shape), pred=SF.sample(r32['pred']), hidden=SF.sample(r32['hidden']), target=SF.sample(r32['target']),
                floors=floors)


def _tap_run(cfg, sd, batch, times, noise, k, w, autocast, names):
    m = _model(cfg, sd)
    with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        loss, hiddens = m(batch, times=times, return_loss=True, return_hiddens=True)
        total = loss + w * hiddens[k].float().pow(2).mean()
    total.backward()
    g = dict(m.named_parameters())
    return {n: g[n].grad.detach().float().clone() for n in names}, len(hiddens), tuple(hiddens[k].shape)


def make_taps(name):
    cfg, sd, batch, times, noise = build_case(SF.TAPS_CASE)
    names = SF.tap_parameter_names(cfg.depth)
    _, gp32 = _plain(cfg, sd, batch, times, noise, False)
    _, gp16 = _plain(cfg, sd, batch, times, noise, True)
    gp32 = {n: gp32[n] for n in names}; gp16 = {n: gp16[n].float() for n in names}
    pnorm = sum(float(v.double().norm()) ** 2 for v in gp32.values()) ** 0.5
    out = dict(case=name, base_case=SF.TAPS_CASE, names=names, plain_norm=pnorm, taps={},
               reference='lucidrains/transfusion-pytorch v0.19.4 Transfusion.forward(return_loss=True, return_hiddens=True), modality_processing=flat, fp32, CPU',
               input_checksum=input_checksum(sd, batch, times, noise))
    for k in SF.tap_indices(cfg.depth):
        g1, nh, shape = _tap_run(cfg, sd, batch, times, noise, k, 1.0, False, names)
        s1 = sum(float((g1[n] - gp32[n]).double().norm()) ** 2 for n in names) ** 0.5
        w = float(f'{SF.TAP_SHARE * pnorm / s1:.3g}')
        g32, _, _ = _tap_run(cfg, sd, batch, times, noise, k, w, False, names)
        g16, _, _ = _tap_run(cfg, sd, batch, times, noise, k, w, True, names)
        share32 = {n: g32[n] - gp32[n] for n in names}
        share16 = {n: g16[n] - gp16[n] for n in names}
        sn, sh = _pack(share32)
        mean, worst = _dev(share16, share32)
        out['taps'][k] = dict(w=w, share_norms=sn, share_head=sh, share_fraction=sum(v ** 2 for v in sn.values()) ** 0.5 / pnorm,
                              floor_mean=mean, floor_worst=worst, n_hiddens=nh, shape=shape)
    return out


def make(name):
    return make_taps(name) if name == SF.TAPS_FIXTURE else make_wrapper(name)


def save(name, g):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f'{name}.pt')
    torch.save(g, path)
    if name == SF.TAPS_FIXTURE:
        for k, t in g['taps'].items():
            print(f'{name}: tap {k} w {t["w"]} share {t["share_fraction"]:.3f} of the plain gradient, bf16 floor mean {t["floor_mean"]:.2e} worst {t["floor_worst"]:.2e}')
    else:
        f = g['floors']
        print(f'{name}: total {float(g["total_loss"]):.6f} student {float(g["student_loss"]):.6f} rep {float(g["rep_loss"]):.6f}, share {g["share_fraction"]:.3f}; '
              f'bf16 floors rep {f["rep"]:.1e} share mean {f["share_mean"]:.2e} worst {f["share_worst"]:.2e} grads mean {f["grad_mean"]:.2e} head mean {f["head_mean"]:.2e}')
    print(f'  {os.path.getsize(path) / 1e6:.2f} MB')


if __name__ == '__main__':
    torch.set_num_threads(1)                     # one thread: the sums of a CPU GEMM depend on the thread count, every machine has one
    for n in (sys.argv[1:] or [*SF.WRAPPER_CASES, SF.TAPS_FIXTURE]):
        save(n, make(n))
