"""Generate the LASER attention fixtures tests/golden/laser_*.pt from the UNMODIFIED reference (only where the reference is present).

    python tools/make_golden_laser.py                 # all four
    python tools/make_golden_laser.py laser_text1

TEST INFRASTRUCTURE ONLY.  The reference model is `tp.Transfusion(..., transformer=dict(..., attn_laser=True))` on the deterministic inputs and
state_dict of oracle/cases.py (LASER adds no parameters: the load is strict).  Each fixture also records, on the same inputs,
  plain_loss          the reference's loss with attn_laser=False (proves the flag was on: tests/test_laser_cpu.py)
  bf16_logits_rel     rel-Frobenius deviation of the reference's own bf16-autocast logits from its fp32 logits (the floor the GPU tolerances sit above)
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.cases import build_case, build_text_case, default_shapes, input_checksum      # noqa: E402
from oracle.ref_runner import import_reference, inject_noise                              # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
TRAIN = {'laser_small2': 'small2', 'laser_head8': 'head8'}
TEXT = {'laser_text1': 'text1'}
SAMPLING = {'laser_sampling': 'sampling'}
SAMPLING_RUNS = [('free', {}), ('forced', dict(force_modality_at_start=0)), ('forced_nocfg', dict(force_modality_at_start=0, cfg_scale=1.))]


def _model(cfg, sd, laser):
    tp = import_reference()
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    torch.manual_seed(0)
    m = tp.Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, modality_default_shape=default_shapes(cfg),
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, attn_laser=laser),
                       modality_processing='flat', prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _train_logits(model, batch, times, noise, autocast=False):
    cap = {}
    h1 = model.to_text_logits.register_forward_hook(lambda m, i, o: cap.__setitem__('logits', o.detach().float()))
    h2 = model.transformer.norm.register_forward_hook(lambda m, i, o: cap.__setitem__('embed', o.detach().float()))
    with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        loss, bd = model(batch, times=times, return_breakdown=True)
    h1.remove(); h2.remove()
    return loss, bd, cap


def make_train(name):
    cfg, sd, batch, times, noise = build_case(TRAIN[name])
    model = _model(cfg, sd, True)
    model.train()
    loss, bd, cap = _train_logits(model, batch, times, noise)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    with torch.no_grad():
        _, _, cap16 = _train_logits(model, batch, times, noise, autocast=True)
        plain = _model(cfg, sd, False).train()
        ploss, _, _ = _train_logits(plain, batch, times, noise)
    g = dict(case=name, base_case=TRAIN[name], reference='lucidrains/transfusion-pytorch v0.19.4, attn_laser=True, modality_processing=flat, fp32, CPU',
             input_checksum=input_checksum(sd, batch, times, noise),
             loss=loss.detach().double(), text_loss=bd.text.detach().double(), flow_losses=[f.detach().double() for f in bd.flow],
             logits=cap['logits'].clone(), grad_norms={k: float(v.double().norm()) for k, v in grads.items()},
             grad_head={k: v.reshape(-1)[:1024].clone() for k, v in grads.items()},
             plain_loss=ploss.detach().double(), bf16_logits_rel=_rel(cap16['logits'], cap['logits']))
    return g


def make_text(name):
    cfg, sd, text = build_text_case(TEXT[name])
    model = _model(cfg, sd, True)
    model.train()
    loss = model.forward_text(text)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    with torch.no_grad():
        logits, (kv, seen) = model.forward_text(text[:, :-1], return_loss=False, return_kv_cache=True)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            logits16 = model.forward_text(text[:, :-1], return_loss=False).float()
        ploss = _model(cfg, sd, False).train().forward_text(text)
    g = dict(case=name, base_case=TEXT[name], reference='lucidrains/transfusion-pytorch v0.19.4 forward_text, attn_laser=True, fp32, CPU',
             input_checksum=float(text.double().abs().sum() + sum(float(v.double().abs().sum()) for v in sd.values())),
             loss=loss.detach().double(), logits=logits.detach().clone(),
             grad_norms={k: float(v.double().norm()) for k, v in grads.items()},
             grad_head={k: v.reshape(-1)[:1024].clone() for k, v in grads.items()},
             plain_loss=ploss.detach().double(), bf16_logits_rel=_rel(logits16, logits),
             # the returned KV cache (T:977: stacked BEFORE the laser transform - raw v): layer 0 and the last layer, batch row 0, first 32 positions
             kv_seen=int(seen), kv_shape=tuple(kv.shape), kv_head=kv[[0, -1], :, 0, :, :32].detach().clone())
    # greedy KV-cached generation (generate_text_only, T:2666-2707) with the top-2 margin of every step
    model.eval()
    prompt = text[:, :16].clone()
    prompt[prompt < 0] = 0
    with torch.no_grad():
        gen = model.generate_text_only(prompt, 16 + 24, temperature=0.)
        full = torch.cat((prompt, gen), dim=-1)
        lg = model.forward_text(full[:, :-1], return_loss=False)[:, 15:]
    top2 = lg.topk(2, dim=-1).values
    assert torch.equal(lg.argmax(-1), gen), 'cached generation must equal the teacher-forced argmax in the fp32 reference'
    g.update(gen_prompt=prompt, gen_tokens=gen.clone(), gen_margin=(top2[..., 0] - top2[..., 1]).clone())
    return g


def make_sampling(name):
    """`sample_many` on the setup of tests/golden/sampling.pt (oracle/make_golden_sampling.py: weights, prompts, initial noise, greedy text, margins
    of every greedy decision recorded the same way), with attn_laser=True"""
    from oracle.make_golden_sampling import MarginRecorder, sampling_case, to_plain
    cfg, sd, prompts, noise = sampling_case(False)
    model = _model(cfg, sd, True).eval()
    g = dict(case=name, base_case=SAMPLING[name], reference='lucidrains/transfusion-pytorch v0.19.4 sample_many, attn_laser=True, fp32, CPU',
             runs={}, margins={})
    rec = MarginRecorder().install()
    try:
        for run, kw in SAMPLING_RUNS:
            kwargs = dict(max_length=12, text_temperature=0., init_modality_noise=noise, modality_steps=4, fixed_modality_shape=(4,), cfg_scale=3.)
            kwargs.update(kw)
            outs = model.sample_many([p if not isinstance(p, list) else list(p) for p in prompts], **kwargs)
            g['runs'][run] = [to_plain(o) for o in outs]
            g['margins'][run] = rec.take()
    finally:
        rec.remove()
    # the flag check and the bf16 floor on the same weights: forward_text of the text prompt
    text = prompts[0][None].long()
    with torch.no_grad():
        m2 = _model(cfg, sd, True).train()
        loss, ploss = m2.forward_text(text), _model(cfg, sd, False).train().forward_text(text)
        lg = m2.forward_text(text[:, :-1], return_loss=False)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            lg16 = m2.forward_text(text[:, :-1], return_loss=False).float()
    g.update(loss=loss.double(), plain_loss=ploss.double(), bf16_logits_rel=_rel(lg16, lg))
    return g


def make(name):
    if name in SAMPLING:
        return make_sampling(name)
    g = make_train(name) if name in TRAIN else make_text(name)
    return g


def save(name, g):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f'{name}.pt')
    torch.save(g, path)
    print(f'{name}: loss {float(g["loss"]):.6f} (plain {float(g["plain_loss"]):.6f}), bf16-autocast logits rel {g["bf16_logits_rel"]:.2e} '
          f'({os.path.getsize(path) / 1e6:.2f} MB)')


if __name__ == '__main__':
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for n in (sys.argv[1:] or [*TRAIN, *TEXT, *SAMPLING]):
        save(n, make(n))
