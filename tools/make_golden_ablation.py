"""Generate the attention-ablation fixtures tests/golden/ablate_*.pt from the UNMODIFIED reference (only where the reference is present).

    python tools/make_golden_ablation.py                 # all of them
    python tools/make_golden_ablation.py ablate_both_text1

TEST INFRASTRUCTURE ONLY.  The reference model is `tp.Transfusion(..., transformer=dict(..., qk_rmsnorm=False, attn_kwargs=dict(gate_values=False)))`
- either switch, or both, per fixture - on the deterministic inputs and state_dict of oracle/cases.py.  Without value gating the reference's
attention has no `to_gates` module (T:901-904): those keys are dropped from the case's state_dict before the STRICT load.  Without QK-RMSNorm it
keeps its q_norm / k_norm modules (T:893-894) and never calls them: their gammas load, and their .grad stays None.  On the pattern of tools/make_golden_laser.py every fixture also records, on
the same inputs,
  plain_loss          the reference's loss with the default attention (proves the switch was thrown: tests/test_ablation_cpu.py)
  bf16_logits_rel     rel-Frobenius deviation of the reference's own bf16-autocast logits from its fp32 logits (the floor the GPU tolerances sit above)
and, for the host layer,
  state_keys          the reference's sorted state_dict key list
  grad_none           the names of the parameters whose .grad the reference leaves None after the backward (training and text fixtures)
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
NEAR_TIE = 0.05
# fixture -> (case of oracle/cases.py, transformer switches)
NOQK, NOGATE = dict(qk_rmsnorm=False), dict(attn_kwargs=dict(gate_values=False))
BOTH = dict(NOQK, **NOGATE)
TRAIN = {'ablate_noqk_small2': ('small2', NOQK), 'ablate_nogate_small2': ('small2', NOGATE), 'ablate_both_head8': ('head8', BOTH),
         'ablate_both_laser_small2': ('small2', dict(BOTH, attn_laser=True))}
TEXT = {'ablate_both_text1': ('text1', BOTH)}
SAMPLING = {'ablate_both_sampling': ('sampling', BOTH)}
SAMPLING_RUNS = [('free', {}), ('forced', dict(force_modality_at_start=0)), ('forced_nocfg', dict(force_modality_at_start=0, cfg_scale=1.))]
REF = 'lucidrains/transfusion-pytorch v0.19.4'


def has_gates(sw):
    return sw.get('attn_kwargs', {}).get('gate_values', True)


def strip_state(sd, sw):
    """the case's state_dict in the shape the switched reference model has: no `to_gates` keys without value gating"""
    return sd if has_gates(sw) else {k: v for k, v in sd.items() if '.to_gates.' not in k}


def _model(cfg, sd, sw):
    tp = import_reference()
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    torch.manual_seed(0)
    m = tp.Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, modality_default_shape=default_shapes(cfg),
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, **sw),
                       modality_processing='flat', prob_uncond=0.)
    m.load_state_dict(strip_state(sd, sw), strict=True)
    return m


def _plain_switches(sw):
    return {k: v for k, v in sw.items() if k == 'attn_laser'}      # the same model with the default attention block (LASER is no ablation)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _train_logits(model, batch, times, noise, autocast=False):
    cap = {}
    h1 = model.to_text_logits.register_forward_hook(lambda m, i, o: cap.__setitem__('logits', o.detach().float()))
    with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        loss, bd = model(batch, times=times, return_breakdown=True)
    h1.remove()
    return loss, bd, cap


def _grad_record(model):
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return dict(grad_norms={k: float(v.double().norm()) for k, v in grads.items()},
                grad_head={k: v.reshape(-1)[:1024].clone() for k, v in grads.items()},
                grad_none=sorted(k for k, p in model.named_parameters() if p.requires_grad and p.grad is None),
                state_keys=sorted(model.state_dict()))


def make_train(name):
    base, sw = TRAIN[name]
    cfg, sd, batch, times, noise = build_case(base)
    model = _model(cfg, sd, sw)
    model.train()
    loss, bd, cap = _train_logits(model, batch, times, noise)
    loss.backward()
    with torch.no_grad():
        _, _, cap16 = _train_logits(model, batch, times, noise, autocast=True)
        ploss, _, _ = _train_logits(_model(cfg, sd, _plain_switches(sw)).train(), batch, times, noise)
    g = dict(case=name, base_case=base, switches=sw, reference=f'{REF}, {sw}, modality_processing=flat, fp32, CPU',
             input_checksum=input_checksum(sd, batch, times, noise),
             loss=loss.detach().double(), text_loss=bd.text.detach().double(), flow_losses=[f.detach().double() for f in bd.flow],
             logits=cap['logits'].clone(), plain_loss=ploss.detach().double(), bf16_logits_rel=_rel(cap16['logits'], cap['logits']))
    g.update(_grad_record(model))
    return g


def make_text(name):
    base, sw = TEXT[name]
    cfg, sd, text = build_text_case(base)
    model = _model(cfg, sd, sw)
    model.train()
    loss = model.forward_text(text)
    loss.backward()
    with torch.no_grad():
        logits, (kv, seen) = model.forward_text(text[:, :-1], return_loss=False, return_kv_cache=True)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            logits16 = model.forward_text(text[:, :-1], return_loss=False).float()
        ploss = _model(cfg, sd, _plain_switches(sw)).train().forward_text(text)
    g = dict(case=name, base_case=base, switches=sw, reference=f'{REF} forward_text, {sw}, fp32, CPU',
             input_checksum=float(text.double().abs().sum() + sum(float(v.double().abs().sum()) for v in sd.values())),
             loss=loss.detach().double(), logits=logits.detach().clone(),
             plain_loss=ploss.detach().double(), bf16_logits_rel=_rel(logits16, logits),
             # the returned KV cache: layer 0 and the last layer, batch row 0, first 32 positions
             kv_seen=int(seen), kv_shape=tuple(kv.shape), kv_head=kv[[0, -1], :, 0, :, :32].detach().clone())
    g.update(_grad_record(model))
    # greedy KV-cached generation (generate_text_only, T:2666-2707) with the top-2 margin of every step
    model.eval()
    prompt = text[:, :16].clone()
    prompt[prompt < 0] = 0
    with torch.no_grad():
        gen = model.generate_text_only(prompt, 16 + 24, temperature=0.)
        full = torch.cat((prompt, gen), dim=-1)
        lg = model.forward_text(full[:, :-1], return_loss=False)[:, 15:]
    top2 = lg.topk(2, dim=-1).values
    margin = top2[..., 0] - top2[..., 1]
    assert torch.equal(lg.argmax(-1), gen), 'cached generation must equal the teacher-forced argmax in the fp32 reference'
    decisive = float((margin > NEAR_TIE).float().mean())
    assert decisive >= 0.75, f'{name}: only {decisive:.2f} of the greedy steps have a top-2 margin above {NEAR_TIE}: choose another prompt'
    g.update(gen_prompt=prompt, gen_tokens=gen.clone(), gen_margin=margin.clone())
    return g


def make_sampling(name):
    """`sample_many` on the setup of tests/golden/sampling.pt (oracle/make_golden_sampling.py: weights, prompts, initial noise, greedy text, margins
    of every greedy decision recorded the same way), with the switches thrown"""
    from oracle.make_golden_sampling import MarginRecorder, sampling_case, to_plain
    base, sw = SAMPLING[name]
    cfg, sd, prompts, noise = sampling_case(False)
    model = _model(cfg, sd, sw).eval()
    g = dict(case=name, base_case=base, switches=sw, reference=f'{REF} sample_many, {sw}, fp32, CPU', runs={}, margins={},
             state_keys=sorted(model.state_dict()))
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
    for run, per_sample in g['margins'].items():
        ms = [v for mg in per_sample for _, _, v in mg]
        assert not ms or sum(v > NEAR_TIE for v in ms) >= 0.75 * len(ms), f'{name} [{run}]: too few decisive greedy steps'
    # the switch check and the bf16 floor on the same weights: forward_text of the text prompt
    text = prompts[0][None].long()
    with torch.no_grad():
        m2 = _model(cfg, sd, sw).train()
        loss, ploss = m2.forward_text(text), _model(cfg, sd, _plain_switches(sw)).train().forward_text(text)
        lg = m2.forward_text(text[:, :-1], return_loss=False)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            lg16 = m2.forward_text(text[:, :-1], return_loss=False).float()
    g.update(loss=loss.double(), plain_loss=ploss.double(), bf16_logits_rel=_rel(lg16, lg))
    return g


def make(name):
    if name in SAMPLING:
        return make_sampling(name)
    return make_train(name) if name in TRAIN else make_text(name)


def save(name, g):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f'{name}.pt')
    torch.save(g, path)
    assert os.path.getsize(path) < 1 << 20, f'{name}: {os.path.getsize(path)} bytes'
    print(f'{name}: loss {float(g["loss"]):.6f} (plain {float(g["plain_loss"]):.6f}), bf16-autocast logits rel {g["bf16_logits_rel"]:.2e} '
          f'({os.path.getsize(path) / 1e6:.2f} MB)')


if __name__ == '__main__':
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for n in (sys.argv[1:] or [*TRAIN, *TEXT, *SAMPLING]):
        save(n, make(n))
