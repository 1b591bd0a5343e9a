"""Generate the LoRA fixtures tests/golden/lora_*.pt from the UNMODIFIED reference (only where the reference is present).

    python tools/make_golden_lora.py                 # all of them
    python tools/make_golden_lora.py lora_head8

TEST INFRASTRUCTURE ONLY.  The reference has no adapters: it is loaded with W_eff = W + s B A as the weights of the adapted matrices (deterministic, non-zero
A and B - with B = 0, dA would vanish) on the deterministic inputs and state_dict of oracle/cases.py, and its weight gradients dW give, in float64,
    dA_ref = s B^T dW        dB_ref = s dW A^T
- the chain rule through W_eff, whatever the adapter kernels do.  On the pattern of tools/make_golden_ablation.py every fixture also records
  plain_loss          the reference's loss without the adapters (a model that ignores them cannot pass: tests/test_lora_cpu.py)
  bf16_logits_rel     rel-Frobenius deviation of the reference's own bf16-autocast logits from its fp32 logits
  bf16_grad_rel       the same for every dA / dB: derived from the bf16-autocast run's dW
  dW                  the reference's full dW of ONE adapted matrix (a trainable base weight beside its adapter, tests/test_lora_gpu.py)
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
REF = 'lucidrains/transfusion-pytorch v0.19.4'
MODULE = {'to_qk': '1.fn.to_qk.0', 'to_v': '1.fn.to_v.0', 'to_out': '1.fn.to_out.1', 'net.0': '2.fn.net.0', 'net.3': '2.fn.net.3'}
ALL = ('to_qk', 'to_v', 'to_out', 'net.0', 'net.3')
# fixture -> (case of oracle/cases.py, kind, rank, alpha, targets, layers (None = all))
CASES = {'lora_small2': ('small2', 'train', 8, 16, ALL, (1, 3)),
         'lora_head8': ('head8', 'train', 4, 4, ('to_qk', 'to_v', 'to_out'), None),
         'lora_text1': ('text1', 'text', 16, 32, ALL, (0, 2))}          # (two layers and every fourth logit row keep the file under the size limit)
TEXT_ROW_STEP = 4
# Standard deviation of B, per fixture.  Chosen on the reference alone, by two conditions `make` asserts: the adapters move the reference's loss by at least
# 10 x LOSS_TOL (a model that ignores them fails), and the reference's OWN bf16-autocast logits stay within 0.9 x LOGIT_TOL of its fp32 logits - large adapters
# grow the activations until the reference in bf16 misses the logits gate of tests/test_model_gpu.py itself, and a gate the reference's bf16 run cannot meet
# measures the fixture, not the code under test.
B_STD = {'lora_small2': 0.13, 'lora_head8': 0.2, 'lora_text1': 0.1}
LOSS_TOL, LOGIT_TOL = 1e-3, 1e-2


def adapters_for(name, sd, depth):
    """deterministic A [r, d_in] ~ N(0, 1 / d_in), B [d_out, r] ~ N(0, B_STD[name]^2) per adapted matrix, keyed by module path"""
    _, _, rank, alpha, targets, layers = CASES[name]
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    out = {}
    for i in (range(depth) if layers is None else layers):
        for t in targets:
            path = f'transformer.layers.{i}.{MODULE[t]}'
            d_out, d_in = sd[path + '.weight'].shape
            out[path] = (torch.randn(rank, d_in, generator=g) * d_in ** -0.5, torch.randn(d_out, rank, generator=g) * B_STD[name])
    return out, alpha / rank


def effective(sd, ad, s):
    sd = dict(sd)
    for path, (A, B) in ad.items():
        sd[path + '.weight'] = sd[path + '.weight'] + s * (B @ A)
    return sd


def _model(cfg, sd):
    tp = import_reference()
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    torch.manual_seed(0)
    m = tp.Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl, modality_default_shape=default_shapes(cfg),
                       transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), modality_processing='flat', prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _run(kind, model, inputs, autocast=False):
    """(loss, breakdown or None, logits) of one forward; the backward has run"""
    model.zero_grad(set_to_none=True)
    if kind == 'train':
        batch, times, noise = inputs
        cap = {}
        h = model.to_text_logits.register_forward_hook(lambda m, i, o: cap.__setitem__('logits', o.detach().float()))
        with inject_noise(noise), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            loss, bd = model(batch, times=times, return_breakdown=True)
        h.remove()
        loss.backward()
        return loss, bd, cap['logits']
    text, = inputs
    with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        loss = model.forward_text(text)
    loss.backward()
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        logits = model.forward_text(text[:, :-1], return_loss=False).float()
    return loss, None, logits[:, ::TEXT_ROW_STEP].contiguous()


def adapter_grads(model, ad, s):
    prm = dict(model.named_parameters())
    out = {}
    for path, (A, B) in ad.items():
        dW = prm[path + '.weight'].grad.double()
        out[path + '.A'] = (s * (B.double().T @ dW)).float()
        out[path + '.B'] = (s * (dW @ A.double().T)).float()
    return out


def make(name):
    base, kind, rank, alpha, targets, layers = CASES[name]
    if kind == 'train':
        cfg, sd, batch, times, noise = build_case(base)
        inputs, chk = (batch, times, noise), input_checksum(sd, batch, times, noise)
    else:
        cfg, sd, text = build_text_case(base)
        inputs, chk = (text,), float(text.double().abs().sum() + sum(float(v.double().abs().sum()) for v in sd.values()))
    ad, s = adapters_for(name, sd, cfg.depth)
    model = _model(cfg, effective(sd, ad, s)).train()
    loss, bd, logits = _run(kind, model, inputs)
    grads = adapter_grads(model, ad, s)
    dw_name = next(iter(ad)) + '.weight'
    dW = dict(model.named_parameters())[dw_name].grad.detach().clone()
    loss16, _, logits16 = _run(kind, model, inputs, autocast=True)
    grads16 = adapter_grads(model, ad, s)
    ploss, _, _ = _run(kind, _model(cfg, sd).train(), inputs)
    g = dict(case=name, base_case=base, kind=kind, rank=rank, alpha=alpha, scale=s, targets=tuple(targets), layers=layers,
             reference=f'{REF} with W + s B A as weights, modality_processing=flat, fp32, CPU', input_checksum=chk,
             A={p: a for p, (a, _) in ad.items()}, B={p: b for p, (_, b) in ad.items()},
             loss=loss.detach().double(), logits=logits.clone(), row_step=TEXT_ROW_STEP if kind == 'text' else 1, plain_loss=ploss.detach().double(),
             grads=grads, dW_name=dw_name, dW=dW,
             bf16_logits_rel=_rel(logits16, logits), bf16_grad_rel={k: _rel(grads16[k], v) for k, v in grads.items()})
    assert abs(float(g['loss']) - float(g['plain_loss'])) >= 10 * LOSS_TOL, f'{name}: the adapters move the loss by too little'
    assert g['bf16_logits_rel'] <= 0.9 * LOGIT_TOL, f"{name}: the reference's own bf16 logits deviate by {g['bf16_logits_rel']:.2e}"
    if bd is not None:
        g.update(text_loss=bd.text.detach().double(), flow_losses=[f.detach().double() for f in bd.flow])
    return g


def save(name, g):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f'{name}.pt')
    torch.save(g, path)
    assert os.path.getsize(path) < 1 << 20, f'{name}: {os.path.getsize(path)} bytes'
    worst = max(g['bf16_grad_rel'].items(), key=lambda kv: kv[1])
    print(f'{name}: loss {float(g["loss"]):.6f} (plain {float(g["plain_loss"]):.6f}), bf16-autocast logits rel {g["bf16_logits_rel"]:.2e}, '
          f'worst dA / dB rel {worst[1]:.2e} ({worst[0]}) ({os.path.getsize(path) / 1e6:.2f} MB)')


if __name__ == '__main__':
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for n in (sys.argv[1:] or CASES):
        save(n, make(n))
