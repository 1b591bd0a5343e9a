"""What per-token losses (`model.set_token_losses_()`) cost: the row-value forwards against the `_w` forwards they extend, and the whole step on the
token-loss plan - only `loss` used - against the plain step.  Alternated rounds on one process, HIP events around the launches: the method of
tools/bench_loss_weights.py.

  kernels   (arm `plain` = the `_w` launch the rows launch extends)  tfx_ce_w_fwd | tfx_ce_rows_fwd at 16 384 x 32 064 (V = 32 003: the wide kernel) and at 65 536 x 448 (V = 395: the narrow one), all-ones weights;
            tfx_mse_w_fwd_bwd | tfx_mse_rows_fwd at BASELINE config 2's latent rows (the `_w` kernel also writes d pred: the forward alone should undercut it).
            The expectation for the cross entropy is one more 4-byte store per row: the rows arm inside the spread of the `_w` arm.
  step      BASELINE config 2 (dim 512, depth 8, 64 x 1024 tokens of the canonical sample): forward, backward, clip + FusedAdam, plain | token losses, with the
            256-token vocabulary and with a 32 k one.  The split backward re-reads the fp32 logits instead of scaling bf16 seeds: reported, not gated.

Information only (profiles/token_losses.txt).  One JSON line per part.

    python tools/bench_token_losses.py
    python tools/bench_token_losses.py --rounds 2 --reps 5 --steps 3 --batch 16
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's batch)
from bench_frozen import timed_steps                        # noqa: E402
from bench_loss_weights import run_arms                     # noqa: E402
from transfusion_pytorch_amd import Transfusion, capi      # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402


def kernels(a):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    acc, aux = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    for T, V, ld in ((16384, 32003, 32064), (65536, 395, 448)):
        lg = torch.randn(T, ld, device=dev, generator=g) * 3
        lab = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
        lab[::7] = -1
        lse, rows, w = torch.empty(T, device=dev), torch.empty(T, device=dev), torch.ones(T, device=dev)
        fwd = dict(T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, z_weight=0., smoothing=0., aux=aux, row_w=w)
        arms = {'plain': ('tfx_ce_w_fwd', capi.make_args('tfx_ce_w_chunk_args', **fwd)), 'rows_fwd': ('tfx_ce_rows_fwd', capi.make_args('tfx_ce_rows_args', row_loss=rows, **fwd))}
        res[f'ce_fwd_{T}x{ld}'] = run_arms(arms, a, T * ld * 4)
        del lg
    batch = bench.canonical_batch(a.batch, dev, g)
    R = sum(p[1].shape[0] if isinstance(p, tuple) else p.shape[0] for s in batch for p in s if isinstance(p, tuple) or p.is_floating_point())
    dlat = 384
    pred, flow = torch.randn(R, dlat, device=dev, generator=g), torch.randn(R, dlat, device=dev, generator=g)
    dp, w, sse = torch.empty(R, dlat, device=dev, dtype=torch.bfloat16), torch.ones(R, device=dev), torch.zeros(R, device=dev)
    arms = {'plain': ('tfx_mse_w_fwd_bwd', capi.make_args('tfx_mse_w_args', R=R, dl=dlat, pred=pred, ld_pred=dlat, flow=flow, grad_scale=1e-3, dpred=dp, ld_d=dlat, acc=acc, row_w=w)),
            'rows_fwd': ('tfx_mse_rows_fwd', capi.make_args('tfx_mse_rows_args', R=R, dl=dlat, pred=pred, ld_pred=dlat, flow=flow, ld_d=dlat, acc=acc, row_w=w, row_sse=sse))}
    res[f'mse_{R}x{dlat}'] = run_arms(arms, a, R * dlat * 8)
    print(json.dumps(dict(part='kernels', rounds=a.rounds, reps=a.reps, **res)), flush=True)


def step(a, vocab):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=vocab, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=512, depth=8)).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.canonical_batch(a.batch, dev, gen)
    arms = {'plain': lambda b: model.set_token_losses_(False)(b), 'token_losses': lambda b: model.set_token_losses_()(b)[0]}
    res = {k: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[]) for k in arms}
    for _ in range(a.rounds):
        for name, call in arms.items():
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
            total, (f, b, o) = timed_steps(call, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            assert model._live[0].token_losses == (name == 'token_losses')
            del opt
    best = {k: {m: min(v) for m, v in r.items()} for k, r in res.items()}
    spread = {k: round(max(r['step_ms']) - min(r['step_ms']), 3) for k, r in res.items()}
    print(json.dumps(dict(part='step', vocab=vocab, dim=512, depth=8, tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam', best=best,
                          spread_ms=spread, over_plain_ms=round(best['token_losses']['step_ms'] - best['plain']['step_ms'], 3),
                          rounds_ms={k: v['step_ms'] for k, v in res.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--part', choices=('kernels', 'step', 'step32k', 'all'), default='all')
    a = ap.parse_args()
    if a.part in ('kernels', 'all'):
        kernels(a)
    if a.part in ('step', 'all'):
        step(a, 256)
    if a.part in ('step32k', 'all'):
        step(a, 32000)


if __name__ == '__main__':
    main()
