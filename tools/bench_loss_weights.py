"""What per-token loss weights (`model(batch, loss_weights=...)`) cost: the `_w` loss launches against their unweighted counterparts, and the whole step with the
weights off, all ones, and half the text zeroed.  Alternated rounds on one process (the arms share the buffers, the weights and the box's drift), HIP events around
the launches - the method of tools/bench_text_loss_terms.py.

  kernels   tfx_ce_reg_fwd_bwd | tfx_ce_w_fwd_bwd at 65 536 x 448 (V = 395: the fused kernel's register path), tfx_ce_reg_fwd | tfx_ce_w_fwd and tfx_ce_reg_bwd |
            tfx_ce_w_bwd on a 16 384-row chunk x 32 064 (V = 32 003: the wide kernels), both with z = e = 0 next to the plain entry points; tfx_mse_fwd_bwd |
            tfx_mse_w_fwd_bwd at BASELINE config 2's latent rows.  The `_w` arms run all-ones weights and weights with a quarter of the rows at zero.
  step      BASELINE config 2 (dim 512, depth 8, 64 x 1024 tokens of the canonical sample): forward, backward, clip + FusedAdam with loss_weights None | all
            ones | the first half of every text part zeroed.

Per arm the best round and the spread of its rounds (max - min): the expectation is one more 4-byte load per row, so a `_w` arm inside the spread of its plain arm.
Information only (profiles/loss_weights.txt).  One JSON line per part.

    python tools/bench_loss_weights.py
    python tools/bench_loss_weights.py --rounds 2 --reps 5 --steps 3 --batch 16
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
from bench_text_loss_terms import summarise, time_launch    # noqa: E402
from transfusion_pytorch_amd import Transfusion, capi      # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402


def run_arms(arms, a, nbytes):
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (fn, args) in arms.items():
            rounds[k].append(time_launch(fn, args, a.reps))
    return summarise(rounds, nbytes)


def row_weights(n, dev, g):
    ones = torch.ones(n, device=dev)
    part = 2. * torch.rand(n, device=dev, generator=g)
    part[torch.rand(n, device=dev, generator=g) < 0.25] = 0.
    return {'w_ones': ones, 'w_quarter_zero': part}


def kernels(a):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    acc, aux = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    # ---- fused, 65 536 x 448
    T, V, ld = 65536, 395, 448
    lg = torch.randn(T, ld, device=dev, generator=g) * 3
    lab = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
    lab[::7] = -1
    dl = torch.empty(T, ld, device=dev, dtype=torch.bfloat16)
    common = dict(T=T, V=V, logits=lg, ld=ld, labels=lab, grad_scale=1e-3, dlogits=dl, ld_d=ld, acc=acc)
    reg = dict(z_weight=0., smoothing=0., aux=aux)
    arms = {'plain': ('tfx_ce_fwd_bwd', capi.make_args('tfx_ce_args', **common)), 'reg': ('tfx_ce_reg_fwd_bwd', capi.make_args('tfx_ce_reg_args', **reg, **common))}
    ws = row_weights(T, dev, g)
    for k, w in ws.items():
        arms[k] = ('tfx_ce_w_fwd_bwd', capi.make_args('tfx_ce_w_args', row_w=w, **reg, **common))
    res['fused_65536x448'] = run_arms(arms, a, T * ld * 6)
    del lg, dl
    # ---- split, a 16 384-row chunk x 32 064
    T, V, ld = 16384, 32003, 32064
    lg = torch.randn(T, ld, device=dev, generator=g) * 3
    lab = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
    lab[::7] = -1
    dl = torch.empty(T, ld, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(T, device=dev)
    common = dict(T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, grad_scale=1e-3, scale_dev=None, dlogits=dl, ld_d=ld)
    plain = capi.make_args('tfx_ce_chunk_args', **common)
    regc = capi.make_args('tfx_ce_reg_chunk_args', **reg, **common)
    ws = row_weights(T, dev, g)
    wc = {k: capi.make_args('tfx_ce_w_chunk_args', row_w=w, **reg, **common) for k, w in ws.items()}
    for d, nbytes in (('fwd', T * ld * 4), ('bwd', T * ld * 6)):
        arms = {'plain': (f'tfx_ce_{d}', plain), 'reg': (f'tfx_ce_reg_{d}', regc), **{k: (f'tfx_ce_w_{d}', v) for k, v in wc.items()}}
        res[f'{d}_16384x32064'] = run_arms(arms, a, nbytes)
    del lg, dl
    # ---- squared error at config 2's latent rows
    batch = bench.canonical_batch(a.batch, dev, g)
    R = sum(p[1].shape[0] if isinstance(p, tuple) else p.shape[0] for s in batch for p in s if isinstance(p, tuple) or p.is_floating_point())
    dlat, ldd = 384, 384
    pred, flow = torch.randn(R, dlat, device=dev, generator=g), torch.randn(R, dlat, device=dev, generator=g)
    dp = torch.empty(R, ldd, device=dev, dtype=torch.bfloat16)
    common = dict(R=R, dl=dlat, pred=pred, ld_pred=dlat, flow=flow, grad_scale=1e-3, dpred=dp, ld_d=ldd, acc=acc)
    arms = {'plain': ('tfx_mse_fwd_bwd', capi.make_args('tfx_mse_args', **common))}
    for k, w in row_weights(R, dev, g).items():
        arms[k] = ('tfx_mse_w_fwd_bwd', capi.make_args('tfx_mse_w_args', row_w=w, **common))
    res[f'mse_{R}x{dlat}'] = run_arms(arms, a, R * dlat * 10)
    print(json.dumps(dict(part='kernels', rounds=a.rounds, reps=a.reps, **res)), flush=True)


def step(a):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=256, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=512, depth=8)).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.canonical_batch(a.batch, dev, gen)
    is_text = lambda p: not isinstance(p, tuple) and not p.is_floating_point()

    def half(p):
        w = torch.ones(p.numel(), device=dev)
        w[:p.numel() // 2] = 0.
        return w
    arms = {'off': None, 'ones': [[torch.ones(p.numel(), device=dev) if is_text(p) else 1.0 for p in s] for s in batch],
            'half_text_zero': [[half(p) if is_text(p) else None for p in s] for s in batch]}
    res = {k: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[]) for k in arms}
    losses = {}
    for _ in range(a.rounds):
        for name, lw in arms.items():
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
            call = (lambda b, lw=lw: model(b, loss_weights=lw)) if lw is not None else model
            total, (f, b, o) = timed_steps(call, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            assert model._live[0].weighted == (lw is not None)
            with torch.no_grad():
                losses[name] = float(call(batch))
            del opt
    best = {k: {m: min(v) for m, v in r.items()} for k, r in res.items()}
    spread = {k: round(max(r['step_ms']) - min(r['step_ms']), 3) for k, r in res.items()}
    over = {k: round(best[k]['step_ms'] - best['off']['step_ms'], 3) for k in arms if k != 'off'}
    print(json.dumps(dict(part='step', dim=512, depth=8, tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam', best=best, spread_ms=spread,
                          over_off_ms=over, inside_off_spread={k: bool(abs(v) <= spread['off']) for k, v in over.items()},
                          rounds_ms={k: v['step_ms'] for k, v in res.items()}, last_loss=losses)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--part', choices=('kernels', 'step', 'all'), default='all')
    a = ap.parse_args()
    if a.part in ('kernels', 'all'):
        kernels(a)
    if a.part in ('step', 'all'):
        step(a)


if __name__ == '__main__':
    main()
