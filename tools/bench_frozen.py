"""What freezing native parameters (`p.requires_grad_(False)`) saves on the training step: BASELINE config 2 (dim 512, depth 8, 64 x 1024 tokens of the
canonical sample), the whole step - forward, backward, clip + FusedAdam - with nothing frozen and with three frozen sets, timed in alternated rounds on
one model (the arms differ in `requires_grad` only, so they share weights, plans and the box's drift).  Per arm: ms per step, its forward / backward /
optimizer shares (HIP events around each), launches and weight-gradient products of the backward list, and where the list ends.  Information only
(profiles/frozen_params.txt); the unfrozen arm is the unchanged path.  Prints one JSON line.

    python tools/bench_frozen.py                     # five rounds of 10 steps
    python tools/bench_frozen.py --batch 16 --steps 5 --rounds 2
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's model and batch)
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

HEADS = ('model_to_latent_projs.', 'to_text_logits.weight')


def _layer(n):
    return int(n.split('.')[2]) if n.startswith('transformer.layers.') else None


def arms(depth):
    """name -> predicate "this native parameter trains" """
    return {
        'unfrozen': lambda n: True,
        'trunk_frozen_modality0_projs': lambda n: n.startswith(('latent_to_model_projs.0.', 'model_to_latent_projs.0.')),
        'top_half_and_heads': lambda n: n.startswith(HEADS) or n == 'transformer.norm.gamma' or (_layer(n) is not None and _layer(n) >= depth / 2),
        'heads_only': lambda n: n.startswith(HEADS),
    }


def set_arm(model, trains):
    for n, p in model.store.params.items():
        p.requires_grad_(bool(trains(n)))


def timed_steps(model, opt, batch, steps, warmup):
    def step(ev=None):
        if ev:
            ev[0].record()
        loss = model(batch)
        if ev:
            ev[1].record()
        loss.backward()
        if ev:
            ev[2].record()
        opt.step(); opt.zero_grad()
        if ev:
            ev[3].record()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
    for ev in evs:
        step(ev)
    torch.cuda.synchronize()
    total = evs[0][0].elapsed_time(evs[-1][3]) / steps
    parts = [sum(e[k].elapsed_time(e[k + 1]) for e in evs) / steps for k in range(3)]
    return total, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    cfg = bench.CONFIGS[2]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.make_batch(cfg['two'], a.batch, dev, gen)
    opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
    A = arms(cfg['depth'])
    res = {name: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[]) for name in A}
    lists = {}
    for _ in range(a.rounds):                               # alternated rounds: box drift hits every arm alike
        for name, trains in A.items():
            set_arm(model, trains)
            total, (f, b, o) = timed_steps(model, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            plan = model._live[0]
            tn = sum(1 for fn, _ in plan.bwd if fn == 'tfx_gemm_tn')
            lists[name] = dict(launches=len(plan.bwd), ends_at=plan.bwd_end, tn_launches=tn, trainable=sum(p.requires_grad for p in model.store.params.values()),
                               frozen_elements=sum(b - a_ for a_, b in model.store.frozen_ranges()), elements=model.store.numel)
    best = {name: {k: min(v) for k, v in r.items()} for name, r in res.items()}
    base = best['unfrozen']
    out = dict(config=2, dim=cfg['dim'], depth=cfg['depth'], tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam',
               best_ms=best, saved_ms={k: round(base['step_ms'] - v['step_ms'], 3) for k, v in best.items()},
               saved_bwd_ms={k: round(base['bwd_ms'] - v['bwd_ms'], 3) for k, v in best.items()},
               unfrozen_spread_ms=round(max(res['unfrozen']['step_ms']) - min(res['unfrozen']['step_ms']), 3), lists=lists, rounds_ms={k: v['step_ms'] for k, v in res.items()})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
