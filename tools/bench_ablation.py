"""Cost of the two attention ablations - Transformer(qk_rmsnorm=False) and Transformer(attn_kwargs=dict(gate_values=False)) - on the training step:
the same box, the same data, four models of config 2's dimensions (default, each switch, both), timed in interleaved rounds.  Information only
(profiles/ablation_switches.txt); the default arm is the unchanged path.  Prints one JSON line.

    python tools/bench_ablation.py                               # dim 512, depth 8, 8 heads x 64, 64 x 1024 tokens (65 536 per step)
    python tools/bench_ablation.py --dim 384 --batch 16 --steps 20
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transfusion_pytorch_amd import Transfusion            # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

ARMS = {'default': {}, 'qk_rmsnorm=False': dict(qk_rmsnorm=False), 'gate_values=False': dict(attn_kwargs=dict(gate_values=False)),
        'both': dict(qk_rmsnorm=False, attn_kwargs=dict(gate_values=False))}


def step_ms(model, opt, batch, steps, warmup):
    for _ in range(warmup):
        model.forward_text(batch).backward(); opt.step(); opt.zero_grad()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        model.forward_text(batch).backward(); opt.step(); opt.zero_grad()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=512); ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--heads', type=int, default=8); ap.add_argument('--batch', type=int, default=64); ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10); ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    batch = torch.randint(0, 256, (a.batch, a.seq + 1), device='cuda')
    models = {}
    for name, sw in ARMS.items():
        torch.manual_seed(0)
        m = Transfusion(num_text_tokens=256, transformer=dict(dim=a.dim, depth=a.depth, dim_head=64, heads=a.heads, **sw)).cuda().train()
        models[name] = (m, FusedAdam(m, lr=1e-4, max_grad_norm=0.5))
    res = {name: [] for name in ARMS}
    for _ in range(a.rounds):                         # interleaved rounds: box drift hits every arm alike
        for name in ARMS:
            res[name].append(round(step_ms(*models[name], batch, a.steps, a.warmup), 3))
    best = {name: min(v) for name, v in res.items()}
    print(json.dumps(dict(dim=a.dim, depth=a.depth, heads=a.heads, tokens_per_step=a.batch * a.seq, workload='forward_text + backward + FusedAdam',
                          step_ms=best, over_default={k: round(v / best['default'], 4) for k, v in best.items()}, rounds_ms=res)))


if __name__ == '__main__':
    main()
