"""What activation checkpointing (`model.set_activation_checkpointing_()`) costs and saves: BASELINE configs 2 (dim 512, depth 8) and 3 (dim 1024, depth 24),
64 x 1024 tokens of the canonical sample, the whole step - forward, backward, clip + FusedAdam - plain against checkpointed, timed in alternated rounds on
one model (the arms differ in the switch only, so they share weights and the box's drift).  A second pair of arms is the user this is for: the trunk
frozen with rank-16 LoRA adapters on the attention targets.  Per arm: ms per step and its forward / backward / optimizer shares (HIP events around each),
`torch.cuda.max_memory_allocated` of a process that holds this arm's plan alone (the plan cache is emptied and the peak counter reset in front of every
arm), the plan's own bytes and its launch counts.  Before the timing, one step of each arm from the same seed: the relative difference of the two
gradient buffers.  Information only (profiles/activation_checkpointing.txt).  Prints one JSON line per config.

    python tools/bench_checkpointing.py                      # configs 2 and 3, five rounds of 10 steps
    python tools/bench_checkpointing.py --config 2 --batch 16 --steps 5 --rounds 2
"""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's model and batch)
from bench_frozen import set_arm, timed_steps               # noqa: E402
from transfusion_pytorch_amd import add_lora_, remove_lora_            # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

ATTN = ('to_qk', 'to_v', 'to_out')
ARMS = {'plain': (False, False), 'checkpointed': (True, False), 'lora_attn_r16_plain': (False, True), 'lora_attn_r16_checkpointed': (True, True)}      # name -> (switch, LoRA arm)


def drop_plans(model):
    model._plans.clear(); model._live = None
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def gradient_difference(model, batch):
    """one forward + backward per setting from the same seed (same times, same noise): rel-Frobenius difference of the flat gradient buffers"""
    grads = []
    for on in (False, True):
        model.set_activation_checkpointing_(on)
        drop_plans(model)
        model.store.grad.zero_()
        torch.manual_seed(1234)
        loss = model(batch)
        loss.backward()
        torch.cuda.synchronize()
        grads.append((float(loss.detach()), model.store.grad.double().clone()))
        for p in model.parameters():
            p.grad = None
    (l0, g0), (l1, g1) = grads
    return dict(loss_plain=l0, loss_checkpointed=l1, grad_rel=float((g1 - g0).norm() / g0.norm()))


def run(config, a):
    cfg = bench.CONFIGS[config]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.make_batch(cfg['two'], a.batch, dev, gen)
    check = gradient_difference(model, batch)
    res = {name: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[], peak_gib=[]) for name in ARMS}
    info = {}
    for _ in range(a.rounds):                               # alternated rounds: box drift hits every arm alike
        for name, (on, lora) in ARMS.items():
            if lora:
                set_arm(model, lambda n: n.startswith(('latent_to_model_projs.0.', 'model_to_latent_projs.0.')))
                add_lora_(model, rank=16, targets=ATTN)
            else:
                set_arm(model, lambda n: True)
            model.set_activation_checkpointing_(on)
            drop_plans(model)
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)           # (per arm: the adapters are external parameters of THIS optimizer)
            total, (f, b, o) = timed_steps(model, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            r['peak_gib'].append(round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
            plan = model._live[0]
            info[name] = dict(plan_gib=round(plan.nbytes / 2 ** 30, 3), n_slots=plan.n_slots, fwd_launches=len(plan.fwd), bwd_launches=len(plan.bwd),
                              recomputed_layers=len(plan._recompute), recompute_launches=sum(hi - lo for lo, hi in plan._recompute.values()), ends_at=plan.bwd_end)
            if lora:
                remove_lora_(model)
            del opt, plan
    best = {name: {k: (max(v) if k == 'peak_gib' else min(v)) for k, v in r.items()} for name, r in res.items()}
    spread = {name: round(max(r['step_ms']) - min(r['step_ms']), 3) for name, r in res.items()}
    out = dict(config=config, dim=cfg['dim'], depth=cfg['depth'], tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam',
               same_seed_step=check, best=best, spread_ms=spread, plans=info, rounds_ms={k: v['step_ms'] for k, v in res.items()})
    print(json.dumps(out), flush=True)
    del model
    gc.collect(); torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=0, choices=(0, 2, 3), help='0: both')
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for config in ((2, 3) if a.config == 0 else (a.config,)):
        run(config, a)


if __name__ == '__main__':
    main()
