"""What LoRA adapters (transfusion_pytorch_amd/lora.py) cost on the training step: BASELINE config 2 (dim 512, depth 8) or 3 (dim 1024, depth 24), 64 x 1024
tokens of the canonical sample, the whole step - forward, backward, clip + FusedAdam - in four arms timed in alternated rounds on one model:

    unfrozen                        everything trains, no adapters: the unchanged path
    trunk_frozen_modality0_projs    the frozen-parameter arm of tools/bench_frozen.py (the data gradient still runs to x_0)
    lora_attn_r16                   base frozen, rank 16 on to_qk / to_v / to_out of every layer
    lora_all_r16                    base frozen, rank 16 on all five targets of every layer

Per arm: ms per step and its forward / backward / optimizer shares (HIP events), the backward list's launches; for the adapter arms also the bytes
tfx_lora_down and tfx_lora_grad move, from their arguments, against reading every adapted matrix's X and dY once.  Information only
(profiles/lora_bench.txt); no target.  Prints one JSON line.

    python tools/bench_lora.py                       # config 2, five rounds of 10 steps
    python tools/bench_lora.py --config 3 --steps 5 --rounds 3
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's model and batch)
from bench_frozen import set_arm, timed_steps               # noqa: E402
from transfusion_pytorch_amd import add_lora_, remove_lora_            # noqa: E402
from transfusion_pytorch_amd import capi                    # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

ATTN = ('to_qk', 'to_v', 'to_out')
ARMS = {'unfrozen': None, 'trunk_frozen_modality0_projs': None, 'lora_attn_r16': ATTN, 'lora_all_r16': ATTN + ('net.0', 'net.3')}


def adapter_traffic(plan):
    """bytes the adapter launches of the backward list move (operands in, results out, the partial sums written and read back), and the bytes of reading
    each adapter's X and dY once (every operand is the Q of exactly one down projection)"""
    import ctypes
    down = grad = once = 0
    for fn, a in plan.bwd:
        if fn == 'tfx_lora_down':
            down += a.M * a.K * 2 + a.r_pad * a.K * 2 + a.M * a.r_pad * 2
            once += a.M * a.K * 2
        elif fn == 'tfx_lora_grad':
            fl = ctypes.c_int64(0)
            capi.check(capi.lib().tfx_lora_grad_plan(ctypes.byref(a), None, None, ctypes.byref(fl)), 'tfx_lora_grad_plan')
            grad += a.M * a.K * 2 + a.M * a.r_pad * 2 + 2 * fl.value * 4 + 2 * a.r * a.K * 4
    return dict(lora_down_bytes=down, lora_grad_bytes=grad, x_and_dy_once_bytes=once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=2, choices=(2, 3))
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    cfg = bench.CONFIGS[a.config]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.make_batch(cfg['two'], a.batch, dev, gen)
    res = {name: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[]) for name in ARMS}
    lists = {}
    for _ in range(a.rounds):                               # alternated rounds: box drift hits every arm alike
        for name, targets in ARMS.items():
            if targets is None:
                set_arm(model, (lambda n: True) if name == 'unfrozen' else (lambda n: n.startswith(('latent_to_model_projs.0.', 'model_to_latent_projs.0.'))))
            else:
                add_lora_(model, rank=16, targets=targets)  # (B = 0: the same forward as the other arms; the cost does not depend on the values)
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)           # (per arm: the adapters are external parameters of THIS optimizer)
            total, (f, b, o) = timed_steps(model, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            plan = model._live[0]
            lists[name] = dict(launches=len(plan.bwd), ends_at=plan.bwd_end, tn_launches=sum(1 for fn, _ in plan.bwd if fn == 'tfx_gemm_tn'),
                               lora_launches=sum(1 for fn, _ in plan.bwd if isinstance(fn, str) and fn.startswith('tfx_lora')),
                               trainable_native=sum(p.requires_grad for p in model.store.params.values()),
                               adapter_elements=sum(p.numel() for p in model.external_parameters()))
            if targets is not None:
                lists[name].update(adapter_traffic(plan))
                remove_lora_(model)
            del opt
    best = {name: {k: min(v) for k, v in r.items()} for name, r in res.items()}
    out = dict(config=a.config, dim=cfg['dim'], depth=cfg['depth'], tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam',
               best_ms=best, unfrozen_spread_ms=round(max(res['unfrozen']['step_ms']) - min(res['unfrozen']['step_ms']), 3), lists=lists,
               rounds_ms={k: v['step_ms'] for k, v in res.items()})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
