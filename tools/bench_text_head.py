"""What chunking the text head (`model.set_text_head_chunking_(rows)`) costs and saves: BASELINE config 2 geometry (dim 512, depth 8, 64 x 1024 tokens of the
canonical sample) at `num_text_tokens` 256 and 32 000, the whole step - forward, backward, clip + FusedAdam - plain against `rows` 4096 and 16384, timed in
alternated rounds on one model (the arms differ in the switch only, so they share weights and the box's drift).  Per arm: ms per step and its forward / backward /
optimizer shares (HIP events around each), `torch.cuda.max_memory_allocated` of a process that holds this arm's plan alone (the plan cache is emptied and the peak
counter reset in front of every arm), the plan's own bytes and launch counts.  Next to them what the switch is expected to cost: one more logits product
(2 T vp dim flop, timed alone) and one more read of the fp32 chunk (4 T vp bytes at the achieved rate of tfx_ce_bwd, timed alone).  Before the timing, one step of
each arm from the same seed: the relative difference of the gradient buffers.  Information only (profiles/text_head_chunking.txt).  One JSON line per vocabulary.

    python tools/bench_text_head.py                          # both vocabularies, five rounds of 10 steps
    python tools/bench_text_head.py --vocab 32000 --batch 16 --steps 5 --rounds 2
"""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's batch)
from bench_frozen import timed_steps                        # noqa: E402
from transfusion_pytorch_amd import Transfusion            # noqa: E402
from transfusion_pytorch_amd.engine import Plan            # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

ARMS = {'plain': None, 'rows_4096': 4096, 'rows_16384': 16384}


def drop_plans(model):
    model._plans.clear(); model._live = None
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def gradient_difference(model, batch):
    """one forward + backward per arm from the same seed (same times, same noise): loss and rel-Frobenius difference of the flat gradient buffer against plain"""
    out, ref = {}, None
    for name, rows in ARMS.items():
        model.set_text_head_chunking_(rows)
        drop_plans(model)
        model.store.grad.zero_()
        torch.manual_seed(1234)
        loss = model(batch)
        loss.backward()
        torch.cuda.synchronize()
        g = model.store.grad.double().clone()
        ref = g if ref is None else ref
        out[name] = dict(loss=float(loss.detach()), grad_rel=float((g - ref).norm() / ref.norm()))
        for p in model.parameters():
            p.grad = None
    return out


def time_range(lst, lo, hi, reps=5):
    """ms of launches [lo, hi) of a list on the current stream, best of `reps`"""
    stream = torch.cuda.current_stream().cuda_stream
    best = float('inf')
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); Plan.run(lst, stream, lo, hi); b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def head_cost(plan):
    """a chunked plan's head, launch family by launch family (each launch timed alone, summed over the chunks): what the backward adds to a plain step is the
    second logits product and tfx_ce_bwd's read of the fp32 chunk"""
    names = [fn if isinstance(fn, str) else fn.__name__ for fn, _ in plan.bwd]
    n = len(plan._chunks())
    per = 4 if 'tfx_gemm_tn' in names[:4] else 3
    assert names[1] == 'tfx_ce_bwd'
    t = dict(logits_product_ms=0., ce_bwd_ms=0., ce_fwd_ms=0.)
    for k in range(n):
        t['logits_product_ms'] += time_range(plan.bwd, per * k, per * k + 1)
        t['ce_bwd_ms'] += time_range(plan.bwd, per * k + 1, per * k + 2)
        t['ce_fwd_ms'] += time_range(plan.fwd, plan.fwd_embed_end + 2 * k + 1, plan.fwd_embed_end + 2 * k + 2)
    T, vp = plan.T, plan.md.vp
    t = {k: round(v, 3) for k, v in t.items()}
    t['ce_bwd_tb_s'] = round(T * vp * 6 / (t['ce_bwd_ms'] * 1e-3) / 1e12, 3)
    t['ce_fwd_tb_s'] = round(T * vp * 4 / (t['ce_fwd_ms'] * 1e-3) / 1e12, 3)
    # one more product + one more read of the fp32 chunk (4 of tfx_ce_bwd's 6 bytes per logit)
    t['expected_extra_ms'] = round(t['logits_product_ms'] + t['ce_bwd_ms'] * 4 / 6, 3)
    return t


def run(vocab, a):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=vocab, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=512, depth=8)).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.canonical_batch(a.batch, dev, gen, num_text_tokens=vocab)
    check = gradient_difference(model, batch)
    res = {name: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[], peak_gib=[]) for name in ARMS}
    info = {}
    for _ in range(a.rounds):                               # alternated rounds: box drift hits every arm alike
        for name, rows in ARMS.items():
            model.set_text_head_chunking_(rows)
            drop_plans(model)
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
            total, (f, b, o) = timed_steps(model, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            r['peak_gib'].append(round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
            plan = model._live[0]
            if name not in info:
                info[name] = dict(plan_gib=round(plan.nbytes / 2 ** 30, 3), chunks=len(plan._chunks()) if plan.chunk else 0, fwd_launches=len(plan.fwd),
                                  bwd_launches=len(plan.bwd), vp=plan.md.vp, T=plan.T)
                if plan.chunk:
                    info[name]['head'] = head_cost(plan)
            del opt, plan
    best = {name: {k: (max(v) if k == 'peak_gib' else min(v)) for k, v in r.items()} for name, r in res.items()}
    spread = {name: round(max(r['step_ms']) - min(r['step_ms']), 3) for name, r in res.items()}
    cost = {}
    for name in ARMS:
        if name != 'plain':
            extra = best[name]['step_ms'] - best['plain']['step_ms']
            cost[name] = dict(extra_ms=round(extra, 3), step_ratio=round(best[name]['step_ms'] / best['plain']['step_ms'], 4),
                              bwd_ratio=round(best[name]['bwd_ms'] / best['plain']['bwd_ms'], 4),
                              measured_over_expected=round(extra / info[name]['head']['expected_extra_ms'], 3),
                              peak_saved_gib=round(best['plain']['peak_gib'] - best[name]['peak_gib'], 3))
    out = dict(num_text_tokens=vocab, dim=512, depth=8, tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam',
               same_seed_step=check, best=best, spread_ms=spread, cost=cost, plans=info, rounds_ms={k: v['step_ms'] for k, v in res.items()})
    print(json.dumps(out), flush=True)
    del model
    gc.collect(); torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vocab', type=int, default=0, help='0: 256 and 32000')
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    for vocab in ((256, 32000) if a.vocab == 0 else (a.vocab,)):
        run(vocab, a)


if __name__ == '__main__':
    main()
