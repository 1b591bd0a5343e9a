"""Cost of LASER attention (Transformer(attn_laser=True)): training-step time with and without the flag on the same box, same model, same data,
the time of a greedy KV-cached `generate_text_only` run, and `sample_many` at config 5 (dim 1024 / depth 24 / dim_latent 384, 64 mixed prompts,
max_length 256, 16 ODE grid points, cfg 3, forced modality at the start: the workload of bench.py's sample_many line) with the flag on and off.
Random weights decode different sequences under the two settings: the tokens / modalities returned are reported beside the times.  Prints one JSON line.

    python tools/bench_laser.py                                  # dim 512, depth 8, 8 heads x 64, 64 x 1024 tokens (65 536 per step)
    python tools/bench_laser.py --dim 384 --batch 16 --steps 20
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transfusion_pytorch_amd import Transfusion            # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402


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


def gen_ms(model, prompt, length, reps=3):
    model.eval()
    with torch.no_grad():
        model.generate_text_only(prompt, length, temperature=0.)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            model.generate_text_only(prompt, length, temperature=0.)
        t1.record(); torch.cuda.synchronize()
    model.train()
    return t0.elapsed_time(t1) / reps


def sample_config5(laser, reps=1):
    torch.manual_seed(0)
    m = Transfusion(num_text_tokens=256, dim_latent=384, modality_default_shape=(4,),
                    transformer=dict(dim=1024, depth=24, attn_laser=laser)).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(1234)
    prompts = []
    for _ in range(16):                                   # the four README prompt kinds, 16 times each
        prompts += [torch.randint(0, 256, (16,), device='cuda', generator=g), (0, torch.randn(4, 384, device='cuda', generator=g)), None,
                    [torch.randint(0, 256, (8,), device='cuda', generator=g), (0, torch.randn(6, 384, device='cuda', generator=g))]]
    noise = torch.randn(16, 384, device='cuda', generator=g)
    kw = dict(max_length=256, modality_steps=16, cfg_scale=3., text_temperature=0., init_modality_noise=noise, fixed_modality_shape=(4,),
              force_modality_at_start=0)
    m.sample_many(prompts, **{**kw, 'max_length': 24})                   # warm-up (plans, shadows)
    times = []
    for _ in range(reps + 1):                                            # the first full call builds its plans; the repeat reuses them
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = m.sample_many(prompts, **kw)
        torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    ntok = sum(sum((p.numel() if not isinstance(p, tuple) else p[1].shape[0]) for p in s) for s in res)
    nmod = sum(sum(isinstance(p, tuple) for p in s) for s in res)
    del m
    torch.cuda.empty_cache()
    return dict(seconds=round(times[0], 3), seconds_repeat_call=round(min(times[1:]), 3), tokens_returned=ntok, modality_instances=nmod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=512); ap.add_argument('--depth', type=int, default=8)
    ap.add_argument('--heads', type=int, default=8); ap.add_argument('--batch', type=int, default=64); ap.add_argument('--seq', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10); ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--no-sample', action='store_true', help='skip the config-5 sample_many timing')
    a = ap.parse_args()
    torch.manual_seed(0)
    batch = torch.randint(0, 256, (a.batch, a.seq + 1), device='cuda')
    prompt = batch[:8, :64].clone()
    models = {}
    for laser in (False, True):
        torch.manual_seed(0)
        m = Transfusion(num_text_tokens=256, transformer=dict(dim=a.dim, depth=a.depth, dim_head=64, heads=a.heads, attn_laser=laser)).cuda().train()
        models[laser] = (m, FusedAdam(m, lr=1e-4, max_grad_norm=0.5))
    res = {False: [], True: []}
    for _ in range(a.rounds):                         # interleaved rounds: box drift hits both arms alike
        for laser in (False, True):
            res[laser].append(step_ms(*models[laser], batch, a.steps, a.warmup))
    plain, laser = min(res[False]), min(res[True])
    g_plain, g_laser = gen_ms(models[False][0], prompt, 64 + 192), gen_ms(models[True][0], prompt, 64 + 192)
    del models
    torch.cuda.empty_cache()
    samp = None if a.no_sample else {'plain': sample_config5(False), 'laser': sample_config5(True)}
    print(json.dumps(dict(sample_many_config5=samp, dim=a.dim, depth=a.depth, heads=a.heads, tokens_per_step=a.batch * a.seq, plain_step_ms=round(plain, 3),
                          laser_step_ms=round(laser, 3), laser_over_plain=round(laser / plain, 4), rounds_ms=res,
                          generate_text_only_ms=dict(plain=round(g_plain, 2), laser=round(g_laser, 2), batch=8, prompt=64, new_tokens=192))))


if __name__ == '__main__':
    main()
