"""Cost of the Adam-atan2 rule against the fused Adam launch on one MI355X.  Prints one JSON line.

  launch     on the flat buffers of BASELINE config 2 (dim 512 / depth 8) and config 3 (dim 1024 / depth 24), the optimizer launch alone:
               adam_ungrouped     `tfx_adam_step`, the launch FusedAdam makes by default - the yardstick, in the same run
               atan2_ungrouped    `tfx_adam_atan2_step` without a range table
               atan2_decay_groups `tfx_adam_atan2_step` with the range table of `optim.decay_groups(model, 0.1)` (2 groups, decoupled decay)
             device events around `--steps` back-to-back launches, `--rounds` rounds, the arms alternated inside every round, after a warm-up;
             traffic 28 bytes per element (p, g, m, v read; p, m, v written).  `spread_of_adam` is (max - min) / mean of the yardstick's rounds: an
             atan2 arm whose ratio to the yardstick lies inside it is not measurably slower.
  step       the whole training step (pack + forward + backward + clip + optimizer) at config 2, FusedAdam against FusedAdamAtan2 on two models of
             the same seed, `--rounds` alternated rounds of `--train-steps` steps, a batch of its own for every step.

    python tools/bench_adam_atan2.py > profiles/adam_atan2_bench.txt
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the BASELINE configs' model builder)
from transfusion_pytorch_amd import capi                     # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam, FusedAdamAtan2, decay_groups   # noqa: E402


def launches(model):
    """arm name -> (closure that enqueues one launch, number of ranges)"""
    ps = model.store
    gen = torch.Generator(device=ps.flat.device).manual_seed(0)
    ps.grad.normal_(generator=gen).mul_(0.01)
    m, v = torch.zeros_like(ps.flat), torch.zeros_like(ps.flat)
    sumsq = (ps.grad.double() ** 2).sum().float().reshape(1)
    stream = torch.cuda.current_stream().cuda_stream
    common = dict(p=ps.flat, g=ps.grad, m=m, v=v, n=ps.numel, lr=3e-4, beta1=0.9, weight_decay=0., max_norm=0.5, grad_scale=1., step=10, sumsq=sumsq)
    keep = [m, v, sumsq]
    plain = capi.make_args('tfx_adam_args', beta2=0.999, eps=1e-8, **common)
    atan2 = capi.make_args('tfx_adam_atan2_args', beta2=0.99, atan2_a=1.27, atan2_b=1., **common)
    opt = FusedAdamAtan2(model, lr=3e-4, param_groups=decay_groups(model, 0.1))
    ranges, nrange = opt._range_table(ps)
    grouped = capi.make_args('tfx_adam_atan2_args', beta2=0.99, atan2_a=1.27, atan2_b=1., **opt._group_table(ps, opt.param_groups), **common)
    keep += [ranges, plain, atan2, grouped]
    arms = {'adam_ungrouped': (lambda: capi.call('tfx_adam_step', plain, stream), 0),
            'atan2_ungrouped': (lambda: capi.call('tfx_adam_atan2_step', atan2, stream), 0),
            'atan2_decay_groups': (lambda: capi.call('tfx_adam_atan2_step', grouped, stream), nrange)}
    return arms, keep


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def bench_launch(c, dev, a):
    cfg = bench.CONFIGS[c]
    torch.manual_seed(0)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    arms, keep = launches(model)
    for fn, _ in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):                                # interleaved rounds: drift of the machine hits every arm alike
        for k, (fn, _) in arms.items():
            ms[k].append(timed(fn, a.steps))
    n = model.store.numel
    res = {k: dict(ranges=arms[k][1], mean_us=round(1e3 * sum(t) / len(t), 1), min_us=round(1e3 * min(t), 1), max_us=round(1e3 * max(t), 1),
                   gb_per_s=round(28 * n / (sum(t) / len(t)) / 1e6, 1)) for k, t in ms.items()}
    yard = res['adam_ungrouped']
    for k in res:
        res[k]['ratio_to_adam_ungrouped'] = round(res[k]['mean_us'] / yard['mean_us'], 4)
    return dict(elements=n, spread_of_adam=round((yard['max_us'] - yard['min_us']) / yard['mean_us'], 4), **res)


def bench_step(c, dev, a):
    cfg = bench.CONFIGS[c]
    gen = torch.Generator(device=dev).manual_seed(1234)
    batches = [bench.make_batch(cfg['two'], a.batch, dev, gen) for _ in range(a.train_steps)]      # a batch of its own for every step of a round
    arms = {}
    for name, cls in (('fused_adam', FusedAdam), ('fused_adam_atan2', FusedAdamAtan2)):
        torch.manual_seed(0)
        model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
        arms[name] = (model, cls(model, lr=3e-4, max_grad_norm=0.5))

    def run(model, opt, n):
        for k in range(n):
            loss = model(batches[k]); loss.backward(); opt.step(); opt.zero_grad()
        return loss

    for model, opt in arms.values():
        run(model, opt, min(a.warmup, a.train_steps))
    ms, last = {k: [] for k in arms}, {}
    for _ in range(a.rounds):
        for k, (model, opt) in arms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            last[k] = run(model, opt, a.train_steps)
            torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / a.train_steps * 1e3)
    res = {k: dict(mean_ms=round(sum(t) / len(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), loss=round(float(last[k].detach()), 4)) for k, t in ms.items()}
    res['fused_adam_atan2']['ratio_to_fused_adam'] = round(res['fused_adam_atan2']['mean_ms'] / res['fused_adam']['mean_ms'], 4)
    return dict(batch=a.batch, steps_per_round=a.train_steps, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20); ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--train-steps', type=int, default=8); ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    for c in (2, 3):
        out[f'launch_config{c}'] = bench_launch(c, dev, a)
        torch.cuda.empty_cache()
    out['step_config2'] = bench_step(2, dev, a)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
