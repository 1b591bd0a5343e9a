"""Cost of optim.FusedMuon on one MI355X, at BASELINE config 2 (dim 512 / depth 8) and config 3 (dim 1024 / depth 24).  Prints one JSON line.

  optimizer step alone   `FusedMuon.step()` against the reference on the same box: `torch.optim.Muon` over the same matrices (a Python loop, 15 vendor
                         GEMMs per matrix and step) + `FusedAdam.step()`.  Same gradients (one real backward, kept), variants alternated in one process
                         after warm-up, device events around `--rounds` x `--steps` steps each.
  whole training step    forward + backward + `step()` with FusedMuon against FusedAdam (config 2, batch 64), alternated the same way.
  work                   4 m^2 n + 2 m^3 flop per matrix and Newton-Schulz iteration (m <= n: gram 2 m^2 n, polynomial 2 m^3, update 2 m^2 n).

    python tools/bench_muon.py                                   # both configs
    python tools/bench_muon.py --config 2 --opt-only --steps 20  # only FusedMuon.step(): the process to put under a kernel trace
                                                                 #   (rocprofv3 --kernel-trace --stats -- python tools/bench_muon.py --config 2 --opt-only)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the BASELINE configs' model / batch builders)
from transfusion_pytorch_amd.optim import FusedAdam, FusedMuon   # noqa: E402


def ns_flop_per_iteration(model):
    tot = 0
    for p in model.muon_parameters():
        m, n = sorted(p.shape)
        tot += 4 * m * m * n + 2 * m ** 3
    return tot


def model_with_gradient(c, dev, batch=8):
    cfg = bench.CONFIGS[c]
    torch.manual_seed(0)
    m = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    gen = torch.Generator(device=dev).manual_seed(1234)
    m(bench.make_batch(cfg['two'], batch, dev, gen)).backward()
    torch.cuda.synchronize()
    return m


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def alternate(variants, steps, rounds, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):                                  # interleaved rounds: box drift hits every arm alike
        for k, fn in variants.items():
            res[k].append(timed(fn, steps))
    return res


def summary(ms):
    return dict(mean_ms=round(sum(ms) / len(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), rounds_ms=[round(x, 4) for x in ms])


def optimizer_alone(c, dev, steps, rounds, warmup):
    native, ref = model_with_gradient(c, dev), model_with_gradient(c, dev)
    on = FusedMuon(native, lr=3e-4, max_grad_norm=0.5)
    oa = FusedAdam(ref, lr=3e-4, max_grad_norm=0.5)
    tm = torch.optim.Muon(ref.muon_parameters())

    def reference():
        tm.step(); oa.step()
    res = alternate({'native': on.step, 'reference': reference}, steps, rounds, warmup)
    gf = ns_flop_per_iteration(native) * on.ns_steps / 1e9
    out = dict(matrices=len(on.muon_params), launches_per_step=on.launches_per_step(), ns_gflop_per_step=round(gf, 2),
               ns_gflop_per_layer_iteration=round(ns_flop_per_iteration(native) / native.md.depth / 1e9, 3),
               fused_muon_step=summary(res['native']), torch_muon_plus_fused_adam_step=summary(res['reference']))
    out['native_over_reference'] = round(out['fused_muon_step']['mean_ms'] / out['torch_muon_plus_fused_adam_step']['mean_ms'], 4)
    out['ns_tflops_if_whole_step_were_products'] = round(gf / out['fused_muon_step']['mean_ms'], 1)     # a lower bound of the product kernels' rate
    del native, ref, on, oa, tm
    torch.cuda.empty_cache()
    return out


def training_step(c, dev, steps, rounds, warmup, batch=64):
    cfg = bench.CONFIGS[c]
    arms = {}
    gen = torch.Generator(device=dev).manual_seed(1234)
    batches = [bench.make_batch(cfg['two'], batch, dev, gen) for _ in range(2)]
    for name, cls in (('fused_adam', FusedAdam), ('fused_muon', FusedMuon)):
        torch.manual_seed(0)
        m = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
        opt = cls(m, lr=3e-4, max_grad_norm=0.5)
        k = [0]

        def step(m=m, opt=opt, k=k):
            m(batches[k[0] % 2]).backward(); opt.step(); opt.zero_grad(); k[0] += 1
        arms[name] = step
    res = alternate(arms, steps, rounds, warmup)
    out = dict(batch=batch, fused_adam=summary(res['fused_adam']), fused_muon=summary(res['fused_muon']))
    out['muon_over_adam'] = round(out['fused_muon']['mean_ms'] / out['fused_adam']['mean_ms'], 4)
    del arms
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=0, help='2 or 3 (default: both)')
    ap.add_argument('--steps', type=int, default=10); ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--opt-only', action='store_true', help='run FusedMuon.step() --steps times and nothing else (for a kernel trace)')
    ap.add_argument('--no-train', action='store_true', help='skip the whole-training-step comparison')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    configs = [a.config] if a.config else [2, 3]
    if a.opt_only:
        for c in configs:
            m = model_with_gradient(c, dev)
            opt = FusedMuon(m, lr=3e-4, max_grad_norm=0.5)
            ms = timed(opt.step, a.steps)
            print(json.dumps(dict(config=c, steps=a.steps, fused_muon_step_ms=round(ms, 4), launches_per_step=opt.launches_per_step(),
                                  ns_gflop_per_step=round(ns_flop_per_iteration(m) * opt.ns_steps / 1e9, 2))))
        return
    out = {}
    for c in configs:
        out[f'config{c}'] = dict(optimizer_step=optimizer_alone(c, dev, a.steps, a.rounds, a.warmup))
        if c == 2 and not a.no_train:
            out[f'config{c}']['training_step'] = training_step(c, dev, a.steps, a.rounds, a.warmup)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
