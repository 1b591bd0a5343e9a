"""Time and memory of a SelfMaskedRepTraining step against the plain step (BASELINE config 2: dim 512 / depth 8, 64 x 1024 tokens).

    python tools/bench_selfflow.py [--rounds 5] [--steps 6] [--batch 64] [--out profiles/selfflow_bench.txt]
    python tools/bench_selfflow.py --trace-steps 3          # nothing but wrapper steps, for `rocprofv3 --kernel-trace --stats -- python ...`

Three loops, alternated round by round, fresh batch per step, device-synchronised, after a warm-up:
  (a) the plain training step                     loss = model(batch); loss.backward(); FusedAdam step
  (b) a no-grad forward of the same batch         model(batch) under torch.no_grad()
  (c) the wrapper step (student_layer -3, teacher_layer -1)   total, _ = wrapper(batch); total.backward(); FusedAdam(wrapper) step; update_teacher()
(c) - (a) - (b) is what the prediction head and the loss cost.  Peak memory (torch.cuda.max_memory_allocated) is taken per loop kind in a fresh phase.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench                                                                   # noqa: E402
from transfusion_pytorch_amd import SelfMaskedRepTraining                       # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--trace-steps', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    cfg = bench.CONFIGS[2]
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    state = {'opt': FusedAdam(model, lr=3e-4, max_grad_norm=0.5)}      # ONE optimizer at a time: the wrapper's replaces it (and then steps the plain loop too)
    batch_of = lambda: bench.make_batch(cfg['two'], a.batch, dev, gen)

    def plain(batch):
        loss = model(batch)
        loss.backward()
        state['opt'].step(); state['opt'].zero_grad()

    def nograd(batch):
        with torch.no_grad():
            model(batch)

    def wrapped(batch):
        if 'w' not in state:
            state['w'] = SelfMaskedRepTraining(model, use_asymmetric_dropout=False, rep_loss_weight=0.1, student_layer=-3, teacher_layer=-1).cuda().train()
            state['opt'] = FusedAdam(state['w'], lr=3e-4, max_grad_norm=0.5)
        total, _ = state['w'](batch)
        total.backward()
        state['opt'].step(); state['opt'].zero_grad()
        state['w'].update_teacher()

    def timed(fn, n):
        batches = [batch_of() for _ in range(n)]                     # a fresh batch per step, drawn outside the timed region
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            fn(b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    if a.trace_steps:
        for _ in range(a.trace_steps):
            wrapped(batch_of())
        torch.cuda.synchronize()
        return

    lines = [f'config 2 (dim {cfg["dim"]} depth {cfg["depth"]}), batch {a.batch} x 1024 tokens, {a.rounds} alternated rounds of {a.steps} steps, warm-up {a.warmup}']
    peak = {}
    for name, fn in (('plain', plain), ('wrapper', wrapped)):       # memory first, each kind from a clean high-water mark (the plans stay cached)
        for _ in range(a.warmup):
            fn(batch_of())
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        fn(batch_of()); torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() / 2 ** 30
    for _ in range(a.warmup):
        nograd(batch_of())
    ms = {'plain': [], 'nograd': [], 'wrapper': []}
    for r in range(a.rounds):
        for name, fn in (('plain', plain), ('nograd', nograd), ('wrapper', wrapped)):
            ms[name].append(timed(fn, a.steps))
    for name, label in (('plain', '(a) plain training step'), ('nograd', '(b) no-grad forward'), ('wrapper', '(c) wrapper step')):
        v = ms[name]
        lines.append(f'{label:28s} median {statistics.median(v):8.3f} ms   min {min(v):8.3f}   max {max(v):8.3f}   rounds {" ".join(f"{x:.3f}" for x in v)}')
    rest = statistics.median(ms['wrapper']) - statistics.median(ms['plain']) - statistics.median(ms['nograd'])
    lines.append(f'(c) - (a) - (b) = {rest:.3f} ms per step: the prediction head, the cosine loss, the teacher update')
    lines.append(f'peak memory: (a) {peak["plain"]:.2f} GiB   (c) {peak["wrapper"]:.2f} GiB (student plan + head buffers + the EMA copy and its hiddens-only plan, all resident)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
