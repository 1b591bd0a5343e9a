"""Cost of the optimizer launch over the flat buffer on one MI355X: parameter groups and the Adam-atan2 rule against the launch FusedAdam makes by
default, optionally against a second build.  Prints one JSON line.

  launch     on the flat buffers of BASELINE config 2 (dim 512 / depth 8) and config 3 (dim 1024 / depth 24), the optimizer launch alone:
               adam_ungrouped      `tfx_adam_step`, the launch FusedAdam makes by default - the yardstick, in the same run
               adam_decay_groups   `tfx_adam_step_groups` with the range table of `optim.decay_groups(model, 0.1)` (2 groups, decoupled decay)
               adam_layers8        the same entry point with 8 groups cut at layer boundaries
               atan2_ungrouped     `tfx_adam_atan2_step` without a range table
               atan2_decay_groups  `tfx_adam_atan2_step` with the range table of `decay_groups`
             device events around `--steps` back-to-back launches, `--rounds` rounds, the arms alternated inside every round, after a warm-up;
             traffic 28 bytes per element (p, g, m, v read; p, m, v written).  `spread_of_adam` is (max - min) / mean of the yardstick's rounds: an
             arm whose ratio to the yardstick lies inside it is not measurably slower.
  --parent-lib PATH   a second libtfx_hip.so (e.g. the build of the commit before) on a handle of its own.  Before any timing every arm is launched
             once on both libraries from identical copies of p, m, v: `same_bits` is byte equality of all three.  Then both libraries run every
             arm, alternated inside each round: `ratio_to_parent`, and `parent_spread`, (max - min) / mean of the parent's own rounds.
  --step     also the whole training step (pack + forward + backward + clip + optimizer) at config 2, FusedAdam against FusedAdamAtan2 on two models
             of the same seed, `--rounds` alternated rounds of `--train-steps` steps, a batch of its own for every step.

    python tools/bench_optim_launch.py --parent-lib /path/to/libtfx_hip.so
"""
import argparse
import ctypes
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


def layer_groups(model, groups=8):
    """`groups` parameter groups cut at layer boundaries (what is no layer's rides in the first), each with a learning rate of its own"""
    depth = model.md.depth
    out = [dict(params=[], lr=3e-4 * (1 + k)) for k in range(groups)]
    for n, p in model.store.params.items():
        parts = n.split('.')
        layer = int(parts[2]) if n.startswith('transformer.layers.') else 0
        out[layer * groups // depth]['params'].append(p)
    return out


def launches(model):
    """arm name -> (entry point, args, number of ranges); the buffers p, m, v the launches write; what must stay alive"""
    ps = model.store
    gen = torch.Generator(device=ps.flat.device).manual_seed(0)
    ps.grad.normal_(generator=gen).mul_(0.01)
    m, v = torch.zeros_like(ps.flat), torch.zeros_like(ps.flat)
    sumsq = (ps.grad.double() ** 2).sum().float().reshape(1)
    common = dict(p=ps.flat, g=ps.grad, m=m, v=v, n=ps.numel, lr=3e-4, beta1=0.9, weight_decay=0., max_norm=0.5, grad_scale=1., step=10, sumsq=sumsq)
    adam, atan2 = dict(beta2=0.999, eps=1e-8, **common), dict(beta2=0.99, atan2_a=1.27, atan2_b=1., **common)
    arms = {'adam_ungrouped': ('tfx_adam_step', capi.make_args('tfx_adam_args', **adam), 0)}
    keep = [sumsq]
    for name, opt in (('adam_decay_groups', FusedAdam(model, param_groups=decay_groups(model, 0.1))),
                      ('adam_layers8', FusedAdam(model, param_groups=layer_groups(model))),
                      ('atan2_ungrouped', None),
                      ('atan2_decay_groups', FusedAdamAtan2(model, lr=3e-4, param_groups=decay_groups(model, 0.1)))):
        table = opt._group_table(ps, opt.param_groups) if opt is not None else {}
        entry, struct_, fields = ('tfx_adam_step_groups', 'tfx_adam_group_args', adam) if name.startswith('adam') else ('tfx_adam_atan2_step', 'tfx_adam_atan2_args', atan2)
        arms[name] = (entry, capi.make_args(struct_, **table, **fields), table.get('nrange', 0))
        keep.append(table.get('ranges'))
    return arms, (ps.flat, m, v), keep


def caller(lib, stream):
    """(entry point, args) -> one launch on `lib` (a bare ctypes handle gets the three prototypes)"""
    for name in ('tfx_adam_step', 'tfx_adam_step_groups', 'tfx_adam_atan2_step'):
        fn = getattr(lib, name)
        if fn.argtypes is None:
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    return lambda entry, args: capi.check(getattr(lib, entry)(ctypes.byref(args), ctypes.c_void_p(stream)), entry)


def same_bits(arms, libs, bufs):
    """arm -> whether one launch from identical copies of p, m, v leaves the same bytes in all three on every library; p, m, v are put back"""
    start, out = [b.clone() for b in bufs], {}
    for k, (entry, args, _) in arms.items():
        got = []
        for go in libs.values():
            for b, b0 in zip(bufs, start):
                b.copy_(b0)
            go(entry, args); torch.cuda.synchronize()
            got.append([b.clone().view(torch.int32) for b in bufs])
        out[k] = all(torch.equal(x, y) for x, y in zip(*got))
    for b, b0 in zip(bufs, start):
        b.copy_(b0)
    return out


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def bench_launch(c, dev, a, parent):
    cfg = bench.CONFIGS[c]
    torch.manual_seed(0)
    model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
    arms, bufs, keep = launches(model)
    stream = torch.cuda.current_stream().cuda_stream
    libs = {'': caller(capi.lib(), stream)}
    if parent is not None:
        libs['parent_'] = caller(parent, stream)
    for go in libs.values():
        for entry, args, _ in arms.values():
            for _ in range(a.warmup):
                go(entry, args)
    torch.cuda.synchronize()
    same = same_bits(arms, libs, bufs) if parent is not None else {}          # after the warm-up: the moments are no longer zero
    ms = {(pre, k): [] for k in arms for pre in libs}
    for _ in range(a.rounds):                                # interleaved rounds: drift of the machine hits every arm and both libraries alike
        for (pre, k), t in ms.items():
            entry, args, _ = arms[k]
            t.append(timed(lambda: libs[pre](entry, args), a.steps))
    n = model.store.numel
    mean, spread = lambda t: sum(t) / len(t), lambda t: round((max(t) - min(t)) / (sum(t) / len(t)), 4)
    res = {}
    for k in arms:
        t = ms['', k]
        res[k] = dict(ranges=arms[k][2], mean_us=round(1e3 * mean(t), 1), min_us=round(1e3 * min(t), 1), max_us=round(1e3 * max(t), 1),
                      gb_per_s=round(28 * n / mean(t) / 1e6, 1), ratio_to_adam_ungrouped=round(mean(t) / mean(ms['', 'adam_ungrouped']), 4))
        if parent is not None:
            tp = ms['parent_', k]
            res[k].update(parent_mean_us=round(1e3 * mean(tp), 1), ratio_to_parent=round(mean(t) / mean(tp), 4), parent_spread=spread(tp), same_bits=same[k])
    return dict(elements=n, spread_of_adam=spread(ms['', 'adam_ungrouped']), **res)


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
    ap.add_argument('--config', type=int, default=0, help='2 or 3 (default: both)')
    ap.add_argument('--steps', type=int, default=20); ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='a second libtfx_hip.so: same_bits and ratio_to_parent for every arm')
    ap.add_argument('--step', action='store_true', help='also the whole training step at config 2, FusedAdam against FusedAdamAtan2')
    ap.add_argument('--train-steps', type=int, default=8); ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    out = {}
    for c in ([a.config] if a.config else [2, 3]):
        out[f'launch_config{c}'] = bench_launch(c, dev, a, parent)
        torch.cuda.empty_cache()
    if a.step:
        out['step_config2'] = bench_step(2, dev, a)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
