"""Cost of parameter groups in the fused Adam launch on one MI355X, on the flat buffers of BASELINE config 2 (dim 512 / depth 8) and config 3
(dim 1024 / depth 24).  Prints one JSON line.

  arms       ungrouped          `tfx_adam_step`, the launch FusedAdam makes by default
             decay_groups       `tfx_adam_step_groups` with the range table of `optim.decay_groups(model, 0.1)` (2 groups, decoupled decay)
             layers8            the same entry point with 8 groups cut at layer boundaries
             parent_ungrouped   `tfx_adam_step` of a second library (`--parent-lib`, e.g. the build of the commit before): the yardstick
  time       device events around `--steps` back-to-back launches, `--rounds` rounds, the arms alternated inside every round, after a warm-up
  traffic    28 bytes per element: p, g, m, v read, p, m, v written

    python tools/bench_adam_groups.py --parent-lib /path/to/libtfx_hip.so
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the BASELINE configs' model builder)
from transfusion_pytorch_amd import capi                     # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam, decay_groups   # noqa: E402


def layer_groups(model, groups=8):
    """`groups` parameter groups cut at layer boundaries (what is no layer's rides in the first), each with a learning rate of its own"""
    depth = model.md.depth
    out = [dict(params=[], lr=3e-4 * (1 + k)) for k in range(groups)]
    for n, p in model.store.params.items():
        parts = n.split('.')
        layer = int(parts[2]) if n.startswith('transformer.layers.') else 0
        out[layer * groups // depth]['params'].append(p)
    return out


def launches(model, parent):
    """arm name -> (closure that enqueues one launch, number of ranges)"""
    ps = model.store
    gen = torch.Generator(device=ps.flat.device).manual_seed(0)
    ps.grad.normal_(generator=gen).mul_(0.01)
    m, v = torch.zeros_like(ps.flat), torch.zeros_like(ps.flat)
    sumsq = (ps.grad.double() ** 2).sum().float().reshape(1)
    stream = torch.cuda.current_stream().cuda_stream
    common = dict(p=ps.flat, g=ps.grad, m=m, v=v, n=ps.numel, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0., max_norm=0.5, grad_scale=1.,
                  step=10, sumsq=sumsq)
    keep = [m, v, sumsq]
    plain = capi.make_args('tfx_adam_args', **common)
    arms = {'ungrouped': (lambda: capi.call('tfx_adam_step', plain, stream), 0)}
    if parent is not None:
        fn = parent.tfx_adam_step
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
        arms['parent_ungrouped'] = (lambda: capi.check(fn(ctypes.byref(plain), ctypes.c_void_p(stream)), 'parent tfx_adam_step'), 0)
    for name, pg in (('decay_groups', decay_groups(model, 0.1)), ('layers8', layer_groups(model))):
        opt = FusedAdam(model, param_groups=pg)
        ranges, nrange = opt._range_table(ps)
        rec = list(zip(*(opt._group_scalars(g) for g in opt.param_groups)))
        a = capi.make_args('tfx_adam_group_args', ranges=ranges, nrange=nrange, ngroup=len(opt.param_groups), group_lr=rec[0], group_beta1=rec[1],
                           group_beta2=rec[2], group_eps=rec[3], group_weight_decay=rec[4], group_decoupled=rec[5], **common)
        keep += [ranges, a]
        arms[name] = (lambda a=a: capi.call('tfx_adam_step_groups', a, stream), nrange)
    return arms, keep


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=0, help='2 or 3 (default: both)')
    ap.add_argument('--steps', type=int, default=20); ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help='a second libtfx_hip.so whose tfx_adam_step is timed in the same rounds')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    out = {}
    for c in ([a.config] if a.config else [2, 3]):
        cfg = bench.CONFIGS[c]
        torch.manual_seed(0)
        model = bench.build_model(cfg['dim'], cfg['depth'], cfg['two'], dev).train()
        arms, keep = launches(model, parent)
        for fn, _ in arms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):                            # interleaved rounds: box drift hits every arm alike
            for k, (fn, _) in arms.items():
                ms[k].append(timed(fn, a.steps))
        n = model.store.numel
        res = {k: dict(ranges=arms[k][1], mean_us=round(1e3 * sum(t) / len(t), 1), min_us=round(1e3 * min(t), 1), max_us=round(1e3 * max(t), 1),
                       gb_per_s=round(28 * n / (sum(t) / len(t)) / 1e6, 1)) for k, t in ms.items()}
        yard = 'parent_ungrouped' if parent is not None else 'ungrouped'
        for k in res:
            res[k]['ratio_to_' + yard] = round(res[k]['mean_us'] / res[yard]['mean_us'], 4)
        out[f'config{c}'] = dict(elements=n, **res)
        del model, arms, keep
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
