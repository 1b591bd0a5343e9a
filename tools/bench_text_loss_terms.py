"""What the text loss terms (`model.set_text_loss_terms_(z_loss, label_smoothing)`) cost: the `_reg` cross-entropy launches against the plain ones, and the whole
step with the terms off and on.  Alternated rounds on one process (the arms share the buffers, the weights and the box's drift), HIP events around the launches.

  kernels   tfx_ce_fwd_bwd | tfx_ce_reg_fwd_bwd at 65 536 x 448 (V = 395: the fused kernel's register path), tfx_ce_fwd | tfx_ce_reg_fwd and tfx_ce_bwd |
            tfx_ce_reg_bwd on a 16 384-row chunk x 32 064 (V = 32 003: the wide kernels), us per launch and TB/s over the bytes a launch has to move (fp32 logits in,
            bf16 d logits out).  The `_reg` arms run z alone, smoothing alone (the extra row sum) and both.
  step      BASELINE config 2 (dim 512, depth 8, 64 x 1024 tokens of the canonical sample): forward, backward, clip + FusedAdam, terms off against (1e-4, 0.1).

Per arm the best round and the spread of its rounds (max - min): the expectation is that an `_reg` arm sits inside the spread of the plain arm of the same run.
Information only (profiles/text_loss_terms.txt).  One JSON line per part.

    python tools/bench_text_loss_terms.py
    python tools/bench_text_loss_terms.py --rounds 2 --reps 5 --steps 3 --batch 16
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                # noqa: E402  (the flagship workload's batch)
from bench_frozen import timed_steps                        # noqa: E402
from transfusion_pytorch_amd import Transfusion, capi      # noqa: E402
from transfusion_pytorch_amd.optim import FusedAdam        # noqa: E402

REG_ARMS = {'z': (1e-4, 0.0), 'smooth': (0.0, 0.1), 'both': (1e-4, 0.1)}


def time_launch(fn, args, reps):
    """mean us of `reps` back-to-back launches of one entry point (one warm-up launch in front)"""
    stream = torch.cuda.current_stream().cuda_stream
    capi.call(fn, args, stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        capi.call(fn, args, stream)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def summarise(rounds, nbytes):
    out = {}
    for arm, us in rounds.items():
        out[arm] = dict(best_us=round(min(us), 2), spread_us=round(max(us) - min(us), 2), tb_s=round(nbytes / (min(us) * 1e-6) / 1e12, 3), rounds_us=[round(v, 2) for v in us])
    for arm in out:
        if arm != 'plain':
            out[arm]['over_plain_us'] = round(out[arm]['best_us'] - out['plain']['best_us'], 2)
            out[arm]['inside_plain_spread'] = bool(abs(out[arm]['over_plain_us']) <= out['plain']['spread_us'])
    return out


def kernels(a):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    # ---- fused, 65 536 x 448
    T, V, ld = 65536, 395, 448
    lg = torch.randn(T, ld, device=dev, generator=g) * 3
    lab = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
    lab[::7] = -1
    dl = torch.empty(T, ld, device=dev, dtype=torch.bfloat16)
    acc, aux = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    common = dict(T=T, V=V, logits=lg, ld=ld, labels=lab, grad_scale=1e-3, dlogits=dl, ld_d=ld, acc=acc)
    arms = {'plain': ('tfx_ce_fwd_bwd', capi.make_args('tfx_ce_args', **common))}
    for name, (z, e) in REG_ARMS.items():
        arms[name] = ('tfx_ce_reg_fwd_bwd', capi.make_args('tfx_ce_reg_args', z_weight=z, smoothing=e, aux=aux, **common))
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (fn, args) in arms.items():
            rounds[k].append(time_launch(fn, args, a.reps))
    res['fused_65536x448'] = summarise(rounds, T * ld * 6)
    del lg, dl
    # ---- split, a 16 384-row chunk x 32 064
    T, V, ld = 16384, 32003, 32064
    lg = torch.randn(T, ld, device=dev, generator=g) * 3
    lab = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
    lab[::7] = -1
    dl = torch.empty(T, ld, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(T, device=dev)
    common = dict(T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, grad_scale=1e-3, scale_dev=None, dlogits=dl, ld_d=ld)
    plain = capi.make_args('tfx_ce_chunk_args', **common)
    regs = {name: capi.make_args('tfx_ce_reg_chunk_args', z_weight=z, smoothing=e, aux=aux, **common) for name, (z, e) in REG_ARMS.items()}
    for d, nbytes in (('fwd', T * ld * 4), ('bwd', T * ld * 6)):
        arms = {'plain': (f'tfx_ce_{d}', plain), **{k: (f'tfx_ce_reg_{d}', v) for k, v in regs.items()}}
        rounds = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, (fn, args) in arms.items():
                rounds[k].append(time_launch(fn, args, a.reps))
        res[f'{d}_16384x32064'] = summarise(rounds, nbytes)
    print(json.dumps(dict(part='kernels', rounds=a.rounds, reps=a.reps, reg_arms={k: list(v) for k, v in REG_ARMS.items()}, **res)), flush=True)


def step(a):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Transfusion(num_text_tokens=256, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=512, depth=8)).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = bench.canonical_batch(a.batch, dev, gen)
    arms = {'off': (0.0, 0.0), 'on': (1e-4, 0.1)}
    res = {k: dict(step_ms=[], fwd_ms=[], bwd_ms=[], opt_ms=[]) for k in arms}
    terms = None
    for _ in range(a.rounds):
        for name, (z, e) in arms.items():
            model.set_text_loss_terms_(z, e)
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
            total, (f, b, o) = timed_steps(model, opt, batch, a.steps, a.warmup)
            r = res[name]
            r['step_ms'].append(round(total, 3)); r['fwd_ms'].append(round(f, 3)); r['bwd_ms'].append(round(b, 3)); r['opt_ms'].append(round(o, 3))
            assert (model._live[0].reg is not None) == (name == 'on')
            if name == 'on':
                t = model.text_loss_terms()
                terms = dict(text=float(t.text), ce=float(t.ce), lse_sq=float(t.lse_sq))
            del opt
    best = {k: {m: min(v) for m, v in r.items()} for k, r in res.items()}
    spread = {k: round(max(r['step_ms']) - min(r['step_ms']), 3) for k, r in res.items()}
    extra = round(best['on']['step_ms'] - best['off']['step_ms'], 3)
    print(json.dumps(dict(part='step', dim=512, depth=8, tokens_per_step=a.batch * 1024, workload='forward + backward + clip(0.5) + FusedAdam', terms_on=list(arms['on']),
                          best=best, spread_ms=spread, on_over_off_ms=extra, inside_off_spread=bool(abs(extra) <= spread['off']),
                          rounds_ms={k: v['step_ms'] for k, v in res.items()}, last_text_loss_terms=terms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64); ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--part', choices=('kernels', 'step', 'all'), default='all')
    a = ap.parse_args()
    if a.part in ('kernels', 'all'):
        kernels(a)
    if a.part in ('step', 'all'):
        step(a)


if __name__ == '__main__':
    main()
