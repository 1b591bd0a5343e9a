"""Throughput of the KV-cached decode twin (sample_many / generate_text_only) on one GPU: tokens per second, host-bound or not.
   python tools/bench_sample.py [--dim 512 --depth 8 --batch 64 --new 64] [--ode-method euler --modality-steps 31]
   python tools/bench_sample.py --config5 --ode-method ab4 --modality-steps 16    # a multistep rule: 24 forwards per modality against midpoint's 30
   python tools/bench_sample.py --config5 --ode-method rk4 --modality-steps 9      # sample_many alone, at the configuration `bench.py --sample` times
   python tools/bench_sample.py --config5 --temperature 1 --top-k 40 --top-p 0.9   # the text draw behind the top-k / top-p filters (a temperature: greedy ignores them)"""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transfusion_pytorch_amd import Transfusion

ap = argparse.ArgumentParser()
ap.add_argument('--dim', type=int, default=512); ap.add_argument('--depth', type=int, default=8)
ap.add_argument('--batch', type=int, default=64); ap.add_argument('--new', type=int, default=64); ap.add_argument('--prompt', type=int, default=128)
ap.add_argument('--ode-method', default='midpoint', help='fixed-grid solver of the modality phases: euler, midpoint, heun2, heun3, rk4, or a multistep rule ab2, ab3, ab4 (ode.py)')
ap.add_argument('--modality-steps', type=int, default=8, help='grid points of the solver: stages x (modality-steps - 1) forwards per modality (ab2 / ab3 / ab4: one per step after the start-up steps)')
ap.add_argument('--config5', action='store_true', help='time sample_many alone at SURVEY 8(d) config 5 (dim 1024, depth 24, 64 mixed prompts, '
                'max_length 256, cfg 3, greedy text, a forced modality at the start), as `bench.py --sample` does for midpoint with 16 grid points')
ap.add_argument('--top-k', type=int, default=None, help='top-k filter of the text draw (tfx_sample_tokens_filtered); needs a temperature')
ap.add_argument('--top-p', type=float, default=None, help='nucleus filter of the text draw; needs a temperature')
ap.add_argument('--temperature', type=float, default=None, help='text temperature (default: greedy, 0, where the runs below are greedy today; sample_many\'s own 1 in the last)')
a = ap.parse_args()
temp = 0. if a.temperature is None else a.temperature
if (a.top_k or (a.top_p is not None and a.top_p < 1.)) and temp == 0.:
    print('note: greedy text (temperature 0) ignores --top-k / --top-p; pass --temperature')
torch.manual_seed(0)
okw = dict(odeint_kwargs=dict(atol=1e-5, rtol=1e-5, method=a.ode_method))
if a.config5:
    from transfusion_pytorch_amd.ode import ode_schedule
    m = Transfusion(num_text_tokens=256, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=1024, depth=24), **okw).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(1234)
    prompts = []
    for _ in range(16):                                              # the four README prompt kinds, as bench.py's sample_prompts
        prompts += [torch.randint(0, 256, (16,), device='cuda', generator=g), (0, torch.randn(4, 384, device='cuda', generator=g)), None,
                    [torch.randint(0, 256, (8,), device='cuda', generator=g), (0, torch.randn(6, 384, device='cuda', generator=g))]]
    noise = torch.randn(16, 384, device='cuda', generator=g)
    kw = dict(max_length=256, modality_steps=a.modality_steps, cfg_scale=3., text_temperature=temp, init_modality_noise=noise, fixed_modality_shape=(4,),
              force_modality_at_start=0, text_top_k=a.top_k, text_top_p=a.top_p)
    m.sample_many(prompts, **{**kw, 'max_length': 24})                # warm-up (plans, shadows)
    secs = []
    for _ in range(2):                                               # the first full-length call builds its plans; the second runs on the kept ones
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = m.sample_many(prompts, **kw)
        torch.cuda.synchronize(); secs.append(time.perf_counter() - t0)
    nmod = sum(sum(isinstance(p, tuple) for p in s) for s in res) - sum(sum(isinstance(q, tuple) for q in (p if isinstance(p, list) else [p])) for p in prompts)
    evals = len(ode_schedule(a.ode_method, a.modality_steps))
    print(f'sample_many config5_forced {a.ode_method} S={a.modality_steps} ({evals} evaluations per modality), '
          f'temperature {temp} top_k {a.top_k} top_p {a.top_p}: first call {secs[0]:.3f} s, repeat call {secs[1]:.3f} s, {nmod} decoded modalities')
    sys.exit(0)
m = Transfusion(num_text_tokens=256, dim_latent=384, modality_default_shape=(4,), transformer=dict(dim=a.dim, depth=a.depth), **okw).cuda().eval()
prompt = torch.randint(0, 256, (a.batch, a.prompt), device='cuda')
m.generate_text_only(prompt, a.prompt + 4, temperature=temp, top_k=a.top_k, top_p=a.top_p)          # warm-up (plans, shadows)
torch.cuda.synchronize(); t0 = time.perf_counter()
out = m.generate_text_only(prompt, a.prompt + a.new, temperature=temp, top_k=a.top_k, top_p=a.top_p)
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f'generate_text_only dim{a.dim}/d{a.depth}: batch {a.batch}, prompt {a.prompt}, {a.new} new tokens: {dt * 1e3:.1f} ms '
      f'= {dt / a.new * 1e3:.2f} ms/step, {a.batch * a.new / dt:.0f} tokens/s')
prompts = [[torch.randint(0, 256, (16,), device='cuda'), (0, torch.randn(4, 384, device='cuda'))] for _ in range(a.batch)]
m.sample_many(prompts, max_length=8, modality_steps=4)
torch.cuda.synchronize(); t0 = time.perf_counter()
res = m.sample_many(prompts, max_length=a.new, modality_steps=a.modality_steps, text_top_k=a.top_k, text_top_p=a.top_p,
                    **({} if a.temperature is None else dict(text_temperature=a.temperature)))
torch.cuda.synchronize(); dt = time.perf_counter() - t0
ntok = sum(sum((len(p) if not isinstance(p, tuple) else p[1].shape[0]) for p in s) for s in res)
print(f'sample_many ({a.ode_method}, {a.modality_steps} grid points): {a.batch} prompts, max_length {a.new}: {dt * 1e3:.1f} ms, {ntok} tokens in the returned samples')
