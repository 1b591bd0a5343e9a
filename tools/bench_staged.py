"""Per-launch time of the NT GEMMs whose epilogue goes through the staged block (csrc/stage_block.h), one (kernel, epilogue) pair per line, and of the
attention forward / backward at the config-2 geometry (tools/bench_attn.py), one build against another.  Method of tools/bench_nt_ring.py: device events
around 50 launches after warm-up, fresh children alternated between the two libraries.

    python tools/bench_staged.py                          # one pass with the library in use: `<name> <us>` lines
    python tools/bench_staged.py --ab BASE NEW [PAIRS]    # PAIRS (default 5) alternated pairs; per launch both medians, the base build's spread
                                                          # (max - min over its repeats) and whether NEW's median stays within it
Shapes: what a config-2 training step and a config-5 decode plan launch (tests/test_host_cpu.py test_nt_gemm_kernel_selection, tools/bench_nt_ring.py);
every one is checked against tfx_gemm_nt_plan before it is timed.
"""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GLDS, MID, PP, SKINNY, DECODE, OW, OWP = 1, 2, 3, 4, 5, 6, 7
T = 65536
SHAPES = [(OWP, T, 1544, 512, 'BF16'), (OWP, T, 512, 512, 'BF16'), (OWP, T, 512, 1408, 'BF16'), (OW, T, 512, 128, 'BF16'), (OW, T, 512, 1024, 'F32'),
          (PP, T, 2816, 512, 'GEGLU'), (PP, T, 1408, 512, 'GEGLU_BWD'), (PP, T, 512, 512, 'RESID'), (PP, T, 512, 512, 'F32'), (PP, T, 1544, 512, 'QKV_NORM_ROPE'),
          (GLDS, T, 256, 512, 'BF16'), (MID, 8192, 384, 1024, 'BF16'), (SKINNY, 640, 3080, 1024, 'BF16'), (DECODE, 640, 1024, 1024, 'BF16'),
          (DECODE, 64, 5632, 1024, 'BF16'), (DECODE, 640, 1024, 1024, 'RESID'), (DECODE, 640, 1544, 1024, 'QKV_NORM_ROPE')]


def one_pass():
    import torch
    from transfusion_pytorch_amd import capi
    from bench_gemm import timeit, st, dev, BF
    for kind, M, N, K, epi in SHAPES:
        A = torch.randn(M, K, device=dev).to(BF); B = (torch.randn(N, K, device=dev) * K ** -0.5).to(BF)
        ldc = (N + 63) // 64 * 64 if epi == 'QKV_NORM_ROPE' else 2 * N if epi == 'GEGLU_BWD' else N
        kw = dict(C=torch.empty(M, ldc, device=dev, dtype=torch.float32 if epi == 'F32' else BF), ldc=ldc)
        if epi == 'GEGLU':
            kw.update(C2=torch.empty(M, N // 2, device=dev, dtype=BF), ldc2=N // 2, bias=torch.randn(N, device=dev))
        elif epi == 'GEGLU_BWD':
            kw.update(aux=torch.randn(M, 2 * N, device=dev).to(BF), ldaux=2 * N)
        elif epi == 'RESID':
            kw.update(R=torch.randn(M, N, device=dev).to(BF), ldr=N, bias=torch.randn(N, device=dev))
        elif epi == 'QKV_NORM_ROPE':                           # 8 heads; the decode launch appends its k~ | v rows to a KV cache
            ang = torch.arange(1024).float()[:, None] * (1. / (10000 ** (torch.arange(0, 64, 2).float() / 64)))[None]
            kw.update(C2=torch.empty(M, 1024, device=dev, dtype=BF), ldc2=1024, qk_heads=8, qk_gamma_q=torch.randn(64, device=dev) * 0.2,
                      qk_gamma_k=torch.randn(64, device=dev) * 0.2, qk_rot_pos=torch.randint(0, 1000, (M,), device=dev, dtype=torch.int32),
                      qk_cos=ang.cos().to(dev).contiguous(), qk_sin=ang.sin().to(dev).contiguous(), qk_q_scale=0.125, qk_norm_scale=8.0,
                      qk_plan=torch.empty(8, device=dev), qk_softcap=50.0)
            if kind == DECODE:
                kw.update(qk_cache=torch.empty(4 * M, 1024, device=dev, dtype=BF), qk_ld_cache=1024,
                          qk_cache_pos=torch.randperm(4 * M, device=dev)[:M].to(torch.int32))
        a = capi.make_args('tfx_gemm_nt_args', A=A, lda=K, B=B, ldb=K, M=M, N=N, K=K, epi=capi.ENUMS['TFX_EPI_' + epi], **kw)
        k, g = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(k), ctypes.byref(g)) == 0 and k.value == kind, (kind, M, N, K, epi, k.value)
        t = timeit(lambda: capi.call('tfx_gemm_nt', a, st()), n=50)
        print(f'nt{kind}_{M}x{N}x{K}_{epi} {t * 1e6:.2f}', flush=True)
        del A, B, kw, a
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'bench_attn.py'), '20'], capture_output=True, text=True, timeout=300)   # fresh child, same TFX_LIB
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r'attn_fwd\s+([\d.]+) us.*attn_bwd \(prep \+ dkv \+ dq\)\s+([\d.]+) us', r.stdout)
    print(f'attn_fwd_config2 {m.group(1)}\nattn_bwd_config2 {m.group(2)}', flush=True)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if len(sys.argv) > 1 and sys.argv[1] == '--ab':
        import bench_nt_ring
        bench_nt_ring.__file__ = os.path.abspath(__file__)     # its children run this file's pass
        bench_nt_ring.ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5)
    else:
        one_pass()
