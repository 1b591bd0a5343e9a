"""Per-launch time of the 4-wave LDS-DMA NT kernels (csrc/nt_ring.h: glds / mid / skinny) on shapes the planner sends to each, and of FusedMuon.step()
(its grouped products run the same K loop), one build against another.  Method of tools/bench_gemm.py: device events around 50 launches after warm-up.

    python tools/bench_nt_ring.py                          # one pass over the shapes with the library in use: `<name> <us>` lines
    python tools/bench_nt_ring.py --ab BASE NEW [PAIRS]    # PAIRS (default 5) alternated fresh children per library (TFX_LIB); per shape both medians, the
                                                           # base build's spread (max - min over its repeats) and whether NEW's median stays within it
Shapes: the config-2 training step's 128 x 128 launches and the dim-1024 decode / prefill / conditioning launches of the config-5 sample_many plans
(tests/test_host_cpu.py test_nt_gemm_kernel_selection); every one is checked against tfx_gemm_nt_plan before it is timed.
"""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GLDS, MID, SKINNY = 1, 2, 4
SHAPES = [(GLDS, 65536, 256, 512, 'BF16'), (GLDS, 16384, 512, 512, 'BF16'), (GLDS, 65536, 128, 1024, 'F32'), (GLDS, 16384, 1024, 1408, 'BF16'),
          (MID, 8192, 384, 1024, 'BF16'), (MID, 640, 5504, 1024, 'BF16'), (MID, 1024, 3080, 1024, 'BF16'), (MID, 2048, 2048, 24576, 'F32'),
          (SKINNY, 640, 3080, 1024, 'BF16'), (SKINNY, 256, 5504, 1024, 'BF16'), (SKINNY, 64, 5632, 128, 'BF16'), (SKINNY, 512, 4096, 1024, 'SILU')]


def one_pass():
    import torch
    from transfusion_pytorch_amd import capi
    from transfusion_pytorch_amd.optim import FusedMuon
    from bench_gemm import timeit, st, dev, BF
    import bench_muon
    for kind, M, N, K, epi in SHAPES:
        A = torch.randn(M, K, device=dev).to(BF); B = (torch.randn(N, K, device=dev) * K ** -0.5).to(BF)
        C = torch.empty(M, N, device=dev, dtype=torch.float32 if epi == 'F32' else BF)
        kw = dict(C2=torch.empty(M, N, device=dev, dtype=BF), ldc2=N) if epi == 'SILU' else {}
        a = capi.make_args('tfx_gemm_nt_args', A=A, lda=K, B=B, ldb=K, M=M, N=N, K=K, epi=capi.ENUMS['TFX_EPI_' + epi], C=C, ldc=N, **kw)
        k, g = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(k), ctypes.byref(g)) == 0 and k.value == kind, (kind, M, N, K, k.value)
        t = timeit(lambda: capi.call('tfx_gemm_nt', a, st()), n=50)
        print(f'nt{kind}_{M}x{N}x{K}_{epi} {t * 1e6:.2f}', flush=True)
    for c in (2, 3):                                           # all Newton-Schulz products of the config's matrices: 15 grouped launches per step
        m = bench_muon.model_with_gradient(c, torch.device('cuda:0'))
        opt = FusedMuon(m, lr=3e-4, max_grad_norm=0.5)
        for _ in range(3):
            opt.step()
        print(f'fused_muon_step_config{c} {bench_muon.timed(opt.step, 50) * 1e3:.2f}', flush=True)
        del m, opt


def ab(base, new, pairs):
    res = {base: {}, new: {}}
    for i in range(pairs):
        for lib in ((base, new), (new, base))[i & 1]:          # neither build always runs second
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, TFX_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            for ln in r.stdout.splitlines():
                name, us = ln.split()
                res[lib].setdefault(name, []).append(float(us))
    bad = 0
    print(f'{"launch":34s} {"base median":>12s} {"new median":>12s} {"base spread":>12s}   (us; {pairs} alternated pairs)')
    for name, b in res[base].items():
        n = res[new][name]
        mb, mn, spread = statistics.median(b), statistics.median(n), max(b) - min(b)
        ok = mn <= mb + spread
        bad += not ok
        print(f'{name:34s} {mb:12.2f} {mn:12.2f} {spread:12.2f}   {"ok" if ok else "SLOWER"}')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if len(sys.argv) > 1 and sys.argv[1] == '--ab':
        ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 5)
    else:
        one_pass()
