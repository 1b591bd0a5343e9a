"""Bit identity of the 4-wave LDS-DMA NT kernels (csrc/nt_ring.h) between two builds of the library: sha256 of every output buffer of every form-1 / 2 / 4
case of tests/_gemm_cases.py NT_CASES and of the problems of tests/test_muon_gpu.py test_grouped_products_asymmetric_ragged, on their seeded operands.

    python tools/nt_ring_digests.py                    # the listing of the library in use (TFX_LIB or the in-tree build)
    python tools/nt_ring_digests.py LIB_A LIB_B        # one fresh child per library; exit status 1 unless the listings are equal line for line
    python tools/nt_ring_digests.py --staged [LIB_A LIB_B]
                                                       # the staged epilogues (csrc/stage_block.h) instead: every case of NT_CASES, NT_FAMILY_CASES (a second child
                                                       # per library with TFX_NT_PP_MIN=1, as in the tests), the fused QK-norm + RoPE projection on the ping-pong
                                                       # kernel (M = 1025) and on the decode kernel with its KV-cache append, and tests/_attn_cases.py's catalogue
                                                       # through run_kernels (forward, dQ, dK / dV; plain and with the norm + RoPE backward folded in)
"""
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def sha(t):
    return hashlib.sha256(t.contiguous().view(-1).view(__import__('torch').uint8).cpu().numpy().tobytes()).hexdigest()


def listing():
    import _gemm_cases as G
    import test_muon_gpu as TM
    nt_case_digests([sp for sp in G.NT_CASES if sp.form in (1, 2, 4)])

    def digest_group(tag, problems, alpha, beta):
        for i, o in enumerate(TM.run_group(problems, alpha, beta)):
            for k in ('C', 'Ct'):
                if o[k] is not None:
                    print(f'{sha(o[k])}  muon {tag}[{i}] {k}')
    TM.check_group = digest_group                              # the test's own problems and generator, hashed instead of checked
    TM.test_grouped_products_asymmetric_ragged()


def nt_case_digests(specs):
    import torch
    from transfusion_pytorch_amd import capi
    import _gemm_cases as G
    for sp in specs:
        case = G.build_nt(sp, 'cuda')
        a = capi.make_args('tfx_gemm_nt_args', epi=capi.ENUMS['TFX_EPI_' + sp.epi], **case.kw)
        kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0 and kind.value == sp.form, (sp.name, kind.value)
        capi.call('tfx_gemm_nt', a, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for o in case.outs:                                    # whole buffers, guard bands included
            print(f'{sha(o.buf)}  {sp.name} | {o.name}')


def qknr_digests(T, want_kind, with_cache):
    """the operands of test_kernels_gpu's fused QK-norm + RoPE tests; every output buffer whole (NaN-filled before the launch, cache rows 7.0)"""
    import torch
    from transfusion_pytorch_amd import capi
    BF, DEV = torch.bfloat16, 'cuda'
    torch.manual_seed(41)
    d, H = 1024, 8
    HD = H * 64
    N = 3 * HD + H; ldq = (N + 63) // 64 * 64
    u, W = (torch.randn(T, d, device=DEV)).to(BF), (torch.randn(N, d, device=DEV) * d ** -0.5).to(BF)
    gq, gk = torch.randn(64, device=DEV) * 0.2, torch.randn(64, device=DEV) * 0.2
    pos = torch.randint(0, 1000, (T,), device=DEV, dtype=torch.int32)
    ang = torch.arange(1024).float()[:, None] * (1. / (10000 ** (torch.arange(0, 64, 2).float() / 64)))[None]
    cos_t, sin_t = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    cpos = torch.randperm(4 * T, device=DEV)[:T].to(torch.int32)
    cpos[torch.rand(T, device=DEV) < 0.2] = -1
    C = torch.full((T, ldq), float('nan'), device=DEV, dtype=BF); qk = torch.full((T, 2 * HD), float('nan'), device=DEV, dtype=BF)
    cache = torch.full((4 * T, 2 * HD), 7.0, device=DEV, dtype=BF); plan = torch.full((8,), float('nan'), device=DEV)
    kw = dict(A=u, lda=d, B=W, ldb=d, M=T, N=N, K=d, epi=capi.ENUMS['TFX_EPI_QKV_NORM_ROPE'], C=C, ldc=ldq, C2=qk, ldc2=2 * HD, qk_heads=H, qk_gamma_q=gq,
              qk_gamma_k=gk, qk_rot_pos=pos, qk_cos=cos_t, qk_sin=sin_t, qk_q_scale=0.125, qk_norm_scale=8.0, qk_plan=plan, qk_softcap=50.0)
    if with_cache:
        kw.update(qk_cache=cache, qk_ld_cache=2 * HD, qk_cache_pos=cpos)
    a = capi.make_args('tfx_gemm_nt_args', **kw)
    kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
    assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0 and kind.value == want_kind, (T, kind.value)
    capi.call('tfx_gemm_nt', a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isfinite(qk.float()).all()                    # q~ | k~ written (by either form: the plan kind above says that the fused one ran)
    for name, t in (('C', C), ('qk', qk), ('plan', plan)) + ((('cache', cache),) if with_cache else ()):
        print(f'{sha(t)}  qknr nt{want_kind} M={T} cache={int(with_cache)} | {name}')


def listing_staged():
    import _gemm_cases as G
    if os.environ.get('TFX_NT_PP_MIN') == '1':                 # the 256 x 256 family's child
        nt_case_digests(G.NT_FAMILY_CASES)
        return qknr_digests(1025, 3, False)
    nt_case_digests(G.NT_CASES)
    for T in (640, 600, 130):
        qknr_digests(T, 5, True)
    import _attn_cases as AC
    for case in AC.CATALOGUE:
        for nr in (False, True):
            got = AC.run_kernels(case, 0, nr=nr)[-1]
            for k, t in sorted(got['raw'].items()):
                print(f'{sha(t)}  attn {case.name} nr={int(nr)} | {k}')
            for k in ('do_eff', 'delta'):                      # (not dgq / dgk: fp32 atomic sums over the blocks, another rounding order in every run of one library)
                print(f'{sha(got[k])}  attn {case.name} nr={int(nr)} | {k}')


def main():
    libs = sys.argv[1:]
    staged = libs[:1] == ['--staged']
    libs = libs[staged:]
    if not libs:
        return listing_staged() if staged else listing()
    outs = []
    for lib in libs:
        out = []
        for env in ({}, {'TFX_NT_PP_MIN': '1'}) if staged else ({},):
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + ['--staged'] * staged, env=dict(os.environ, TFX_LIB=os.path.abspath(lib), **env),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            out += r.stdout.splitlines()
        outs.append(out)
        print(f'# {lib}: {len(outs[-1])} buffers')
    print('\n'.join(outs[0]))
    diff = [(a, b) for o in outs[1:] for a, b in zip(outs[0], o) if a != b] + [None for o in outs[1:] if len(o) != len(outs[0])]
    for d in diff:
        print('DIFFERENT:', d)
    print('listings equal line for line' if not diff else f'{len(diff)} lines differ')
    sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
