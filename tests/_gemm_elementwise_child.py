"""Child process of test_gemm_elementwise_gpu.py::test_nt_256_family_per_element and ::test_nt_register_staged_geglu_per_element: the library reads TFX_NT_PP_MIN / TFX_NT_OW once per process, so the
256 x 256 NT family (ping-pong kernel, one-wave kernels) at small shapes runs here, under the switches of its environment.  Every case of
_gemm_cases.NT_FAMILY_CASES: the kind through tfx_gemm_nt_plan, the launch, the fp64 reference, the per-element bound and the guard bands.  One line per case,
`CASE <name> kind=<k> ok ratio=<worst error / bound>` or `CASE <name> FAIL <what, with row, column, error and bound>`; exit status 1 at the first failure.
With TFX_GEMM_GLDS=0 in the environment (every launch on the register-staged kernels) it runs the GEGLU / GEGLU_BWD cases of NT_CASES (NT_STAGED_GEGLU) instead: the one
(form, epilogue) pair the default environment cannot reach, N % 64 == 0 being a multiple of 4."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from transfusion_pytorch_amd import capi  # noqa: E402
import _gemm_cases as G  # noqa: E402

DEV = 'cuda'


def plan_kind(a):
    kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
    assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0
    return kind.value


def qknr_case(st):
    """TFX_EPI_QKV_NORM_ROPE at qk_heads = 2, N = 264, M = 1025 on the ping-pong kernel: the raw projection per element against fp64, q~ | k~ and the soft-cap
    plan bit for bit against tfx_qk_norm_rope_fwd of the kernel's own C"""
    M, N, K, H = 1025, 264, 128, 2
    g = torch.Generator().manual_seed(77)
    u = (torch.randn(M, K, generator=g)).to(G.BF).to(DEV); W = (torch.randn(N, K, generator=g) * K ** -0.5).to(G.BF).to(DEV)
    ubuf, uv = G.padded(u); Wbuf, Wv = G.padded(W)
    gq = (torch.randn(64, generator=g) * 0.2).to(DEV); gk = (torch.randn(64, generator=g) * 0.2).to(DEV)
    pos = torch.randint(0, 1000, (M,), generator=g).to(torch.int32).to(DEV)
    freqs = 1. / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.arange(1024).float()[:, None] * freqs[None]
    cos_t, sin_t = ang.cos().to(DEV).contiguous(), ang.sin().to(DEV).contiguous()
    Cbuf, Cv = G.guarded(M, N, G.BF, DEV); Qbuf, Qv = G.guarded(M, 2 * H * 64, G.BF, DEV)
    before = (Cbuf.clone(), Qbuf.clone())
    plan1 = torch.full((8,), float('nan'), device=DEV)
    a = capi.make_args('tfx_gemm_nt_args', A=uv, lda=K + G.GUARD, B=Wv, ldb=K + G.GUARD, M=M, N=N, K=K, epi=capi.ENUMS['TFX_EPI_QKV_NORM_ROPE'], C=Cv, ldc=N + G.GUARD,
                       C2=Qv, ldc2=2 * H * 64 + G.GUARD, qk_heads=H, qk_gamma_q=gq, qk_gamma_k=gk, qk_rot_pos=pos, qk_cos=cos_t, qk_sin=sin_t, qk_q_scale=0.125,
                       qk_norm_scale=8.0, qk_plan=plan1, qk_softcap=50.0)
    kind = plan_kind(a)
    assert kind == 3, f'planner names kind {kind}, not the ping-pong kernel'
    capi.call('tfx_gemm_nt', a, st)
    torch.cuda.synchronize()
    x, E = G.nt_ref(u, W)
    worst = G.assert_elementwise('qknr C', Cv, x, G.tol_bf16(x, E), (256, 256))
    qk0 = torch.full((M, 2 * H * 64), float('nan'), device=DEV, dtype=G.BF); plan0 = torch.full((8,), float('nan'), device=DEV)
    b = capi.make_args('tfx_qk_norm_rope_args', T=M, H=H, qkv=Cv, ld_qkv=N + G.GUARD, qk=qk0, ld_qk=2 * H * 64, gamma_q=gq, gamma_k=gk, rot_pos=pos, cos_tab=cos_t,
                       sin_tab=sin_t, q_scale=0.125, norm_scale=8.0, sc_plan=plan0, softcap=50.0)
    capi.call('tfx_qk_norm_rope_fwd', b, st)
    torch.cuda.synchronize()
    assert torch.isfinite(qk0.float()).all()
    assert torch.equal(G._bits(Qv), G._bits(qk0)), f'q~ | k~ differ from tfx_qk_norm_rope_fwd of the same C in {int((G._bits(Qv) != G._bits(qk0)).sum())} elements'
    assert torch.equal(plan1, plan0), 'soft-cap plan'
    for nm, buf, bef, rows, cols in (('qknr C', Cbuf, before[0], M, N), ('qknr C2', Qbuf, before[1], M, 2 * H * 64)):
        written = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
        written[G.GUARD:G.GUARD + rows, :cols] = True
        G.assert_untouched(nm, buf, bef, written)
    return kind, worst


def main():
    st = torch.cuda.current_stream().cuda_stream
    pp_only = os.environ.get('TFX_NT_OW') == '0'
    staged = os.environ.get('TFX_GEMM_GLDS') == '0'
    assert staged or os.environ.get('TFX_NT_PP_MIN') == '1'
    for sp in (G.NT_STAGED_GEGLU if staged else G.NT_FAMILY_CASES):
        if pp_only and sp.form == 3:
            continue                                              # (already ran on the ping-pong kernel in the default mode)
        want = 0 if staged else 3 if pp_only else sp.form
        try:
            case = G.build_nt(sp, DEV)
            a = capi.make_args('tfx_gemm_nt_args', epi=capi.ENUMS['TFX_EPI_' + sp.epi], **case.kw)
            kind = plan_kind(a)
            assert kind == want, f'planner names kind {kind}, the case wants {want}'
            capi.call('tfx_gemm_nt', a, st)
            torch.cuda.synchronize()
            worst = G.check_case(case)
        except AssertionError as e:
            print(f'CASE {sp.name} FAIL {e}', flush=True)
            return 1
        print(f'CASE {sp.name} kind={kind} ok ratio={worst:.3f}', flush=True)
    if not pp_only and not staged:
        try:
            kind, worst = qknr_case(st)
        except AssertionError as e:
            print(f'CASE qknr 1025x264x128 FAIL {e}', flush=True)
            return 1
        print(f'CASE qknr 1025x264x128 kind={kind} ok ratio={worst:.3f}', flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
