"""Bit identity of the 4-wave LDS-DMA NT kernels (csrc/nt_ring.h) between two builds of the library: sha256 of every output buffer of every form-1 / 2 / 4
case of tests/_gemm_cases.py NT_CASES and of the problems of tests/test_muon_gpu.py test_grouped_products_asymmetric_ragged, on their seeded operands.

    python tools/nt_ring_digests.py                    # the listing of the library in use (TFX_LIB or the in-tree build)
    python tools/nt_ring_digests.py LIB_A LIB_B        # one fresh child per library; exit status 1 unless the listings are equal line for line
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
    import torch
    from transfusion_pytorch_amd import capi
    import _gemm_cases as G
    import test_muon_gpu as TM
    st = lambda: torch.cuda.current_stream().cuda_stream
    for sp in G.NT_CASES:
        if sp.form not in (1, 2, 4):
            continue
        case = G.build_nt(sp, 'cuda')
        a = capi.make_args('tfx_gemm_nt_args', epi=capi.ENUMS['TFX_EPI_' + sp.epi], **case.kw)
        kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0 and kind.value == sp.form, sp.name
        capi.call('tfx_gemm_nt', a, st())
        torch.cuda.synchronize()
        for o in case.outs:                                    # whole buffers, guard bands included
            print(f'{sha(o.buf)}  {sp.name} | {o.name}')

    def digest_group(tag, problems, alpha, beta):
        for i, o in enumerate(TM.run_group(problems, alpha, beta)):
            for k in ('C', 'Ct'):
                if o[k] is not None:
                    print(f'{sha(o[k])}  muon {tag}[{i}] {k}')
    TM.check_group = digest_group                              # the test's own problems and generator, hashed instead of checked
    TM.test_grouped_products_asymmetric_ragged()


def main():
    libs = sys.argv[1:]
    if not libs:
        return listing()
    outs = []
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, TFX_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout.splitlines())
        print(f'# {lib}: {len(outs[-1])} buffers')
    print('\n'.join(outs[0]))
    diff = [(a, b) for o in outs[1:] for a, b in zip(outs[0], o) if a != b] + [None for o in outs[1:] if len(o) != len(outs[0])]
    for d in diff:
        print('DIFFERENT:', d)
    print('listings equal line for line' if not diff else f'{len(diff)} lines differ')
    sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
