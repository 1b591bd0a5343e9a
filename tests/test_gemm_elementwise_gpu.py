"""Every GEMM kernel form per element: tfx_gemm_nt (plan kinds 0-7, six epilogues + QKV_NORM_ROPE, split / row-gathered A, scattered output rows, the
in-place residual) and tfx_gemm_tn (kinds -1, 0, 2, 3, a `group_next` chain, a device table) against the fp64 reference, the derived per-element bound and
the guard bands of tests/_gemm_cases.py - whose CPU test (tests/test_gemm_refs_cpu.py) shows what this catches that a whole-matrix ratio does not.  Every
case first asserts its kind through the planner: a shape that moves to another kernel fails there.  lda / ldb / ldc / ldc2 / ldr / ldaux are all wider than
the rows they hold."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from transfusion_pytorch_amd import capi  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as G  # noqa: E402

DEV = 'cuda'


def stream():
    return torch.cuda.current_stream().cuda_stream


def tn_plan(a):
    out = [ctypes.c_int32(-9) for _ in range(4)]
    assert capi.lib().tfx_gemm_tn_plan(ctypes.byref(a), *[ctypes.byref(o) for o in out]) == 0
    return tuple(o.value for o in out)


@pytest.mark.parametrize('form', [5, 4, 2, 1, 0])
def test_nt_per_element(form):
    """decode / skinny / mid / LDS-DMA 128 x 128 / register-staged kernels at the smallest shapes that reach them (the covering list NT_CASES)"""
    specs = [sp for sp in G.NT_CASES if sp.form == form]
    assert specs
    worst = {}
    for sp in specs:
        case = G.build_nt(sp, DEV)
        a = capi.make_args('tfx_gemm_nt_args', epi=capi.ENUMS['TFX_EPI_' + sp.epi], **case.kw)
        kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert capi.lib().tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0
        assert kind.value == form, f'{sp.name}: the planner names kind {kind.value}; choose another shape for form {form}'
        capi.call('tfx_gemm_nt', a, stream())
        torch.cuda.synchronize()
        r = G.check_case(case)
        key = 'fp32 out' if sp.epi == 'F32' else 'bf16 out'
        worst[key] = max(worst.get(key, 0.), r)
    print(f'NT kind {form}: {len(specs)} cases, worst error / bound {worst}')


CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_gemm_elementwise_child.py')
SWITCHES = ('TFX_NT_OWP', 'TFX_NT_OW', 'TFX_GEMM_GLDS', 'TFX_NT_PP_MIN', 'TFX_GELU_TABLE')


def run_child(extra, kinds, count):
    """one child under the switches `extra`: exit status 0, one ok line per case, exactly the kinds wanted"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('CASE')]
    print('\n'.join(lines))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert all(' ok ' in ln for ln in lines)
    met = {int(ln.split('kind=')[1].split()[0]) for ln in lines}
    assert met == kinds, f'kinds met {met}, wanted {kinds}'
    assert len(lines) == count
    for k in sorted(met):
        print(f'NT kind {k} (child {extra}): worst error / bound {max(float(ln.split("ratio=")[1]) for ln in lines if f"kind={k} " in ln):.3f}')


def test_nt_256_family_per_element():
    """ping-pong (kind 3) and one-wave kernels (kinds 6, 7) at M = 1025 / 1279 in a child with TFX_NT_PP_MIN=1 (QKV_NORM_ROPE among its cases); a second child
    with TFX_NT_OW=0 runs the plain epilogues on the ping-pong kernel too.  The second child starts only if the first exits 0."""
    run_child({'TFX_NT_PP_MIN': '1'}, {3, 6, 7}, len(G.NT_FAMILY_CASES) + 1)
    run_child({'TFX_NT_PP_MIN': '1', 'TFX_NT_OW': '0'}, {3}, sum(sp.form != 3 for sp in G.NT_FAMILY_CASES))


def test_nt_register_staged_geglu_per_element():
    """GEGLU / GEGLU_BWD on the register-staged kernel (kind 0), which N % 64 == 0 reaches only with TFX_GEMM_GLDS=0: a child of its own"""
    run_child({'TFX_GEMM_GLDS': '0'}, {0}, len(G.NT_STAGED_GEGLU))


@pytest.mark.parametrize('form', [-1, 0, 2, 3])
def test_tn_per_element(form):
    specs = [sp for sp in G.TN_CASES if sp.form == form]
    assert specs
    worst = 0.
    for sp in specs:
        case = G.build_tn(sp, DEV)
        a = capi.make_args('tfx_gemm_tn_args', **case.kw)
        kind = tn_plan(a)[0]
        assert kind == form, f'{sp.name}: the planner names kind {kind}'
        capi.call('tfx_gemm_tn', a, stream())
        torch.cuda.synchronize()
        worst = max(worst, G.check_tn(case))
    print(f'TN kind {form}: {len(specs)} cases, worst error / bound {worst:.3f}')


def test_tn_group_chain_per_element():
    """two products over the same 448 rows as one launch of the one-wave kernel: each member within its own guards"""
    cases = [G.build_tn(sp, DEV) for sp in G.TN_CHAIN]
    structs = [capi.make_args('tfx_gemm_tn_args', **c.kw) for c in cases]
    structs[0].group_next = ctypes.addressof(structs[1])
    tiles = sum(-(-sp.N // 256) * -(-sp.K // 256) for sp in G.TN_CHAIN)
    assert tn_plan(structs[0]) == (3, tiles, 2, (tiles * 2 + 7) // 8 * 8)
    capi.call('tfx_gemm_tn', structs[0], stream())
    torch.cuda.synchronize()
    print(f'TN group chain: worst error / bound {max(G.check_tn(c) for c in cases):.3f}')


def test_tn_table_per_element():
    """three records at M = 512 (different N, K, row map, colsum, k_group) as one table launch; the table bytes come from test_tn_table_gpu.build_table"""
    from test_tn_table_gpu import build_table
    cases = [G.build_tn(sp, DEV) for sp in G.TN_TABLE]
    entries = [dict(kw=c.kw, cshape=(1, 1), bref=None, col0=0) for c in cases]
    head, outs, tiles = build_table(entries, 512, 0, mutate=lambda k, kw: kw.update(C=cases[k].kw['C'], colsum=cases[k].kw.get('colsum')))
    assert tiles == sum(-(-sp.N // 256) * -(-sp.K // 256) for sp in G.TN_TABLE)
    kind, t, s, grid = tn_plan(head)
    assert (kind, t) == (3, tiles) and s in (1, 2) and grid == (tiles * s + 7) // 8 * 8
    capi.call('tfx_gemm_tn', head, stream())
    torch.cuda.synchronize()
    print(f'TN table ({s} chunks): worst error / bound {max(G.check_tn(c) for c in cases):.3f}')
