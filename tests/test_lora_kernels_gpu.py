"""tfx_lora_merge / tfx_lora_down / tfx_lora_grad through the C ABI, per element against the float64 restatements, derived bounds and guard bands of
tests/_lora_cases.py.  Every test prints `BOUND <form> <worst error / bound>` lines: profiles/lora_bounds.txt keeps a copy."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from transfusion_pytorch_amd import capi  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lora_cases as C  # noqa: E402
from _gemm_cases import assert_elementwise, assert_untouched, _bits  # noqa: E402

DEV = 'cuda'


def stream():
    return torch.cuda.current_stream().cuda_stream


def call(fn, struct, **kw):
    a = capi.make_args(struct, **kw)
    capi.call(fn, a, stream())
    torch.cuda.synchronize()
    return a


def grad_plan(**kw):
    a = capi.make_args('tfx_lora_grad_args', **kw)
    chunks, grid, floats = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    capi.check(capi.lib().tfx_lora_grad_plan(ctypes.byref(a), ctypes.byref(chunks), ctypes.byref(grid), ctypes.byref(floats)), 'tfx_lora_grad_plan')
    return chunks.value, grid.value, floats.value


def plan_of(M, K, r):
    return grad_plan(M=M, K=K, r=r, r_pad=C.r_pad_of(r), ldp=C.r_pad_of(r), ldq=K)


def smallest_m_with_three_runs(K):
    return next(M for M in range(1, 4096) if plan_of(M, K, 8)[0] >= 3)


def run_grad(c):
    chunks, grid, floats = grad_plan(**c.kw)
    part = torch.full((floats,), float('nan'), device=DEV)                 # every element the sum reads must have been written by the product kernel
    call('tfx_lora_grad', 'tfx_lora_grad_args', partials=part, **c.kw)
    return chunks


def check_grad(name, c):
    worst = assert_elementwise(name, c.pick(c.buf), c.ref, c.tol, (32, 128))
    assert_untouched(name, c.buf, c.before, c.written)
    return worst


# ---------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize('K', C.MERGE_K)
@pytest.mark.parametrize('N', C.MERGE_N)
def test_merge_elementwise_guards_and_zero_b(N, K):
    worst = 0.
    for r in C.RANKS:
        c = C.build_merge(N, K, r, 0.75, DEV)
        call('tfx_lora_merge', 'tfx_lora_merge_args', **c.kw)
        worst = max(worst, assert_elementwise(f'merge {N}x{K} r{r}', c.view, c.ref, c.tol))
        written = torch.zeros(c.buf.shape, dtype=torch.bool, device=DEV)
        written[C.GUARD:C.GUARD + N, :K] = True
        assert_untouched(f'merge {N}x{K} r{r}', c.buf, c.before, written)
        first = c.view.clone()
        call('tfx_lora_merge', 'tfx_lora_merge_args', **c.kw)
        assert torch.equal(first, c.view)
        z = C.build_merge(N, K, r, 0.75, DEV, zero_b=True)
        call('tfx_lora_merge', 'tfx_lora_merge_args', **z.kw)
        assert torch.equal(_bits(z.view), _bits(z.W.contiguous())), 'B = 0 must return W bit for bit (the negative zero included)'
    c = C.build_merge(N, K, 0, 1.0, DEV)                                   # r = 0: the plain copy of the unadapted rows of a fused block
    c.kw.update(A=None, B=None)
    call('tfx_lora_merge', 'tfx_lora_merge_args', **c.kw)
    assert torch.equal(_bits(c.view), _bits(c.W.contiguous()))
    print(f'BOUND lora_merge N={N} K={K} {worst:.3f}')


# ---------------------------------------------------------------------------------------------- down
@pytest.mark.parametrize('K', C.GRAD_K)
@pytest.mark.parametrize('M', C.GRAD_M)
def test_down_elementwise_and_guards(M, K):
    worst = 0.
    for r in C.RANKS:
        c = C.build_down(M, K, r, DEV)
        call('tfx_lora_down', 'tfx_lora_down_args', **c.kw)
        worst = max(worst, assert_elementwise(f'down {M}x{K} r{r}', c.view, c.ref, c.tol, (32, 32)))
        written = torch.zeros(c.buf.shape, dtype=torch.bool, device=DEV)
        written[C.GUARD:C.GUARD + M, :c.kw['r_pad']] = True
        assert_untouched(f'down {M}x{K} r{r}', c.buf, c.before, written)
        assert not bool(c.view[:, r:].any()), 'zero rows of R give zero columns of P'
        first = c.view.clone()
        call('tfx_lora_down', 'tfx_lora_down_args', **c.kw)
        assert torch.equal(first, c.view)
    print(f'BOUND lora_down M={M} K={K} {worst:.3f}')


# ---------------------------------------------------------------------------------------------- grad
def test_grad_plan_row_runs():
    for K in C.GRAD_K:
        m3 = smallest_m_with_three_runs(K)
        assert plan_of(m3, K, 8)[0] >= 3 and plan_of(m3 - 1, K, 8)[0] < 3
        for M in C.GRAD_M + (m3,):
            for r in C.RANKS:
                chunks, grid, floats = plan_of(M, K, r)
                kt = -(-K // 128)
                assert chunks >= 1 and grid == chunks * kt and floats == chunks * C.r_pad_of(r) * kt * 128
    a = capi.make_args('tfx_lora_grad_args', M=64, K=60, r=8, r_pad=32, ldp=32, ldq=64)
    assert capi.lib().tfx_lora_grad_plan(ctypes.byref(a), None, None, None) != 0, 'K % 8 != 0 is refused'
    a = capi.make_args('tfx_lora_grad_args', M=64, K=64, r=65, r_pad=64, ldp=64, ldq=64)
    assert capi.lib().tfx_lora_grad_plan(ctypes.byref(a), None, None, None) != 0, 'rank above 64 is refused'


@pytest.mark.parametrize('K', C.GRAD_K)
@pytest.mark.parametrize('M', C.GRAD_M + ('three-runs',))
def test_grad_elementwise_guards_accumulate_and_repeat(M, K):
    if M == 'three-runs':
        M = smallest_m_with_three_runs(K)
    worst = 0.
    for r in C.RANKS:
        for acc in (0, 1):
            c = C.build_grad(M, K, r, alpha=0.75, accumulate=acc, device=DEV)
            chunks = run_grad(c)
            worst = max(worst, check_grad(f'grad {M}x{K} r{r} acc{acc} ({chunks} runs)', c))
            # the same call twice: from the same initial G the same bits
            first = c.buf.clone()
            c.buf.copy_(c.before)
            run_grad(c)
            assert torch.equal(_bits(first), _bits(c.buf))
    print(f'BOUND lora_grad M={M} K={K} {worst:.3f}')


@pytest.mark.parametrize('acc', (0, 1))
def test_grad_transposed_mapped_store(acc):
    """dB's form: element (j, k) at G[colmap[k]][j], dropped columns and every other element of the buffer untouched"""
    worst = 0.
    for (M, K, r) in ((192, 200, 8), (1000, 520, 24), (70, 64, 64)):
        c = C.build_grad(M, K, r, alpha=2.0, accumulate=acc, device=DEV, mapped=True)
        run_grad(c)
        worst = max(worst, check_grad(f'grad mapped {M}x{K} r{r} acc{acc}', c))
    print(f'BOUND lora_grad mapped acc={acc} {worst:.3f}')


def test_down_then_grad_composed_bound():
    """U = X A^T through tfx_lora_down, dB^T = s U^T dY through tfx_lora_grad, against float64 from X, A, dY alone: the bound carries the one bf16 rounding of U"""
    worst = 0.
    for (M, K, N, r) in ((1000, 200, 520, 8), (192, 520, 64, 64)):
        d = C.build_down(M, K, r, DEV)
        call('tfx_lora_down', 'tfx_lora_down_args', **d.kw)
        c = C.build_grad(M, N, r, alpha=0.5, accumulate=0, device=DEV, P=d.view)
        run_grad(c)
        Pex = d.ref                                                        # the exact product, float64
        dP = C.U16 * Pex.abs() + 2 * d.E
        ref = 0.5 * (Pex[:, :r].T @ c.Q.double())
        S = 0.5 * (Pex[:, :r].abs().T @ c.Q.double().abs())
        tol = 0.5 * (dP[:, :r].T @ c.Q.double().abs()) + C.e32(M, S + 0.5 * (dP[:, :r].T @ c.Q.double().abs()))
        worst = max(worst, assert_elementwise(f'down->grad {M}x{K}x{N} r{r}', c.pick(c.buf), ref, tol, (32, 128)))
    print(f'BOUND lora_down_grad composed {worst:.3f}')
