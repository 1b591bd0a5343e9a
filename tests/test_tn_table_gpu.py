"""Weight-gradient table launches on the GPU (tfx.h `table`): the kernel's block -> (product, row chunk, tile) mapping at the smallest shapes where it can go
wrong, and one training step of a small model with the per-layer groups, runs of 2 layers and the whole stack deferred."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from transfusion_pytorch_amd import capi  # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16
REC = capi.STRUCTS['tfx_gemm_tn_args']
TOL = 5e-3                     # the project's TN tolerance (rel-Frobenius against fp32 torch on the bf16 operands), as test_gemm_tn_grouped_launch
LOSS_ULPS = 16                 # see test_model_step_deferred_weight_gradients
C0, B0 = 0.25, 2.0             # C / bias start values: "always accumulates" is part of the contract


def stream():
    return torch.cuda.current_stream().cuda_stream


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def check(name, got, ref, tol):
    assert torch.isfinite(got.float()).all(), f'{name}: non-finite output'
    e = relerr(got, ref)
    print(f'{name}: rel err {e:.3e} (tol {tol})')
    assert e <= tol, f'{name}: rel err {e} > {tol}'


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(BF)


# nine products (the kernel-argument form holds six), 35 tiles: 280 blocks at 8 chunks = a second round of the chip
#   (N, K, feature)
SHAPES = [(512, 512, None), (264, 300, None), (520, 64, None), (300, 520, 'rowmap+colsum'), (512, 128, 'k_group'), (512, 256, 'half0'), (512, 256, 'half1'),
          (768, 512, None), (512, 768, None)]
_CACHE = {}


def problems(M, shapes=tuple(SHAPES)):
    """operands + fp32 references of the products over M rows, built once per (M, shapes) and left unchanged; each entry: (struct kwargs, C shape, reference of
    the product placed in C, bias reference or None)"""
    key = (M, shapes)
    if key in _CACHE:
        return _CACHE[key]
    torch.manual_seed(11)
    out, half_c = [], None
    for N, K, feat in shapes:
        lda, ldb = (N + 7) // 8 * 8, (K + 7) // 8 * 8
        A, B = rnd(M, lda, scale=0.5), rnd(M, ldb, scale=0.5)
        prod = A[:, :N].float().T @ B[:, :K].float()
        kw = dict(A=A, lda=lda, a_cols=lda, B=B, ldb=ldb, b_cols=ldb, M=M, N=N, K=K, ldc=K, k_valid=K, splits=0, accumulate=1, alpha=1.0)
        e = dict(kw=kw, keep=[A, B], cshape=(N, K), ref=prod, bref=None, col0=0)
        if feat == 'rowmap+colsum':
            rowmap = torch.randperm(N, device=DEV).to(torch.int32)
            rowmap[3] = -1
            keep = rowmap >= 0
            ref = torch.zeros(N, K, device=DEV); ref[rowmap[keep].long()] = prod[keep]
            bref = torch.zeros(N, device=DEV); bref[rowmap[keep].long()] = A[:, :N].float().sum(0)[keep]
            kw.update(rowmap=rowmap)
            e.update(ref=ref, bref=bref); e['keep'].append(rowmap)
        elif feat == 'k_group':
            kg = 48
            kout = K // 64 * kg
            kw.update(k_group=kg, ldc=kout)
            e.update(cshape=(N, kout), ref=prod.view(N, K // 64, 64)[:, :, :kg].reshape(N, kout))
        elif feat in ('half0', 'half1'):                       # two members write the two column halves of ONE C (ldc = 2 K): the skip projection's gradient
            kw.update(ldc=2 * K)
            e.update(cshape=(N, 2 * K), col0=K if feat == 'half1' else 0, shared=True)
        out.append(e)
    _CACHE[key] = out
    return out


def build_table(entries, M, splits, mutate=None):
    """fresh outputs + the table (device bytes, host copy, head struct) over the cached operands"""
    n, rs = len(entries), ctypes.sizeof(REC)
    host = ctypes.create_string_buffer(n * (rs + 4))
    ends = (ctypes.c_int32 * n).from_buffer(host, n * rs)
    outs, tiles, shared_c = [], 0, None
    for k, e in enumerate(entries):
        kw = dict(e['kw'])
        if e.get('shared'):
            if e['col0'] == 0 or shared_c is None:
                shared_c = torch.full(e['cshape'], C0, device=DEV)
            C = shared_c
        else:
            C = torch.full(e['cshape'], C0, device=DEV)
        bias = torch.full((e['cshape'][0],), B0, device=DEV) if e['bref'] is not None else None
        kw.update(C=C.data_ptr() + 4 * e['col0'], colsum=bias)
        if mutate:
            mutate(k, kw)
        a = capi.make_args('tfx_gemm_tn_args', **kw)
        ctypes.memmove(ctypes.addressof(host) + k * rs, ctypes.addressof(a), rs)
        tiles += -(-kw['N'] // 256) * -(-kw['K'] // 256)
        ends[k] = tiles
        outs.append((C, bias, kw))
    dev = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(DEV)
    head = REC.from_buffer_copy(host, 0)
    head.table, head.table_host, head.table_count, head.splits = dev.data_ptr(), ctypes.addressof(host), n, splits
    head._keep = (host, dev)
    return head, outs, tiles


def plan_of(head):
    out = [ctypes.c_int32(-9) for _ in range(4)]
    assert capi.lib().tfx_gemm_tn_plan(ctypes.byref(head), *[ctypes.byref(o) for o in out]) == 0
    return tuple(o.value for o in out)


def run_and_check(name, entries, head, outs):
    capi.call('tfx_gemm_tn', head, stream())
    torch.cuda.synchronize()
    for k, (e, (C, bias, kw)) in enumerate(zip(entries, outs)):
        K = e['ref'].shape[1]
        got = C[:, e['col0']:e['col0'] + K]
        check(f'{name} member {k} {kw["N"]}x{kw["K"]}', got, e['ref'] + C0, TOL)
        if e['bref'] is not None:
            check(f'{name} member {k} bias grad', bias, e['bref'] + B0, TOL)


@pytest.mark.parametrize('splits', [1, 2, 3, 8])
def test_table_forced_chunks(splits):
    """nine products at M = 1536 with 1, 2, 3 and 8 row chunks (8 x 192 rows: the shortest legal chunk, and 280 blocks: a second round of the chip): ragged last
    tiles in N and K, a narrow product, row map + folded bias gradient, compacted per-head columns, two members on the halves of one C.  Outputs start non-zero."""
    M = 1536
    entries = problems(M)
    head, outs, tiles = build_table(entries, M, splits)
    assert tiles == 35
    assert plan_of(head) == (3, tiles, splits, (tiles * splits + 7) // 8 * 8)
    run_and_check(f'table M={M} chunks={splits}', entries, head, outs)


def test_table_ragged_last_chunk():
    """M = 832 at 2 chunks: 448 rows + a last chunk of 384"""
    M = 832
    entries = problems(M)
    head, outs, tiles = build_table(entries, M, 2)
    assert plan_of(head) == (3, tiles, 2, (tiles * 2 + 7) // 8 * 8)
    run_and_check(f'table M={M} chunks=2', entries, head, outs)


def test_table_library_chosen_chunks():
    """splits = 0: the plan the launch runs is kind 3 over the summed tiles, with chunks of >= 256 rows"""
    M = 1536
    entries = problems(M)
    head, outs, tiles = build_table(entries, M, 0)
    kind, t, s, grid = plan_of(head)
    assert (kind, t) == (3, tiles) and s >= 1 and -(-M // s) >= 256 and grid == (tiles * s + 7) // 8 * 8
    run_and_check(f'table M={M} library chunks ({s})', entries, head, outs)


@pytest.mark.parametrize('case', ['a_rowmap', 'other_M', 'M1000'])
def test_table_fallbacks(case):
    """tables with a member the one-wave kernel does not take run record by record - same results, and the plan is not kind 3"""
    shapes = tuple(SHAPES[:4])
    if case == 'M1000':
        M = 1000
        entries = problems(M, shapes)
        head, outs, tiles = build_table(entries, M, 0)
    elif case == 'a_rowmap':
        M = 1536
        entries = problems(M, shapes)
        ident = torch.arange(M, device=DEV, dtype=torch.int32)
        head, outs, tiles = build_table(entries, M, 0, mutate=lambda k, kw: kw.update(a_rowmap=ident) if k == 1 else None)
        head._keep += (ident,)
    else:
        M = 1536
        entries = [dict(e) for e in problems(M, shapes)]
        small = problems(768, (SHAPES[2],))[0]
        entries[2] = small                                                 # one member over 768 rows
        head, outs, tiles = build_table(entries, M, 0)
    assert plan_of(head)[0] != 3
    run_and_check(f'table fallback {case}', entries, head, outs)


# ---------------------------------------------------------------------------------------------- model level
def _step(sd, batch, times, noise, run, dp_groups, monkeypatch):
    from transfusion_pytorch_amd import Transfusion
    monkeypatch.setenv('TFX_TN_DEFER', str(run))
    m = Transfusion(num_text_tokens=32, dim_latent=(16, 8), transformer=dict(dim=64, depth=5, heads=1), prob_uncond=0.)
    m.load_state_dict(sd)
    m = m.cuda().train()
    if dp_groups:
        m._dp_groups = dp_groups
    m._noise_override = {t: v.clone() for t, v in noise.items()}
    loss = m(batch, times=times)
    loss.backward()
    torch.cuda.synchronize()
    plan = next(p for p in m._plans.values() if getattr(p, 'bwd', None) is not None and len(p.bwd))
    grads = {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}
    return float(loss), grads, plan


@pytest.mark.parametrize('dp_groups', [0, 2])
def test_model_step_deferred_weight_gradients(dp_groups, monkeypatch):
    """depth 5 (U-Net skips into the upper layers), dim 64, two modality types, b 4 x n 128 (T = 512): one training step from identical weights and
    inputs with run length 0, 2 and all.  The forward is the same list, so the loss is equal - up to the last bits: the loss kernels add their per-block partial
    sums with fp32 atomics (tokenwise.hip, `atomicAdd(p.acc, ...)`), so two replays of the SAME list already differ in the last bits (measured on MI355X, printed
    below: the run-length-0 step twice 0.5 and 1.0 ulp apart; run length 2 against 0: 2 ulp).  Bound: LOSS_ULPS = 16 fp32 ulp, the order-of-summation error of <= 128 block partials of like sign
    (~sqrt(128) / 2 ulp typical, 6; doubled and rounded up) - a forward that differed in anything but that order would be off by far more.  Only the order of the
    fp32 sums of the weight gradients differs otherwise: every parameter gradient within 1e-3 rel-Frobenius of the run-length-0 gradients.  With dp_groups = 2 runs
    stop at the exchange cuts, whose number is unchanged.  Measured worst parameter: 8.2e-7 (run length all), 7.1e-7 (2)."""
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(5)
    base = Transfusion(num_text_tokens=32, dim_latent=(16, 8), transformer=dict(dim=64, depth=5, heads=1), prob_uncond=0.)
    sd = {k: v.detach().clone() for k, v in base.state_dict().items()}
    g = torch.Generator(device='cuda').manual_seed(3)
    T_ = lambda n: torch.randint(0, 32, (n,), device='cuda', generator=g)
    Lt = lambda t, n: (t, torch.randn(n, (16, 8)[t], device='cuda', generator=g))
    batch = [[T_(20), Lt(0, 30), T_(17), Lt(1, 21), T_(9)], [T_(40), Lt(0, 50)], [Lt(1, 33), T_(60)], [T_(14), Lt(0, 12), T_(26), Lt(0, 16), T_(12), Lt(1, 11)]]
    times = torch.full((4, 3), 0.4, device='cuda')
    noise = {t: torch.randn(sum(p[1].shape[0] for s in batch for p in s if isinstance(p, tuple) and p[0] == t), (16, 8)[t], device='cuda', generator=g)
             for t in (0, 1)}
    ref_loss, ref, plan0 = _step(sd, batch, times, noise, 0, dp_groups, monkeypatch)
    assert plan0.T == 512 and not plan0.tn_tables
    again = _step(sd, batch, times, noise, 0, dp_groups, monkeypatch)[0]
    print(f'dp_groups={dp_groups}: loss {ref_loss!r}; the same run-length-0 step again {again!r} (|diff| = {abs(again - ref_loss) / (1.1920929e-07 * abs(ref_loss)):.1f} fp32 ulp)')
    for run in (2, 'all'):
        loss, grads, plan = _step(sd, batch, times, noise, run, dp_groups, monkeypatch)
        assert len(plan.bwd_cuts) == len(plan0.bwd_cuts)
        want = {(0, 2): 3, (0, 'all'): 1, (2, 2): 3, (2, 'all'): 2}[(dp_groups, run)]          # depth 5: runs of 2 from the top; groups of 3 layers with 2 cuts
        assert len(plan.tn_tables) == want, [t[:3] for t in plan.tn_tables]
        for idx, lo, hi, tab, n in plan.tn_tables:                           # the launches really are table launches of the one-wave kernel
            out = [ctypes.c_int32(-9) for _ in range(4)]
            assert capi.lib().tfx_gemm_tn_plan(ctypes.byref(plan.bwd[idx][1]), *[ctypes.byref(o) for o in out]) == 0
            assert out[0].value == 3, [o.value for o in out]
        assert abs(loss - ref_loss) <= LOSS_ULPS * 1.1920929e-07 * abs(ref_loss), (loss, ref_loss)
        assert grads.keys() == ref.keys()
        worst = max((relerr(grads[k], ref[k]), k) for k in ref if ref[k].norm() > 0)
        print(f'dp_groups={dp_groups} run={run}: {len(plan.tn_tables)} table launches, worst gradient rel err {worst[0]:.3e} ({worst[1]})')
        assert worst[0] <= 1e-3, worst
