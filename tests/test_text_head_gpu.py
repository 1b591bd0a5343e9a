"""Chunked text head on the GPU (Transfusion.set_text_head_chunking_, engine.Plan `chunk_rows`): the kernels tfx_ce_fwd / tfx_ce_bwd per element against float64
(cases, restatement and bounds: tests/_text_head_cases.py), and the chunked training step against the reference goldens, the live oracle and the plain step.

Chunked against plain step.  The two steps run the same arithmetic except that the logits product runs over `rows` rows at a time, for which the library may pick
another kernel (another summation order of the 128 .. 512 products of a logit) than for all T: logits differ in their last fp32 bits, isolated elements of the bf16
d logits flip by one ulp, and the weight-gradient sums meet their fp32 atomics in another order.  The size of that gap is not derivable, so it is measured - relative
Frobenius norm of the difference of the loss, of the flat gradient buffer and of the gradient of to_text_logits.weight, on the three fixtures (the figures:
profiles/text_head_chunking.txt; test_fixture_matches_reference_golden_and_the_plain_step prints them) - and the bound is
    max(1e-5, 4 x the largest measured value)
1e-5 being what the suite holds two runs of the same launches to whose fp32 atomics arrive in another order, 4 the room for flips that change with the fixture.
Measured (MI355X): small2 and head8, rows 64 and ragged: at most 9.5e-8 (loss), 3.8e-8 (flat gradient), 7.9e-8 (head weight) - the products agree, the atomics'
order is what differs (plain against plain: 1.3e-8).  text1 (forward_text): loss 4.0e-7, flat gradient 4.82e-3, head weight 1.94e-3, the same in every run: the
plain step writes d logits at grad_scale 1, rounds them to bf16, and scales them by the device scalar 1 / #valid labels in a second pass that rounds again
(tfx_scale_bf16_dev), while tfx_ce_bwd takes that scalar as `scale_dev` and rounds once - one bf16 ulp apart in a fraction of the elements, 2^-9 relative.
One bound from the largest figure would hold the interleaved steps to 1.9e-2 for a difference only forward_text has, so each entry point keeps the bound of
its own largest figure: GAP = max(1e-5, 4 x 9.5e-8) = 1e-5 for forward(), GAP_TEXT = 4 x 4.82e-3 for forward_text()."""
import ctypes
import functools
import gc
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case, build_text_case                   # noqa: E402

import _text_head_cases as C                                           # noqa: E402
import test_frozen_gpu as FZ                                           # noqa: E402  (_golden, _grad_errors, _mean: the goldens' own gradient rule)
import test_model_gpu as TM                                            # noqa: E402  (build_native, compare_losses, rel and the tolerances)
from _gemm_cases import BF, GUARD, assert_elementwise, assert_untouched, guarded          # noqa: E402

DEV = 'cuda'
MEASURED_GAP, MEASURED_GAP_TEXT = 9.5e-8, 4.82e-3          # largest chunked-vs-plain figure on small2 / head8 | on text1 (profiles/text_head_chunking.txt)
GAP, GAP_TEXT = max(1e-5, 4 * MEASURED_GAP), max(1e-5, 4 * MEASURED_GAP_TEXT)
GRAD_EQ = 2e-3              # per-parameter figure of the suite for the same launches under another atomic order (tests/test_checkpointing_gpu.py)
rel = TM.rel


def sync():
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ================================================================================================ 1. the kernels
@functools.lru_cache(maxsize=None)
def _kcase(case):
    """inputs of a case on the device and its float64 reference at scale 1, built once"""
    T, V, ld = case
    lg, lab = C.inputs(T, V, ld, DEV)
    return lg, lab, C.ce_ref(lg, lab, V)


def _args(case, lg, lab, lse, acc, dl=None, grad_scale=1.0, scale_dev=None):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    return capi.make_args('tfx_ce_chunk_args', T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, grad_scale=grad_scale, scale_dev=scale_dev,
                          dlogits=dl, ld_d=ld)


def _run_fwd(case, lg, lab):
    """tfx_ce_fwd into a guarded lse and a prefilled acc: (lse buffer, lse view, acc)"""
    from transfusion_pytorch_amd import capi
    buf, lse = guarded(case[0], 1, torch.float32, DEV, 0)
    acc = torch.tensor(C.ACC_INIT + (9.0, 9.0), device=DEV, dtype=torch.float32)
    capi.call('tfx_ce_fwd', _args(case, lg, lab, lse, acc), _stream())
    sync()
    return buf, lse, acc


def _written(buf, rows):
    w = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    w[GUARD:GUARD + rows] = True
    return w


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_ce_fwd_lse_and_sums_against_float64(case):
    T, V, ld = case
    lg, lab, r = _kcase(case)
    tol_lse, tol_loss, _ = C.bounds(r, V)
    keep = lg.clone()
    buf0, _ = guarded(T, 1, torch.float32, DEV, 0)
    buf, lse, acc = _run_fwd(case, lg, lab)
    worst = assert_elementwise(f'tfx_ce_fwd {case} lse', lse.double(), r.lse[:, None], tol_lse[:, None], tile=(4, 1))
    assert bool((lse[~r.valid] == 0).all()), 'ignored rows get lse 0'
    assert_untouched(f'tfx_ce_fwd {case} lse', buf, buf0, _written(buf, T))
    e_loss = abs(float(acc[0].double()) - (C.ACC_INIT[0] + float(r.loss)))
    print(f'  {C.case_id(case)}: lse worst error / bound {worst:.3f}; sum CE {float(acc[0]):.6f} error / bound {e_loss / float(tol_loss):.3f}; count {float(acc[1])}')
    assert e_loss <= float(tol_loss)
    assert float(acc[1]) == C.ACC_INIT[1] + float(r.count) and acc[2:].tolist() == [9.0, 9.0]
    assert torch.equal(lg.view(torch.int32), keep.view(torch.int32)), 'the forward writes lse and acc only'


@pytest.mark.parametrize('scale_dev', [None, 0.37], ids=['no_scale_dev', 'scale_dev_0.37'])
@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_ce_bwd_dlogits_per_element_against_float64(case, scale_dev):
    """the product's chain: tfx_ce_fwd's own lse feeds tfx_ce_bwd; every element of d logits against the float64 gradient (whose bound carries the forward's)"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg, lab, r1 = _kcase(case)
    gs = 0.0031
    sd = None if scale_dev is None else torch.tensor([scale_dev, 55.0], device=DEV, dtype=torch.float32)
    scale = float(torch.tensor(gs, dtype=torch.float32).double()) * (1.0 if sd is None else float(sd[0].double()))
    r = C.ce_ref(lg, lab, V, scale)
    _, _, tol_d = C.bounds(r, V, scale)
    _, lse, acc = _run_fwd(case, lg, lab)
    acc0, lse0 = acc.clone(), lse.clone()
    buf, dl = guarded(T, ld, BF, DEV, 0)
    before = buf.clone()
    capi.call('tfx_ce_bwd', _args(case, lg, lab, lse, acc, dl, grad_scale=gs, scale_dev=sd), _stream())
    sync()
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tol_d
    worst = assert_elementwise(f'tfx_ce_bwd {case} dlogits', dl.double(), ref, tol, tile=(4, 512))
    assert not bool(dl[:, V:].view(torch.int16).any()) and not bool(dl[~r.valid].view(torch.int16).any()), 'pad columns and ignored rows: zero bits'
    assert_untouched(f'tfx_ce_bwd {case} dlogits', buf, before, _written(buf, T))
    assert torch.equal(acc, acc0) and torch.equal(lse, lse0), 'the backward writes d logits only'
    print(f'  {C.case_id(case)} scale_dev {scale_dev}: d logits worst error / bound {worst:.3f}')


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_all_ignored_chunk_leaves_acc_untouched(case):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg = torch.full((T, ld), float('nan'), device=DEV)
    lab = torch.full((T,), -1, device=DEV, dtype=torch.int32)
    _, lse, acc = _run_fwd(case, lg, lab)
    assert acc.tolist() == list(C.ACC_INIT) + [9.0, 9.0] and not bool(lse.view(torch.int32).any())
    buf, dl = guarded(T, ld, BF, DEV, 0)
    before = buf.clone()
    capi.call('tfx_ce_bwd', _args(case, lg, lab, lse, acc, dl, grad_scale=1.0), _stream())
    sync()
    assert not bool(dl.view(torch.int16).any())
    assert_untouched(f'tfx_ce_bwd {case} all ignored', buf, before, _written(buf, T))


@pytest.mark.parametrize('case', C.FUSED_CASES, ids=C.case_id)
def test_ce_bwd_and_the_fused_kernel_sit_inside_the_same_bound(case):
    """tfx_ce_fwd_bwd on the same logits: its d logits and its sums under the bounds of the split kernels (no equal bits: it forms lse in another order)"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg, lab, _ = _kcase(case)
    lg = torch.where(torch.isnan(lg), torch.zeros_like(lg), lg)             # (the fused kernel's fast path loads an ignored row's logits)
    gs = 0.0031
    scale = float(torch.tensor(gs, dtype=torch.float32).double())
    r = C.ce_ref(lg, lab, V, scale)
    _, tol_loss, tol_d = C.bounds(r, V, scale)
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tol_d
    _, lse, acc = _run_fwd(case, lg, lab)
    _, dl = guarded(T, ld, BF, DEV, 0)
    capi.call('tfx_ce_bwd', _args(case, lg, lab, lse, acc, dl, grad_scale=gs), _stream())
    _, dl_f = guarded(T, ld, BF, DEV, 0)
    acc_f = torch.tensor(C.ACC_INIT, device=DEV, dtype=torch.float32)
    capi.call('tfx_ce_fwd_bwd', capi.make_args('tfx_ce_args', T=T, V=V, logits=lg, ld=ld, labels=lab, grad_scale=gs, dlogits=dl_f, ld_d=ld, acc=acc_f), _stream())
    sync()
    w_s = assert_elementwise(f'tfx_ce_bwd {case}', dl.double(), ref, tol, tile=(4, 512))
    w_f = assert_elementwise(f'tfx_ce_fwd_bwd {case}', dl_f.double(), ref, tol, tile=(4, 512))
    print(f'  {C.case_id(case)}: worst error / bound split {w_s:.3f} fused {w_f:.3f}')
    for a in (acc, acc_f):
        assert abs(float(a[0].double()) - (C.ACC_INIT[0] + float(r.loss))) <= float(tol_loss) and float(a[1]) == C.ACC_INIT[1] + float(r.count)


# ================================================================================================ 2. the model
def _native(cfg, sd, rows=None):
    m = TM.build_native(cfg, sd).train()
    return m.set_text_head_chunking_(rows) if rows else m


def _grads(model):
    return {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}


def _snap(model, loss):
    """what the chunked-vs-plain comparison reads of a finished step"""
    sync()
    ps = model.store
    head = ps.grad_view('to_text_logits.weight').clone() if ps.params['to_text_logits.weight'].grad is not None else None
    return dict(loss=float(loss.detach()), flat=ps.grad.clone(), head=head, grads=_grads(model))


def _gap(a, b):
    """(loss, flat gradient buffer, d to_text_logits.weight): relative differences of step `a` against step `b`"""
    return (abs(a['loss'] - b['loss']) / abs(b['loss']), rel(a['flat'], b['flat']), rel(a['head'], b['head']) if b['head'] is not None else 0.)


def _assert_gap(a, b, what, bound=None):
    g = _gap(a, b)
    print(f'  CHUNKGAP {what}: loss {g[0]:.3e} flat gradient {g[1]:.3e} d to_text_logits.weight {g[2]:.3e}   (bound {bound or GAP:.1e})')
    assert set(a['grads']) == set(b['grads']) and a['grads'], what
    assert max(g) <= (bound or GAP), (what, g)
    return g


def _ragged_rows(T):
    """a chunk size (a multiple of 64 above 64) that leaves a ragged last chunk, or None"""
    return next((r for r in (128, 192, 256, 320) if T % r and T > r), None)


def _fixture_step(name):
    """(model factory, step function, golden) of a fixture: step(model) runs forward + backward, returns (loss, breakdown or None)"""
    g = FZ._golden(name)
    if name == 'text1':
        cfg, sd, text = build_text_case(name)
        return (lambda rows: _native(cfg, sd, rows)), (lambda m: (lambda l: (l.backward(), (l, None))[1])(m.forward_text(text))), g
    cfg, sd, batch, times, noise = build_case(name)

    def make(rows):
        m = _native(cfg, sd, rows)
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        return m

    def step(m):
        loss, bd = m(batch, times=times, return_breakdown=True)
        loss.backward()
        return loss, bd
    return make, step, g


@functools.lru_cache(maxsize=None)
def _plain(name):
    make, step, _ = _fixture_step(name)
    m = make(None)
    loss, _ = step(m)
    s = _snap(m, loss)
    assert m._live[0].chunk is None
    return s, m._live[0].T


@pytest.mark.parametrize('name,rows', [('text1', 64), ('small2', 64), ('small2', 'ragged'), ('head8', 64), ('head8', 'ragged')])
def test_fixture_matches_reference_golden_and_the_plain_step(name, rows):
    """(a) loss and gradients under the gates the fixture has against the reference (tests/test_model_gpu.py: LOSS_TOL / 2e-3 for forward_text, GRAD_TOL or norm +
    GRAD_HEAD_TOL per parameter, GRAD_MEAN_TOL norm-weighted); (b) the same step against the plain one.  T of the interleaved fixtures is a multiple of 64 (training
    lengths are bucketed), so they also run a chunk size that leaves a ragged tail; forward_text's 3 x 97 rows are ragged as they are."""
    make, step, g = _fixture_step(name)
    plain, T = _plain(name)
    if rows == 'ragged':
        rows = _ragged_rows(T)
        assert rows, f'{name}: T = {T} has no ragged chunking'
    m = make(rows)
    loss, bd = step(m)
    s = _snap(m, loss)
    plan = m._live[0]
    chunks = plan._chunks()
    assert plan.chunk == rows and not hasattr(plan, 'logits') and not hasattr(plan, 'dlogits')
    assert len(chunks) >= 3 if rows == 64 else (len(chunks) >= 2 and chunks[-1][1] < rows)
    assert name != 'text1' or chunks[-1][1] < rows
    print(f'  [{name}] T {T} rows {rows}: {len(chunks)} chunks, last {chunks[-1][1]} rows')
    if name == 'text1':
        assert abs(s['loss'] - float(g['loss'])) <= 2e-3 * max(1., abs(float(g['loss'])))
    else:
        TM.compare_losses(dict(loss=s['loss'], text=float(bd.text), flow=[float(f) for f in bd.flow]), g)
    errs = FZ._grad_errors(m, g, [k for k, _ in m.named_parameters() if k in g['grad_norms']])
    assert errs and FZ._mean(errs) <= TM.GRAD_MEAN_TOL
    print(f'  [{name}] gradients against the golden: norm-weighted mean {FZ._mean(errs):.3e}, worst {max(e for e, _ in errs.values()):.3e}')
    _assert_gap(s, plain, f'{name} rows {rows}', GAP_TEXT if name == 'text1' else GAP)


def test_wider_vocabulary_matches_live_oracle():
    """5000 text tokens (5134 columns: the wide kernels), dim 128, depth 2, two samples of about 200 tokens with one modality each, rows = 128: four chunks -
    against the CPU oracle by the rule of tests/test_model_gpu.py::test_odd_configurations_match_live_oracle"""
    from oracle import detdata as D
    from oracle.cases import with_grad
    from oracle.transfusion_oracle import OracleConfig, forward_train
    cfg = OracleConfig(num_text_tokens=5000, dim=128, depth=2, dim_latents=(16,), heads=2, dim_head=64)
    tx = lambda key, n: D.det_randint(f'chunk/{key}', (n,), 0, 5000)
    batch = [[tx('a', 90), (0, D.det_normalish('chunk/m0', (2, 3, 16))), tx('b', 100)],
             [tx('c', 150), (0, D.det_normalish('chunk/m1', (5, 16))), tx('d', 40)]]
    times = D.det_uniform('chunk/t', (2, 1), 0.05, 0.95)
    noise = {0: D.det_normalish('chunk/n0', (11, 16))}
    sd = D.det_state_dict(cfg.state_dict_shapes(), tag='chunk')
    sdg = with_grad(sd)
    ref = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    ref['loss'].backward()
    model = _native(cfg, sd, 128)
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss = model(batch, times=times)
    loss.backward()
    sync()
    plan = model._live[0]
    assert plan.chunk == 128 and plan.T >= 3 * 128 and plan.md.vp > C.WIDE_LD
    lo, lr = float(loss.detach()), float(ref['loss'].detach())
    print(f'  loss native {lo:.6f} oracle {lr:.6f}; T {plan.T}, {len(plan._chunks())} chunks of {plan.md.vp} columns')
    assert abs(lo - lr) <= 2e-3 * max(1., abs(lr))
    wsum = nsum = 0.
    for k, p in model.named_parameters():
        gr = sdg[k].grad if sdg[k].requires_grad else None
        if gr is None or float(gr.norm()) < 1e-7:
            continue
        e = rel(p.grad, gr)
        assert e <= TM.GRAD_HEAD_TOL, (k, e)
        wsum += e * float(gr.norm()); nsum += float(gr.norm())
    print(f'  gradients: norm-weighted mean rel err {wsum / nsum:.3e}')
    assert wsum / nsum <= TM.GRAD_MEAN_TOL


def test_rows_at_least_T_is_one_chunk():
    make, step, _ = _fixture_step('small2')
    plain, T = _plain('small2')
    m = make(4096)
    loss, _ = step(m)
    plan = m._live[0]
    assert T < 4096 and plan.chunk == T and plan._chunks() == [(0, T)] and tuple(plan.logits_c.shape) == (T, plan.md.vp)
    _assert_gap(_snap(m, loss), plain, 'small2 rows 4096 (one chunk)')


def test_peak_memory_falls_by_the_head_buffers():
    """a condition, not a measurement: 8192 text tokens x an 8192-token vocabulary in chunks of 1024 rows - the step's peak falls by at least 0.9 of the
    6 (T - rows) vp bytes of logits and d logits the plan no longer holds, less the 4 T of `ce_lse` (0.9: allocator rounding).  A fresh model per arm."""
    from transfusion_pytorch_amd import Transfusion
    rows, b, n = 1024, 8, 1024
    text = torch.randint(0, 8192, (b, n + 1), generator=torch.Generator().manual_seed(3))
    peaks, vp = {}, None
    for arm in ('plain', 'chunked'):
        gc.collect(); torch.cuda.empty_cache(); sync()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        m = Transfusion(num_text_tokens=8192, dim_latent=16, transformer=dict(dim=128, depth=2, heads=2, dim_head=64)).cuda().train()
        if arm == 'chunked':
            m.set_text_head_chunking_(rows)
        for it in range(2):                                            # a warm-up step, then the measured one
            if it == 1:
                sync(); torch.cuda.reset_peak_memory_stats()
            for p in m.parameters():
                p.grad = None
            m.forward_text(text).backward()
            sync()
        peaks[arm] = torch.cuda.max_memory_allocated() - base
        plan = m._live[0]
        assert plan.T == b * n and (plan.chunk == rows) == (arm == 'chunked')
        vp = plan.md.vp
        del m, plan
    T = b * n
    want = 6 * (T - rows) * vp - 4 * T
    print(f'  peak plain {peaks["plain"] / 2 ** 20:.1f} MiB chunked {peaks["chunked"] / 2 ** 20:.1f} MiB: saved {(peaks["plain"] - peaks["chunked"]) / 2 ** 20:.1f} of {want / 2 ** 20:.1f} MiB')
    assert peaks['plain'] - peaks['chunked'] >= 0.9 * want


def _fingerprint(lst):
    from transfusion_pytorch_amd import capi
    fp = ctypes.c_int64()
    assert capi.lib().tfx_list_fingerprint(lst.native(), len(lst), ctypes.byref(fp)) == 0
    return fp.value


def _clear(m):
    for p in m.parameters():
        p.grad = None


def test_switch_set_and_cleared_leaves_the_plain_lists_as_they_were():
    make, step, _ = _fixture_step('small2')
    m = make(None)
    l0, _ = step(m); sync()
    P = m._live[0]
    fp0 = (_fingerprint(P.fwd), _fingerprint(P.bwd))                   # before the switch was ever set
    m.set_text_head_chunking_(64)
    _clear(m); step(m); sync()
    Q = m._live[0]
    assert Q is not P and Q.chunk == 64 and P.chunk is None
    assert sum(p is P for p in m._plans.values()) == 1 and sum(p is Q for p in m._plans.values()) == 1, 'both plans sit in the cache'
    m.set_text_head_chunking_(None)
    _clear(m); l2, _ = step(m); sync()
    assert m._live[0] is P and (_fingerprint(P.fwd), _fingerprint(P.bwd)) == fp0
    l0, l2 = float(l0.detach()), float(l2.detach())
    assert abs(l2 - l0) <= 1e-6 * max(1., abs(l0))


# ------------------------------------------------------------------------------------------------ combinations, all on small2 with rows = 64
def _pair(prepare=lambda m: None, run=None, what=''):
    """the same step on a plain and a chunked (rows = 64) small2 model after `prepare(model)`; returns [(model, snapshot)] plain first"""
    make, step, _ = _fixture_step('small2')
    out = []
    for rows in (None, 64):
        m = make(rows)
        prepare(m)
        loss = (run or (lambda mm: step(mm)[0]))(m)
        out.append((m, _snap(m, loss)))
        assert m._live[0].chunk == rows
    return out


def test_frozen_text_head():
    (mp, sp), (mc, sc) = _pair(lambda m: m.store.params['to_text_logits.weight'].requires_grad_(False))
    _assert_gap(sc, sp, 'to_text_logits.weight frozen')
    assert mc.store.params['to_text_logits.weight'].grad is None and not bool(mc.store.grad_view('to_text_logits.weight').view(torch.int32).any())
    ops = [fn if isinstance(fn, str) else fn.__name__ for fn, _ in mc._live[0].bwd]
    n = len(mc._live[0]._chunks())
    assert ops[:3 * n] == ['tfx_gemm_nt', 'tfx_ce_bwd', 'tfx_gemm_nt'] * n, 'no weight-gradient product in a chunk'


def test_everything_frozen_launches_nothing():
    make, step, _ = _fixture_step('small2')
    m = make(64)
    for p in m.parameters():
        p.requires_grad_(False)
    _, _, batch, times, _ = build_case('small2')
    loss = m(batch, times=times)
    plan = m._live[0]
    mark = torch.full_like(plan.dembed, 7.)
    plan.dembed.copy_(mark)
    plan.dlogits_c.fill_(3.)
    if loss.requires_grad:
        (loss * 3.).backward()
    sync()
    assert plan.chunk == 64 and plan.bwd_end == 0
    assert torch.equal(plan.dembed, mark) and bool((plan.dlogits_c == 3.).all()) and float(plan.go_dev) == 1.0, 'a backward with nothing trainable launched something'
    assert all(p.grad is None for p in m.store.params.values()) and not bool(m.store.grad.view(torch.int32).any())


def test_with_activation_checkpointing():
    make, step, _ = _fixture_step('small2')
    plain, _ = _plain('small2')
    m = make(64).set_activation_checkpointing_(True)
    loss, _ = step(m)
    plan = m._live[0]
    assert plan.ckpt and plan.chunk == 64 and plan._recompute
    _assert_gap(_snap(m, loss), plain, 'checkpointing + chunking')


def test_two_accumulated_backward_passes_then_fused_adam():
    from transfusion_pytorch_amd.optim import FusedAdam
    make, _, _ = _fixture_step('small2')
    _, _, batch, times, _ = build_case('small2')
    res = []
    for rows in (None, 64):
        m = make(rows)
        opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
        with opt.no_sync():
            m(batch, times=times).backward()
        m(batch, times=times).backward()
        sync()
        g = m.store.grad.clone()
        opt.step(); sync()
        assert m._live[0].chunk == rows
        res.append((g, m.store.flat.clone()))
    (g0, p0), (g1, p1) = res
    print(f'  CHUNKGAP accumulation: gradient buffer {rel(g1, g0):.3e}; parameters after the step {rel(p1, p0):.3e}')
    assert rel(g1, g0) <= GAP and rel(p1, p0) <= 1e-5


def test_half_loss_backward_halves_every_gradient():
    """(0.5 loss).backward(): the upstream gradient reaches tfx_ce_bwd through `scale_dev` and the flow seeds through tfx_scale_bf16_dev.  A factor of 0.5 is exact
    in every rounding on the way, so the gradients are half of the plain backward's up to the order of the fp32 atomics: the suite's GRAD_EQ per parameter"""
    make, step, _ = _fixture_step('small2')
    _, _, batch, times, _ = build_case('small2')
    grads = []
    for f in (1.0, 0.5):
        m = make(64)
        loss = m(batch, times=times)
        (f * loss).backward()
        sync()
        assert abs(float(m._live[0].go_dev) - f) == 0
        grads.append(_grads(m))
    worst = max((rel(2. * grads[1][k], grads[0][k]), k) for k in grads[0] if float(grads[0][k].norm()) > 1e-7)
    print(f'  2 x gradients of (0.5 loss) against those of loss: worst {worst[0]:.3e} ({worst[1]})')
    assert set(grads[0]) == set(grads[1]) and worst[0] <= GRAD_EQ


def test_second_backward_still_raises():
    make, _, _ = _fixture_step('small2')
    _, _, batch, times, _ = build_case('small2')
    m = make(64)
    loss = m(batch, times=times)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()


def test_hidden_taps():
    import _self_flow_cases as SF
    g = torch.load(os.path.join(TM.GOLDEN, f'{SF.TAPS_FIXTURE}.pt'), weights_only=False)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    taps = list(SF.tap_indices(cfg.depth))
    res = []
    for rows in (None, 64):
        m = _native(cfg, sd, rows)
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        loss, hiddens = m(batch, times=times, return_hiddens=True)
        total = loss
        for k in taps:
            total = total + g['taps'][k]['w'] * hiddens[k].pow(2).mean()
        total.backward()
        res.append(_snap(m, loss))
        assert m._live[0].chunk == rows
    _assert_gap(res[1], res[0], f'hidden taps {taps}')


def test_training_graph_replay(monkeypatch):
    """TFX_TRAIN_GRAPH (in process, as tests/test_model_gpu.py and tests/test_checkpointing_gpu.py switch it): from the third identical step both lists of the
    chunked plan replay as graphs - `go_dev` is a fixed address, so the backward's fingerprint holds - and every step equals the plain step"""
    from transfusion_pytorch_amd import engine
    make, step, _ = _fixture_step('small2')
    plain, _ = _plain('small2')
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    m = make(64)
    for k in range(5):
        _clear(m)
        loss, _ = step(m); sync()
        plan = m._live[0]
        if k >= 2:
            st_f, st_b = plan.fwd._auto[(0, len(plan.fwd))], plan.bwd._auto[(0, len(plan.bwd))]
            assert st_f[1] and st_b[1], 'from the third identical step both lists replay as graphs'
        _assert_gap(_snap(m, loss), plain, f'TFX_TRAIN_GRAPH step {k}')
    assert plan.chunk == 64 and plan.bwd._auto[(0, len(plan.bwd))][2] >= 4
