"""Decode-side, loss and small plumbing kernels through the C ABI against the fp64 references of tests/_decode_loss_cases.py (pinned on the CPU by
tests/test_decode_loss_refs_cpu.py): tfx_sample_tokens(_range) cell by cell, tfx_ode_stage / tfx_ode_update element by element and over a whole staggered
solve, every mode of tfx_mse_fwd_bwd, tfx_output_to_flow, the edges of tfx_ce_fwd_bwd, and the small kernels no other test names.

Every output buffer sits between two guard bands of sentinels (>= one row, >= 64 elements) that are compared bit for bit afterwards; elements a call
must not write carry sentinels too.  All calls stay inside the documented contract; the only zero-size calls are those the wrappers answer with 0
before launching."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _decode_loss_cases import (CE_SHAPES, CFG_SCALE, CLEAN_EPS, F64, MSE_SHAPES, ODE_COEF, ODE_MODES, ODE_SHAPE, SAMPLE_MODES, SAMPLE_SEEDS,  # noqa: E402
                                SAMPLE_SHAPES, SOLVE_S, draw_reference, draw_targets, min_p_margin, mse_inputs, mse_reference, ode_evals, ode_reference,
                                sample_logits, solve_field, solve_fields, solve_pred, solve_rows0, solve_schedule, solve_steps, u_for)
from oracle.shims.torchdiffeq import odeint  # noqa: E402
from transfusion_pytorch_amd import capi  # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16
NAN = float('nan')
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32}
U_TOP = 1. - 2. ** -24                                       # the largest fp32 below 1


def sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    capi.check(getattr(capi.lib(), name)(*args, sp()), name)


def bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


class Guarded:
    """a device buffer of `shape` between two bands of `fill` (one row, at least 64 elements, a multiple of 8: the body stays 16-byte aligned)"""

    def __init__(self, shape, dtype, fill):
        self.n = math.prod(shape)
        self.g = max(64, (shape[-1] + 7) // 8 * 8)
        self.full = torch.full((self.n + 2 * self.g,), fill, dtype=dtype, device=DEV)
        self.t = self.full[self.g:self.g + self.n].view(shape)
        self.fill_bits = bits(self.full[:1]).clone()
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        iv = bits(self.full)
        return bool((iv[:self.g] == self.fill_bits).all()) and bool((iv[self.g + self.n:] == self.fill_bits).all())


def dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------- (a) tfx_sample_tokens / tfx_sample_tokens_range
def sample(entry, lg, ld, B, V, Vd, T, mp, u, active=None):
    """one launch; returns the ids (CPU, long).  The id buffer is guarded and starts at -7."""
    out = Guarded((B,), torch.int32, -7)
    if entry == 'range':
        call('tfx_sample_tokens_range', lg.data_ptr(), ld, B, V, Vd, T, mp, ptr(u), ptr(active), out.t.data_ptr())
    else:
        assert Vd == V
        call('tfx_sample_tokens', lg.data_ptr(), ld, B, V, T, mp, ptr(u), ptr(active), out.t.data_ptr())
    got = out.t.cpu().long()
    assert out.intact(), 'the id buffer\'s guard bands'
    return got


def entries_of(V, Vd):
    return ['range'] + (['plain'] if Vd == V else [])


@pytest.mark.parametrize('B,V,Vd,ld', SAMPLE_SHAPES)
def test_sample_tokens_every_aimed_cell_is_hit_exactly(B, V, Vd, ld):
    """u in the middle of a survivor's cell of the inverse CDF (index order) must return that survivor: first, last, the one behind the longest run of
    filtered columns, the ones nearest the kernel's 64-column trip boundary - cells of >= 1e-3 of the surviving mass, fp32 rounding of u, the mass and
    the prefix sums is below 1e-5 of it.  (V_draw = 1 leaves one survivor, hence one target, per row.)"""
    lg = sample_logits(B, V, Vd, ld, SAMPLE_SEEDS[(B, V, Vd, ld)][0])
    if Vd < V:
        assert bool((lg[::2, :V].argmax(-1) >= Vd).all()), 'every second row: global maximum outside the draw range'
    dlg = dev(lg)
    for T, mp in SAMPLE_MODES:
        assert min_p_margin(lg, V, T, mp) >= 1e-3, 'no column may sit on the min-p threshold'
        keep, q = draw_reference(lg, V, Vd, T, mp)
        tg = draw_targets(keep, q)
        for r in range(B):
            assert len(tg[r]) >= min(2, int(keep[r].sum())) and len(tg[r]) >= 1, (r, tg[r])
        for rnd in range(max(len(t) for t in tg)):
            k = torch.tensor([t[rnd % len(t)] for t in tg])
            u = dev(u_for(q, k))
            for entry in entries_of(V, Vd):
                got = sample(entry, dlg, ld, B, V, Vd, T, mp, u)
                assert torch.equal(got, k), (entry, T, mp, got.tolist(), k.tolist())


@pytest.mark.parametrize('B,V,Vd,ld', SAMPLE_SHAPES)
def test_sample_tokens_edge_uniforms(B, V, Vd, ld):
    """u = 0 returns the first survivor; u = 1 - 2^-24 returns a survivor below V_draw at the very top of the CDF - on 64 rows per launch, so that the
    rows whose fp32 total and fp32 prefix sums disagree (the scan ends without crossing u * mass) are met."""
    n = 64
    lg = sample_logits(n, V, Vd, ld, SAMPLE_SEEDS[(B, V, Vd, ld)][1])
    dlg = dev(lg)
    for T, mp in SAMPLE_MODES:
        assert min_p_margin(lg, V, T, mp) >= 1e-3
        keep, q = draw_reference(lg, V, Vd, T, mp)
        assert bool(keep.any(-1).all())
        cdf = q.cumsum(-1)
        first = keep.int().argmax(-1)
        for entry in entries_of(V, Vd):
            got = sample(entry, dlg, ld, n, V, Vd, T, mp, torch.zeros(n, device=DEV))
            assert torch.equal(got, first), (entry, T, mp)
            got = sample(entry, dlg, ld, n, V, Vd, T, mp, torch.full((n,), U_TOP, device=DEV))
            inside = (got >= 0) & (got < Vd)
            gc = got.clamp(0, Vd - 1)[:, None]
            ok = inside & keep.gather(1, gc)[:, 0] & (cdf.gather(1, gc)[:, 0] / cdf[:, -1] >= 1 - 1e-5)
            print(f'u = 1 - 2^-24 {entry} ({B}, {V}, {Vd}, {ld}) T {T} min_p {mp}: {int((~ok).sum())} of {n} rows off the top of the CDF, '
                  f'{int((~inside).sum())} outside the draw range')
            assert bool(ok.all()), (entry, T, mp, (~ok).nonzero().flatten().tolist(), got[~ok].tolist())


@pytest.mark.parametrize('B,V,Vd,ld', [s for s in SAMPLE_SHAPES if s[2] < s[1]])
def test_sample_tokens_range_without_a_survivor_returns_v_draw(B, V, Vd, ld):
    """the maximum lies outside the draw range and min-p removes every text token: the reference's masked logits are all -finfo.max there and its argmax
    takes the first masked column (T:2697-2698; restated in tests/test_decode_loss_refs_cpu.py)"""
    for T, mp in SAMPLE_MODES:
        if mp == 0.:
            continue
        lg = sample_logits(B, V, Vd, ld, SAMPLE_SEEDS[(B, V, Vd, ld)][0])
        lg[:, V - 1] = lg[:, :Vd].amax(-1) + 2. * (-T * math.log(mp))
        keep, _ = draw_reference(lg, V, Vd, T, mp)
        assert not bool(keep.any())
        u = torch.tensor([(0., 0.5, U_TOP)[r % 3] for r in range(B)])
        got = sample('range', dev(lg), ld, B, V, Vd, T, mp, dev(u))
        assert bool((got == Vd).all()), (T, mp, got.tolist())


@pytest.mark.parametrize('B,V,Vd,ld', SAMPLE_SHAPES)
def test_sample_tokens_range_greedy_and_active_mask(B, V, Vd, ld):
    lg = sample_logits(B, V, Vd, ld, SAMPLE_SEEDS[(B, V, Vd, ld)][0])
    tie = B - 1
    lg[tie, min(5, Vd - 1)] = lg[tie, V - 1] = lg[tie, :V].max() + 1.        # a tie between a text column and the last one: the first index wins
    want = torch.tensor([int((row == row.max()).nonzero()[0]) for row in lg[:, :V]])
    got = sample('range', dev(lg), ld, B, V, Vd, 0., 0.1, None)
    assert torch.equal(got, want), 'temperature 0: argmax over all V columns, first index on ties'
    T, mp = SAMPLE_MODES[0]
    assert min_p_margin(lg, V, T, mp) >= 1e-3
    keep, q = draw_reference(lg, V, Vd, T, mp)
    assert bool(keep.any(-1).all())
    first = keep.int().argmax(-1)
    act = torch.tensor([r % 2 == 0 for r in range(B)])
    got = sample('range', dev(lg), ld, B, V, Vd, T, mp, torch.zeros(B, device=DEV), dev(act, torch.int32))
    assert torch.equal(got, torch.where(act, first, torch.full_like(first, -7))), 'rows with active == 0 keep their value'


# ---------------------------------------------------------------------------------------------- (b) tfx_ode_stage / tfx_ode_update
def ode_rows0(B, H, Lc, seed):
    """a compacted table: blocks in shuffled order; sample 3 (finished) without its conditional half, sample 4 (first evaluation) without its null-text
    half (H == 2) or without its only half (H == 1)"""
    neg = {(0, 3), (1, 4) if H == 2 else (0, 4)}
    live = [(h, i) for h in range(H) for i in range(B) if (h, i) not in neg]
    order = torch.randperm(len(live), generator=torch.Generator().manual_seed(seed)).tolist()
    rows0 = [-1] * (H * B)
    for slot, k in enumerate(order):
        h, i = live[k]
        rows0[h * B + i] = slot * Lc
    return rows0, len(live) * Lc


@pytest.mark.parametrize('use_sel', [False, True])
@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('dl', [12, 5])
def test_ode_stage_and_update_element_by_element(dl, H, compact, use_sel):
    B, Lc, Lq, dmax = (ODE_SHAPE[k] for k in ('B', 'Lc', 'Lq', 'dmax'))
    assert B * Lc * dmax > 256, 'more than one block'
    g = torch.Generator().manual_seed(3)
    y, ym = torch.randn(B, Lc, dmax, generator=g), torch.randn(B, Lc, dmax, generator=g)
    y[:, :, dl:] = NAN; ym[:, :, dl:] = NAN                  # columns the calls must neither read nor write
    ctl = torch.tensor([ODE_MODES, ODE_COEF], dtype=torch.float32)
    rows0, n_rows = ode_rows0(B, H, Lc, seed=5) if compact else (None, H * B * Lq)
    sel = [1., 1., 1., 1., 0.] if use_sel else None
    cfg = 2.5
    pred = torch.randn(n_rows, dl, generator=g)
    Y, Ym, X = Guarded((B, Lc, dmax), torch.float32, NAN), Guarded((B, Lc, dmax), torch.float32, NAN), Guarded((n_rows, dl), torch.float32, NAN)
    Y.t.copy_(y); Ym.t.copy_(ym)
    d_ctl, d_rows0, d_sel, d_pred = dev(ctl), dev(None if rows0 is None else torch.tensor(rows0, dtype=torch.int32)), dev(None if sel is None else torch.tensor(sel)), dev(pred)

    call('tfx_ode_stage', Y.t.data_ptr(), Ym.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
    x_ref, y_ref, ym_ref, x_w, y_w, ym_w = ode_reference(y, ym, ctl, pred, H, Lq, dl, cfg, sel=sel, rows0=rows0, n_rows=n_rows)
    want = torch.full((n_rows, dl), NAN)
    want[x_w] = x_ref[x_w].float()
    assert x_w.any() and not x_w.all()
    assert torch.equal(bits(X.t.cpu()), bits(want)), 'staged rows bit-equal, sentinels everywhere else'
    assert X.intact() and torch.equal(bits(Y.t.cpu()), bits(y)) and torch.equal(bits(Ym.t.cpu()), bits(ym))

    call('tfx_ode_update', Y.t.data_ptr(), Ym.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, d_pred.data_ptr(), H, Lq, dl, cfg, ptr(d_sel), ptr(d_rows0))
    fb = torch.zeros(B, Lc, dl, dtype=F64)                   # |u| + |cfg| (|f| + |u|) per element (H == 1: |f|)
    for i in range(B):
        rs = [rows0[h * B + i] if rows0 is not None else (h * B + i) * Lq for h in range(H)]
        if min(rs) < 0:
            continue
        f = pred[rs[0]:rs[0] + Lc].double().abs()
        if H == 2:
            u = pred[rs[1]:rs[1] + Lc].double().abs()
            f = u + abs(cfg) * (f + u)
        fb[i] = f
    bound = torch.zeros(B, Lc, dmax, dtype=F64)
    bound[:, :, :dl] = 4 * 2. ** -24 * (y[:, :, :dl].double().abs() + ctl[1].double().abs()[:, None, None] * fb)
    assert y_w.any() and ym_w.any()
    worst = 0.
    for name, G, before, ref, w in (('y', Y, y, y_ref, y_w), ('ym', Ym, ym, ym_ref, ym_w)):
        got = G.t.cpu()
        assert G.intact()
        assert torch.equal(bits(got)[~w], bits(before)[~w]), f'{name}: an element outside the written set changed'
        err = (got.double() - ref)[w].abs()
        if w.any():
            worst = max(worst, float((err / bound[w]).max()))
            assert bool((err <= bound[w]).all()), (name, float(err.max()))
    print(f'ode_update dl {dl} H {H} compact {compact} sel {use_sel}: worst error / bound {worst:.3f}')


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
def test_ode_kernels_staggered_whole_solve_against_odeint(H, compact):
    """the staggered solve of the CPU test through the kernels (the field evaluated with torch on the device between stage and update) against fp64
    odeint of every sample on its own.  Bound 2e-5 (max|y| + max|c|): 14 updates of at most 8 fp32 roundings each, amplified by at most e^0.9."""
    B, Lc, Lq, dmax, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['Lq'], ODE_SHAPE['dmax'], 5
    ts, evals = ode_evals(SOLVE_S)
    y0, c, cu = (t.float() for t in solve_fields(B, Lc, dl))   # the solve starts from fp32 numbers on both sides
    Y, Ym, X = Guarded((B, Lc, dmax), torch.float32, NAN), Guarded((B, Lc, dmax), torch.float32, NAN), Guarded((H * B * Lq, dl), torch.float32, NAN)
    Y.t[:, :, :dl] = dev(y0)
    d_c, d_cu = dev(c), dev(cu)
    for step in range(solve_steps(evals)):
        sched = solve_schedule(step, evals)
        d_ctl = dev(torch.tensor([[s[0] for s in sched], [s[1] for s in sched]], dtype=torch.float32))
        rows0 = solve_rows0(B, H, Lc, sched, seed=step)[0] if compact else None
        d_rows0 = None if rows0 is None else dev(torch.tensor(rows0, dtype=torch.int32))
        X.t.fill_(NAN)
        call('tfx_ode_stage', Y.t.data_ptr(), Ym.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
        pred = solve_pred(X.t, sched, d_c, d_cu, H, Lq, rows0).contiguous()
        call('tfx_ode_update', Y.t.data_ptr(), Ym.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, pred.data_ptr(), H, Lq, dl, CFG_SCALE, None, ptr(d_rows0))
    got = Y.t.cpu()
    assert Y.intact() and Ym.intact() and X.intact()
    assert bool(torch.isnan(got[:, :, dl:]).all()) and bool(torch.isnan(Ym.t.cpu()[:, :, dl:]).all()), 'columns >= dl stay untouched'
    want = torch.stack([odeint(solve_field(c[i].double(), cu[i].double(), H), y0[i].double(), ts, method='midpoint')[-1] for i in range(B)])
    err = float((got[:, :, :dl].double() - want).abs().max())
    scale = max(float(y0.abs().max()), float(want.abs().max())) + max(float(c.abs().max()), float(cu.abs().max()))
    print(f'staggered solve H {H} compact {compact}: max |y - odeint| {err:.3e}, bound {2e-5 * scale:.3e}')
    assert err <= 2e-5 * scale


# ---------------------------------------------------------------------------------------------- (c) tfx_mse_fwd_bwd modes, tfx_output_to_flow
MSE_RUNS = ['plain', 'plain_acc', 'clean', 'recon0', 'recon1', 'recon0_clean_acc']


@pytest.mark.parametrize('mode', MSE_RUNS)
@pytest.mark.parametrize('R,dl,ldp,ldd', MSE_SHAPES)
def test_mse_modes(R, dl, ldp, ldd, mode):
    """loss sum and d pred of every mode against fp64 autograd of the loss as the reference states it.  acc[0] starts non-zero and must grow by the fp64
    sum to 1e-5 relative (non-negative terms, rounding chains of ~120 steps of 2^-24); d pred elementwise within 2^-8 |ref| + 2^-22 (|g| + |old|) (one
    bf16 rounding is 2^-9; the rest covers an fp32 bit that flips it)."""
    pred, flow, noise, times, row_inst, w = mse_inputs(R, dl, seed=1)
    t_row = times[row_inst.long()]
    clean, accumulate = 'clean' in mode, mode.endswith('_acc')
    rmode = 0 if 'recon0' in mode else 1 if 'recon1' in mode else None
    gs = 0.37
    pp = torch.full((R, ldp), NAN); pp[:, :dl] = pred          # the pad columns of pred are never read
    d_pred, d_flow, d_inst, d_time, d_w = dev(pp), dev(flow), dev(row_inst), dev(times), dev(w)
    dp, acc = Guarded((R, ldd), BF, NAN), Guarded((4,), torch.float32, NAN)
    acc.t[0] = 0.5
    kw = dict(R=R, dl=dl, pred=d_pred, ld_pred=ldp, flow=d_flow, grad_scale=gs, dpred=dp.t, ld_d=ldd, acc=acc.t)
    if clean:
        kw.update(row_inst=d_inst, inst_time=d_time, clean_eps=CLEAN_EPS)
    if rmode is not None:
        kw.update(recon_w=d_w, recon_inst=d_inst, recon_time=d_time, recon_mode=rmode)
    old = None
    if mode == 'plain_acc':                                  # a second target on the same prediction, on top of the plain call's result
        capi.call('tfx_mse_fwd_bwd', capi.make_args('tfx_mse_args', **kw), sp().value)
        flow = torch.randn(R, dl, generator=torch.Generator().manual_seed(9))
        d_flow2 = dev(flow)
        kw.update(flow=d_flow2, accumulate=1)
    elif accumulate:                                         # the product's third target: onto whatever the buffer holds, pad columns included
        dp.t.copy_(dev(torch.randn(R, ldd, generator=torch.Generator().manual_seed(9)).to(BF)))
        kw.update(accumulate=1)
    if accumulate:
        old = dp.t.cpu().clone()
    acc0 = float(acc.t[0].double())
    capi.call('tfx_mse_fwd_bwd', capi.make_args('tfx_mse_args', **kw), sp().value)
    got, acc1 = dp.t.cpu(), acc.t.cpu()
    assert dp.intact() and acc.intact() and torch.equal(bits(acc1[1:]), bits(torch.full((3,), NAN))), 'guard bands / acc[1:]'
    rkw = dict(clean_eps=CLEAN_EPS if clean else None, recon_w=w if rmode is not None else None, recon_mode=rmode or 0)
    loss, g = mse_reference(pred, flow, noise, t_row, gs, **rkw)
    grown = float(acc1[0].double()) - acc0
    print(f'mse {mode} R {R} dl {dl}: loss {float(loss):.6e}, acc grew by {grown:.6e} (rel {abs(grown - float(loss)) / float(loss):.2e})')
    assert abs(grown - float(loss)) <= 1e-5 * float(loss)
    oldv = old[:, :dl].double() if accumulate else torch.zeros_like(g)
    ref = g + oldv
    bound = 2. ** -8 * ref.abs() + 2. ** -22 * (g.abs() + oldv.abs())
    err = (got[:, :dl].double() - ref).abs()
    assert bool(torch.isfinite(got[:, :dl].float()).all())
    print(f'mse {mode} R {R} dl {dl}: worst d pred error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}')
    assert bool((err <= bound).all()), float((err - bound).max())
    if rmode is not None and not accumulate:
        assert bool((w == 0).any()) and bool((got[w == 0] == 0).all()), 'rows of weight zero'
    if accumulate:
        assert torch.equal(bits(got[:, dl:]), bits(old[:, dl:])), 'accumulate: pad columns unchanged'
    else:
        assert bool((got[:, dl:] == 0).all()), 'pad columns zeroed'


@pytest.mark.parametrize('with_eps', [False, True])
@pytest.mark.parametrize('dl', [5, 48])
def test_output_to_flow(dl, with_eps):
    R = 37
    pred, x, eps, times, row_inst, _ = mse_inputs(R, dl, seed=2)
    P = Guarded((R, dl), torch.float32, NAN)
    P.t.copy_(dev(pred))
    d_x, d_eps, d_inst, d_time = dev(x), dev(eps) if with_eps else None, dev(row_inst), dev(times)
    call('tfx_output_to_flow', P.t.data_ptr(), d_x.data_ptr(), ptr(d_eps), d_inst.data_ptr(), d_time.data_ptr(), R, dl, CLEAN_EPS)
    t = times[row_inst.long()].double()[:, None]
    assert bool((t == 0).any()) and bool((t == 1).any()) and bool(((1 - t) < CLEAN_EPS).any())
    noised = x.double() * t + eps.double() * (1 - t) if with_eps else x.double()
    den = (1 - t).clamp(min=CLEAN_EPS)
    ref = (pred.double() - noised) / den
    bound = 4 * 2. ** -24 * (pred.double().abs() + x.double().abs() + (eps.double().abs() if with_eps else 0.)) / den
    err = (P.t.cpu().double() - ref).abs()
    print(f'output_to_flow dl {dl} eps {with_eps}: worst error / bound {float((err / bound).max()):.3f}')
    assert P.intact() and bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------- (d) tfx_ce_fwd_bwd edges
def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-20))


@pytest.mark.parametrize('variant', ['plain', 'x30', 'ignored'])
@pytest.mark.parametrize('T,V,ld,ld_d', CE_SHAPES)
def test_ce_edges(T, V, ld, ld_d, variant):
    """the register fast path at its edge (ld = 512) and just past it (ld = 516), more tokens than one trip of the grid (4100 > 1024 blocks x 4 waves),
    a single row; labels 0 and V - 1, ignored rows, a row of equal logits, logits x 30, every label ignored.  Tolerances of tests/test_kernels_gpu.py."""
    g = torch.Generator().manual_seed(0)
    logits = torch.full((T, ld), NAN); logits[:, :V] = torch.randn(T, V, generator=g) * 2 * (30. if variant == 'x30' else 1.)
    labels = torch.randint(0, V, (T,), generator=g, dtype=torch.int32)
    labels[0] = V - 1
    if T > 2:
        labels[3::5] = -1
        labels[1] = 0; logits[2, :V] = 1.25                   # a row of equal logits
    if variant == 'ignored':
        labels[:] = -1
    scale = 1.0 / 1234
    dlog, acc = Guarded((T, ld_d), BF, NAN), Guarded((4,), torch.float32, NAN)
    acc.t[0] = 0.5; acc.t[1] = 2.
    acc_before = acc.t.cpu().clone()
    d_logits, d_labels = dev(logits), dev(labels)
    a = capi.make_args('tfx_ce_args', T=T, V=V, logits=d_logits, ld=ld, labels=d_labels, grad_scale=scale, dlogits=dlog.t, ld_d=ld_d, acc=acc.t)
    capi.call('tfx_ce_fwd_bwd', a, sp().value)
    got, acc1 = dlog.t.cpu(), acc.t.cpu()
    assert dlog.intact() and acc.intact() and torch.equal(bits(acc1[2:]), bits(acc_before[2:]))
    assert bool((got[:, V:] == 0).all()), 'pad columns zeroed'
    if variant == 'ignored':
        assert torch.equal(bits(acc1), bits(acc_before)), 'acc untouched'
        assert bool((got == 0).all())
        return
    lr = logits[:, :V].double().requires_grad_(True)
    ce = F.cross_entropy(lr, labels.long(), ignore_index=-1, reduction='sum')
    (ce * scale).backward()
    grown = float(acc1[0].double()) - 0.5
    print(f'ce {variant} ({T}, {V}, {ld}, {ld_d}): loss {float(ce):.6e} got {grown:.6e}')
    assert abs(grown - float(ce)) < 1e-3 * float(ce)
    assert float(acc1[1]) == 2. + int((labels >= 0).sum())
    assert bool(torch.isfinite(got.float()).all())
    e = relerr(got[:, :V], lr.grad)
    print(f'ce {variant} dlogits rel err {e:.3e}')
    assert e <= 6e-3
    assert bool((got[labels < 0] == 0).all())


# ---------------------------------------------------------------------------------------------- (e) small kernels
@pytest.mark.parametrize('n', [1, 7, 8, 9, 2048, 2053, 6145])
def test_add_bf16_and_scale_bf16_copy(n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g).to(BF), torch.randn(n, generator=g).to(BF)
    want = (a.float() + b.float()).to(BF)
    d_b = dev(b)
    for alias in (False, True):                              # the engine adds in place: out == a
        A, O = Guarded((n,), BF, NAN), Guarded((n,), BF, NAN)
        A.t.copy_(dev(a))
        out = A if alias else O
        call('tfx_add_bf16', A.t.data_ptr(), d_b.data_ptr(), out.t.data_ptr(), n)
        assert torch.equal(bits(out.t.cpu()), bits(want)) and A.intact() and O.intact(), (n, alias)
        if not alias:
            assert torch.equal(bits(A.t.cpu()), bits(a))
    for sc in (-1.0, 0.37):
        O = Guarded((n,), BF, NAN)
        d_a = dev(a)
        call('tfx_scale_bf16_copy', d_a.data_ptr(), O.t.data_ptr(), n, sc)
        want = (a.float() * torch.tensor(sc, dtype=torch.float32)).to(BF)
        assert torch.equal(bits(O.t.cpu()), bits(want)) and O.intact(), (n, sc)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027])
def test_f32_to_bf16_rounds_to_nearest_even(n):
    inf = float('inf')
    special = torch.tensor([1. + 2. ** -8, 1. + 3 * 2. ** -8, -(1. + 2. ** -8), inf, -inf, 3.4e38, -3.4e38, 3.3895e38, 1. + 2. ** -8 + 2. ** -20, 0., -0.])
    src = torch.randn(n, generator=torch.Generator().manual_seed(n))
    k = min(n, special.numel())
    src[:k] = special[:k]
    if n >= 2 * special.numel():
        src[-special.numel():] = special.flip(0)             # the specials again in the scalar tail and the last vectors
    O = Guarded((n,), BF, NAN)
    d_src = dev(src)
    call('tfx_f32_to_bf16', d_src.data_ptr(), O.t.data_ptr(), n)
    want = src.to(BF)
    assert float(want[0]) == 1. and (n < 4 or float(want[3]) == inf) and (n < 1027 or (float(want[5]) == inf and float(want[1]) == 1. + 2. ** -6))
    assert torch.equal(bits(O.t.cpu()), bits(want)) and O.intact()


def test_cast_block_bf16_inside_larger_matrices():
    """a 5 x 24 block at (row 8, column 16) of a 40-wide fp32 matrix into rows 8 .. 12, columns 8 .. 31 of a 32-wide bf16 matrix"""
    g = torch.Generator().manual_seed(0)
    src = torch.randn(16, 40, generator=g)
    D = Guarded((16, 32), BF, NAN)
    d_src = dev(src)
    s_ptr, d_ptr = d_src.data_ptr() + (8 * 40 + 16) * 4, D.t.data_ptr() + (8 * 32 + 8) * 2
    assert s_ptr % 16 == 0 and d_ptr % 16 == 0
    call('tfx_cast_block_bf16', s_ptr, 40, d_ptr, 32, 5, 24)
    want = torch.full((16, 32), NAN, dtype=BF)
    want[8:13, 8:32] = src[8:13, 16:40].to(BF)
    assert torch.equal(bits(D.t.cpu()), bits(want)) and D.intact()


def test_onehot_bf16():
    T, ld = 37, 72
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 70, (T,), generator=g, dtype=torch.int32)
    ids[0], ids[1], ids[2], ids[3] = -1, 0, 69, -1
    tok_inst = torch.where(torch.arange(T) % 3 == 2, torch.arange(T) % 4, torch.full((T,), -1)).to(torch.int32)
    tok_inst[:3] = -1; tok_inst[3] = 1
    O = Guarded((T, ld), BF, NAN)
    d_ids, d_inst = dev(ids), dev(tok_inst)
    call('tfx_onehot_bf16', d_ids.data_ptr(), d_inst.data_ptr(), O.t.data_ptr(), T, ld)
    want = torch.zeros(T, ld)
    for t in range(T):
        if tok_inst[t] < 0:
            want[t, max(int(ids[t]), 0)] = 1.
    assert bool((tok_inst >= 0).any()) and want[0, 0] == 1 and want[2, 69] == 1 and want[3].sum() == 0
    assert torch.equal(bits(O.t.cpu()), bits(want.to(BF))) and O.intact()


def test_gather_f32():
    n, m = 300, 50
    g = torch.Generator().manual_seed(0)
    src = torch.randn(m, generator=g)
    mp = torch.randint(0, m, (n,), generator=g, dtype=torch.int32)
    mp[::7] = -1; mp[1] = 0; mp[2] = m - 1
    O = Guarded((n,), torch.float32, NAN)
    d_src, d_mp = dev(src), dev(mp)
    call('tfx_gather_f32', d_src.data_ptr(), d_mp.data_ptr(), O.t.data_ptr(), n)
    want = torch.where(mp >= 0, src[mp.clamp(min=0).long()], torch.zeros(n))
    assert torch.equal(bits(O.t.cpu()), bits(want)) and O.intact()


@pytest.mark.parametrize('C', [1, 64, 65, 200])
@pytest.mark.parametrize('R', [1, 3, 257, 1000])
def test_colsum_f32(R, C):
    ld = C + 3
    g = torch.Generator().manual_seed(R * 1000 + C)
    src = torch.full((R, ld), NAN); src[:, :C] = torch.randn(R, C, generator=g)
    out0 = torch.randn(C, generator=g)
    O = Guarded((C,), torch.float32, NAN)
    O.t.copy_(dev(out0))
    d_src = dev(src)
    call('tfx_colsum_f32', d_src.data_ptr(), ld, R, C, O.t.data_ptr())
    x = src[:, :C].double()
    err = (O.t.cpu().double() - (out0.double() + x.sum(0))).abs()
    bound = 1e-5 * (x.abs().sum(0) + out0.double().abs())
    assert O.intact() and bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize('n', [1, 255, 257, 5000])
def test_silu_bwd(n):
    g = torch.Generator().manual_seed(n)
    pre = torch.linspace(-20, 20, n) if n > 1 else torch.zeros(1)
    pre[n // 2] = 0.
    pre = pre[torch.randperm(n, generator=g)].to(BF)
    dy = torch.randn(n, generator=g).to(BF)
    assert bool((pre == 0).any()) and (n == 1 or (float(pre.min()) == -20. and float(pre.max()) == 20.))
    O = Guarded((n,), BF, NAN)
    d_dy, d_pre = dev(dy), dev(pre)
    call('tfx_silu_bwd', d_dy.data_ptr(), d_pre.data_ptr(), O.t.data_ptr(), n)
    x, s = pre.double(), pre.double().sigmoid()
    ref = dy.double() * s * (1 + x * (1 - s))
    got = O.t.cpu()
    assert O.intact() and bool(torch.isfinite(got.float()).all())
    assert relerr(got, ref) <= 1e-2


def test_empty_calls_return_zero_before_launching():
    """B == 0 / n == 0 on the entries whose wrappers answer 0 before any launch"""
    L = capi.lib()
    f, h, i = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV, dtype=BF), torch.zeros(64, device=DEV, dtype=torch.int32)
    F_, H_, I_ = f.data_ptr(), h.data_ptr(), i.data_ptr()
    assert L.tfx_sample_tokens(F_, 8, 0, 8, 1., 0.1, F_, None, I_, sp()) == 0
    assert L.tfx_sample_tokens_range(F_, 8, 0, 8, 4, 1., 0.1, F_, None, I_, sp()) == 0
    assert L.tfx_ode_stage(F_, F_, F_, 0, 2, 4, F_, 1, 2, 4, None, sp()) == 0
    assert L.tfx_ode_update(F_, F_, F_, 0, 2, 4, F_, 1, 2, 4, 1., None, None, sp()) == 0
    assert L.tfx_scale_bf16_copy(H_, H_, 0, 1., sp()) == 0
    assert L.tfx_cast_block_bf16(F_, 8, H_, 8, 0, 8, sp()) == 0
    assert L.tfx_output_to_flow(F_, F_, None, I_, F_, 0, 4, 0.05, sp()) == 0
    assert L.tfx_onehot_bf16(I_, I_, H_, 0, 8, sp()) == 0
    assert L.tfx_gather_f32(F_, I_, F_, 0, sp()) == 0
    assert L.tfx_f32_to_bf16(F_, H_, 0, sp()) == 0
    assert L.tfx_silu_bwd(H_, H_, H_, 0, sp()) == 0
    assert L.tfx_add_bf16(H_, H_, H_, 0, sp()) == 0
    assert L.tfx_colsum_f32(F_, 8, 0, 8, F_, sp()) == 0
    a = capi.make_args('tfx_mse_args', R=0, dl=4, pred=f, ld_pred=4, flow=f, grad_scale=1., dpred=h, ld_d=8, acc=f)
    assert L.tfx_mse_fwd_bwd(ctypes.byref(a), sp()) == 0
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((h == 0).all()) and bool((i == 0).all())
