"""Adams-Bashforth multistep solvers on the device: tfx_ode_ab_update / tfx_ode_ab_axpy through the C ABI against the fp64 restatement of
tests/_ode_ab_cases.py (pinned on the CPU by tests/test_ode_multistep_cpu.py), a whole staggered solve per method against `ab_solve`, and the
sampling paths of a model built with each method - to the bit against the start-up rule on short grids, against each other on a longer one.

Buffers sit between guard bands of NaN sentinels compared bit for bit afterwards; every k slot, history slot and column a call must not read holds a
NaN, so a stray read shows up in the result.  Helpers and models are those of tests/test_ode_solvers_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ode_ab_cases as AB  # noqa: E402
import _ode_rk_cases as RK  # noqa: E402
import test_ode_solvers_gpu as T  # noqa: E402
from _decode_loss_cases import CFG_SCALE, F64, ODE_SHAPE, SOLVE_OFFSETS, SOLVE_S, solve_field, solve_fields, solve_pred, solve_rows0  # noqa: E402

DEV, NAN = T.DEV, T.NAN
Guarded, bits, call, dev, ptr, same_bits = T.Guarded, T.bits, T.call, T.dev, T.ptr, T.same_bits
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))

# ---------------------------------------------------------------------------------------------- 1. one call of stage + update
DTS = [0.25, -0.5, 0.75, 0.125, 1.5]                         # per-sample step sizes: every sample has its own weights
# what each of the 5 samples does in a call.  ('stage', rule, slot): stage 0 of a start-up step, stores g in `slot` (mode 1);  ('last', rule): the last stage
# of a start-up step, no history field (mode 2);  ('ab', P, n, store): the multistep step n of order P, g to slot n mod 3 if `store`;  ('mode', m): mode 0 / 3.
# The guidance-less / compacted / sel variants of the test take samples 3 and 4 out of the update, so 0 .. 2 carry what every variant must check.
ROLES = [
    [('stage', 'rk4', 2), ('ab', 2, 4, True), ('ab', 4, 3, True), ('mode', 3), ('last', 'heun3')],      # ab4 at n = 3: g_3 replaces g_0, which the call reads
    [('ab', 3, 2, True), ('last', 'rk4'), ('ab', 4, 7, False), ('mode', 0), ('stage', 'heun2', 0)],
    [('ab', 4, 5, True), ('stage', 'heun3', 1), ('ab', 2, 1, False), ('ab', 3, 6, True), ('ab', 2, 3, True)],
]


def element_case(roles, H, compact, use_sel, dl, seed):
    B, Lc, Lq, dmax = (ODE_SHAPE[k] for k in ('B', 'Lc', 'Lq', 'dmax'))
    g = torch.Generator().manual_seed(23 + seed)
    y, k, hist = torch.randn(B, Lc, dmax, generator=g), torch.randn(3, B, Lc, dmax, generator=g), torch.randn(3, B, Lc, dmax, generator=g)
    ctl = torch.zeros(16, B)
    ctl[9] = -1.
    alias = 0
    for i, role in enumerate(roles):
        if role[0] == 'mode':
            ctl[0, i] = role[1]
        elif role[0] in ('stage', 'last'):
            _, c, A, b = RK.TABLEAUS[role[1]]
            q = 0 if role[0] == 'stage' else len(c) - 1
            ctl[0, i], ctl[1, i] = (1 if role[0] == 'stage' else 2), q
            for j, a in enumerate(A[q]):
                ctl[2 + j, i] = f32(DTS[i] * float(a))
            for j, bj in enumerate(b):
                ctl[5 + j, i] = f32(DTS[i] * float(bj))
            if role[0] == 'stage':
                ctl[9, i] = role[2]
        else:
            _, P, n, store = role
            beta = AB.MULTISTEP[f'ab{P}'][2]
            ctl[0, i], ctl[1, i], ctl[5, i] = 2, 0, f32(DTS[i] * float(beta[0]))
            for s, j in enumerate(range(P - 1, 0, -1)):
                ctl[10 + s, i], ctl[13 + s, i] = (n - j) % 3, f32(DTS[i] * float(beta[j]))
            if store:
                ctl[9, i] = n % 3
                alias += int(any(int(ctl[10 + s, i]) == n % 3 and float(ctl[13 + s, i]) != 0. for s in range(3)))
    y[:, :, dl:] = NAN; k[:, :, :, dl:] = NAN; hist[:, :, :, dl:] = NAN        # columns the calls must neither read nor write
    for i in range(B):                                       # what the update may not read is a NaN: k slots >= q or of a zero weight, history slots not named with a weight
        q = int(ctl[1, i])
        k[q:, i] = NAN
        for j in range(q):
            if float(ctl[5 + j, i]) == 0.:
                k[j, i] = NAN
        read = {int(ctl[10 + s, i]) for s in range(3) if float(ctl[13 + s, i]) != 0.} if int(ctl[0, i]) == 2 else set()
        for s in range(3):
            if s not in read:
                hist[s, i] = NAN
    if compact:                                              # blocks in shuffled order; sample 3 without its conditional half, sample 4 without its last half
        neg = {(0, 3), (H - 1, 4)}
        live = [(h, i) for h in range(H) for i in range(B) if (h, i) not in neg]
        order = torch.randperm(len(live), generator=torch.Generator().manual_seed(5)).tolist()
        rows0 = [-1] * (H * B)
        for slot, kk in enumerate(order):
            h, i = live[kk]
            rows0[h * B + i] = slot * Lc
        n_rows = len(live) * Lc
    else:
        rows0, n_rows = None, H * B * Lq
    sel = [1., 1., 1., 1., 0.] if use_sel else None
    pred = torch.randn(n_rows, dl, generator=g)
    return dict(B=B, Lc=Lc, Lq=Lq, dmax=dmax, y=y, k=k, hist=hist, ctl=ctl, rows0=rows0, n_rows=n_rows, sel=sel, pred=pred, alias=alias)


@pytest.mark.parametrize('use_sel', [False, True])
@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
def test_ab_update_element_by_element(H, compact, use_sel):
    """per-sample mixed modes in one call: start-up stages that store history, start-up last stages, multistep steps of each order (one whose store slot
    is a slot it reads), modes 0 and 3; y, k, hist and `pred` are random, so a wrong coefficient or slot is an O(1) error.  Bound per element:
    (terms + 4) 2^-24 sum|terms|, 0 (bit-equal) for a stored derivative without guidance."""
    cfg, worst, n_alias, n_hist, n_exact = 2.5, 0., 0, 0, 0
    for dl in (12, 5):
        for v, roles in enumerate(ROLES):
            C = element_case(roles, H, compact, use_sel, dl, v)
            B, Lc, Lq, dmax = C['B'], C['Lc'], C['Lq'], C['dmax']
            assert B * Lc * dmax > 256, 'more than one block'
            Y, K, HS, X = Guarded((B, Lc, dmax), C['y']), Guarded((3, B, Lc, dmax), C['k']), Guarded((3, B, Lc, dmax), C['hist']), Guarded((C['n_rows'], dl))
            d_ctl, d_pred = dev(C['ctl']), dev(C['pred'])
            d_rows0 = dev(None if C['rows0'] is None else torch.tensor(C['rows0'], dtype=torch.int32))
            d_sel = dev(None if C['sel'] is None else torch.tensor(C['sel']))
            R = AB.ab_reference(C['y'], C['k'], C['hist'], C['ctl'], C['pred'], H, Lq, dl, cfg, sel=C['sel'], rows0=C['rows0'], n_rows=C['n_rows'])
            # the staging side is tfx_ode_rk_stage on rows 0..4 of the same block: a multistep evaluation (mode 2, stage 0) stages y itself
            call('tfx_ode_rk_stage', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
            x, x_w = X.t.cpu(), R['x_w']
            for i, role in enumerate(roles):
                if role[0] == 'ab':
                    for h in range(H):
                        r0 = C['rows0'][h * B + i] if compact else (h * B + i) * Lq
                        if r0 >= 0:
                            assert same_bits(x[r0:r0 + Lc], C['y'][i, :, :dl]), 'the input of a multistep evaluation is y to the bit'
                            n_exact += 1
            assert bool(torch.isnan(x[~x_w]).all()) and X.intact() and same_bits(Y.t, C['y']) and same_bits(K.t, C['k'])

            call('tfx_ode_ab_update', Y.t.data_ptr(), K.t.data_ptr(), HS.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, d_pred.data_ptr(), H, Lq, dl, cfg,
                 ptr(d_sel), ptr(d_rows0))
            assert R['y_w'].any() and R['h_w'].any()
            n_alias += C['alias']; n_hist += int(R['h_w'].sum())
            for name, G, before, ref, w, bound in (('y', Y, C['y'], R['y'], R['y_w'], R['y_bound']), ('k', K, C['k'], R['k'], R['k_w'], R['k_bound']),
                                                   ('hist', HS, C['hist'], R['h'], R['h_w'], R['h_bound'])):
                got = G.t.cpu()
                assert G.intact()
                assert torch.equal(bits(got)[~w], bits(before)[~w]), f'{name}: an element outside the written set changed'
                if w.any():
                    assert not bool(torch.isnan(got[w]).any()), f'{name}: a sentinel was read'
                    err = (got.double() - ref)[w].abs()
                    assert bool((err <= bound[w]).all()), (v, name, float(err.max()))
                    worst = max(worst, float((err / bound[w].clamp(min=1e-300)).max()))
                    if name != 'y' and H == 1:
                        assert same_bits(got[w], ref.float()[w]), 'without guidance the stored derivative is the prediction itself'
            ks, hs = K.t.cpu(), HS.t.cpu()
            for i, role in enumerate(roles):                 # a start-up stage 0: the ring gets the bits k_0 gets
                if role[0] == 'stage' and bool(R['k_w'][0, i].any()):
                    assert same_bits(ks[0, i, :, :dl], hs[role[2], i, :, :dl])
    assert n_alias > 0 and n_hist > 0 and n_exact > 0, 'a store slot that is also read, stored history and staged multistep inputs all occur'
    print(f'ab update H {H} compact {compact} sel {use_sel}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------- 2. no history fields: tfx_ode_rk_update's bits
@pytest.mark.parametrize('use_sel', [False, True])
@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
def test_ab_update_without_history_fields_is_rk_update_to_the_bit(H, compact, use_sel):
    for method in ('heun3', 'rk4'):
        for q in range(RK.stages(method)):
            C = T.element_case(method, q, H, compact, use_sel, 5)
            B, Lc, Lq, dmax = C['B'], C['Lc'], C['Lq'], C['dmax']
            ctl16 = torch.zeros(16, B)
            ctl16[:9] = C['ctl']; ctl16[9] = -1.; ctl16[10:13] = 1.        # slots named, weights zero: never read
            d_pred = dev(C['pred'])
            d_rows0 = dev(None if C['rows0'] is None else torch.tensor(C['rows0'], dtype=torch.int32))
            d_sel = dev(None if C['sel'] is None else torch.tensor(C['sel']))
            Y1, K1 = Guarded((B, Lc, dmax), C['y']), Guarded((3, B, Lc, dmax), C['k_update'])
            Y2, K2, HS = Guarded((B, Lc, dmax), C['y']), Guarded((3, B, Lc, dmax), C['k_update']), Guarded((3, B, Lc, dmax))
            call('tfx_ode_rk_update', Y1.t.data_ptr(), K1.t.data_ptr(), dev(C['ctl']).data_ptr(), B, Lc, dmax, d_pred.data_ptr(), H, Lq, 5, 2.5, ptr(d_sel), ptr(d_rows0))
            call('tfx_ode_ab_update', Y2.t.data_ptr(), K2.t.data_ptr(), HS.t.data_ptr(), dev(ctl16).data_ptr(), B, Lc, dmax, d_pred.data_ptr(), H, Lq, 5, 2.5,
                 ptr(d_sel), ptr(d_rows0))
            assert same_bits(Y1.t, Y2.t) and same_bits(K1.t, K2.t), (method, q)
            assert not same_bits(Y1.t, C['y']) or not same_bits(K1.t, C['k_update']), 'the call did something'
            assert bool((bits(HS.full) == HS.fill_bits).all()), 'hist is not touched'
            assert Y2.intact() and K2.intact()


# ---------------------------------------------------------------------------------------------- 3. tfx_ode_ab_axpy
@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('method', AB.METHODS)
def test_ab_axpy_against_the_reference_and_the_state_machine(method, guided):
    """the dense form: n = 1 and n = 5 * 7 * 12 + 3; g_out absent, separate, and aliasing the oldest h_j; the slots the method does not use are NULL with
    a zero weight.  Error bound of the state-machine test, and - one prescribed sequence - bit-equal to tfx_ode_ab_update on the same numbers."""
    B, Lc, dmax = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['dmax']
    P, _, beta = AB.MULTISTEP[method]
    cfg, dt, worst = 2.5, 0.3, 0.
    w = [f32(dt * float(beta[j])) for j in range(P - 1, 0, -1)] + [0.] * (4 - P)
    wg = f32(dt * float(beta[0]))
    for n in (1, B * Lc * dmax + 3):
        g = torch.Generator().manual_seed(3 * P + n)
        y, fc, fu = (torch.randn(n, generator=g) for _ in range(3))
        h = torch.randn(3, n, generator=g)
        gref = (fu.double() + cfg * (fc.double() - fu.double())) if guided else fc.double()
        fb = (fu.double().abs() + cfg * (fc.double().abs() + fu.double().abs())) if guided else fc.double().abs()
        acc, mag = y.double(), y.double().abs()
        for j in range(P - 1):
            acc = acc + w[j] * h[j].double(); mag = mag + (w[j] * h[j].double()).abs()
        want = acc + wg * gref
        bound = (P - 1 + 4) * RK.U24 * (mag + abs(wg) * fb)
        d_y, d_fc, d_fu = dev(y), dev(fc), dev(fu if guided else None)
        outs = {}
        for g_out in ('none', 'own', 'alias'):
            HS, GO, OUT = Guarded((3, n), h), Guarded((n,)), Guarded((n,))
            hp = [HS.t[j].data_ptr() if j < P - 1 else None for j in range(3)]
            go = {'none': None, 'own': GO.t.data_ptr(), 'alias': HS.t[0].data_ptr()}[g_out]
            call('tfx_ode_ab_axpy', d_y.data_ptr(), *hp, *w[:3], wg, d_fc.data_ptr(), ptr(d_fu), cfg, go, OUT.t.data_ptr(), n)
            assert HS.intact() and GO.intact() and OUT.intact()
            out, hs = OUT.t.cpu(), HS.t.cpu()
            err = (out.double() - want).abs()
            assert bool((err <= bound).all()), (method, n, g_out, float(err.max()))
            worst = max(worst, float((err / bound).max()))
            stored = {'none': None, 'own': GO.t.cpu(), 'alias': hs[0]}[g_out]
            if stored is not None:
                assert bool(((stored.double() - gref).abs() <= 3 * RK.U24 * fb).all()) and (guided or same_bits(stored, fc))
            assert same_bits(hs[1:], h[1:]) and (g_out == 'alias' or same_bits(hs[0], h[0])), 'the history is read-only but for the slot that receives g'
            assert g_out == 'own' or bool(torch.isnan(GO.t.cpu()).all())
            outs[g_out] = (out, stored)
        assert same_bits(outs['none'][0], outs['own'][0]) and same_bits(outs['none'][0], outs['alias'][0]), 'out does not depend on where g goes'
        assert same_bits(outs['own'][1], outs['alias'][1])
        if n == 1:
            continue
        # ---- the same numbers through the state machine: dense rows, Lq == Lc, every sample a multistep step whose g replaces slot 0
        m, H = B * Lc * dmax, 2 if guided else 1
        pred = torch.cat([fc[:m], fu[:m]]) if guided else fc[:m]
        ctl = torch.zeros(16, B)
        ctl[0], ctl[5], ctl[9] = 2, wg, 0
        for j in range(3):
            ctl[10 + j], ctl[13 + j] = j, w[j]
        hist = h[:, :m].reshape(3, B, Lc, dmax).clone()
        hist[P - 1:] = NAN                                   # slots of a zero weight
        Y, K, HS = Guarded((B, Lc, dmax), y[:m].view(B, Lc, dmax)), Guarded((3, B, Lc, dmax)), Guarded((3, B, Lc, dmax), hist)
        call('tfx_ode_ab_update', Y.t.data_ptr(), K.t.data_ptr(), HS.t.data_ptr(), dev(ctl).data_ptr(), B, Lc, dmax, dev(pred.view(H * B * Lc, dmax)).data_ptr(),
             H, Lc, dmax, cfg, None, None)
        assert Y.intact() and K.intact() and HS.intact() and bool(torch.isnan(K.t).all())
        assert same_bits(Y.t.view(-1), outs['alias'][0][:m]), 'update of the state machine == dense form, to the bit'
        assert same_bits(HS.t[0].reshape(-1), outs['alias'][1][:m]), 'stored derivative: the same bits in both forms'
    print(f'ab axpy {method} guided {guided}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------- 4. staggered whole solve
_CACHE = {}


def _yardsticks(H):
    B, Lc, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5
    if ('yard', H) not in _CACHE:
        y0, c, cu = (t.float() for t in solve_fields(B, Lc, dl))   # the solve starts from fp32 numbers on both sides
        ts = torch.linspace(0, 1, SOLVE_S, dtype=F64)
        want = {m: torch.stack([AB.ab_solve(m, solve_field(c[i].double(), cu[i].double(), H), y0[i].double(), ts) for i in range(B)]) for m in AB.METHODS}
        _CACHE[('yard', H)] = (y0, c, cu, want)
    return _CACHE[('yard', H)]


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', AB.METHODS)
def test_ab_kernels_staggered_whole_solve_against_ab_solve(method, H, compact):
    """SOLVE_S grid points, sample i starting at global step SOLVE_OFFSETS[i] - so start-up stages, multistep steps, idle and finished samples share a
    launch - the toy field evaluated with torch on the device between stage and update, k and hist NaN at the start (a stale slot read would show),
    against fp64 `ab_solve` of every sample on its own within AB.solve_bound (derived in its docstring)."""
    B, Lc, Lq, dmax, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['Lq'], ODE_SHAPE['dmax'], 5
    y0, c, cu, wants = _yardsticks(H)
    want = wants[method]
    ts, evals = AB.ab_evals(method, SOLVE_S)
    assert SOLVE_S == 8 and len(evals) == AB.forwards(method, SOLVE_S)
    Y, K, HS, X = Guarded((B, Lc, dmax)), Guarded((3, B, Lc, dmax)), Guarded((3, B, Lc, dmax)), Guarded((H * B * Lq, dl))
    Y.t[:, :, :dl] = dev(y0)
    d_c, d_cu = dev(c), dev(cu)
    for step in range(max(SOLVE_OFFSETS) + len(evals) + 1):
        sched = AB.ab_schedule(step, evals)
        d_ctl = dev(AB.ab_ctl(sched))
        rows0 = solve_rows0(B, H, Lc, sched, seed=step)[0] if compact else None
        d_rows0 = None if rows0 is None else dev(torch.tensor(rows0, dtype=torch.int32))
        X.t.fill_(NAN)
        call('tfx_ode_rk_stage', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
        pred = solve_pred(X.t, sched, d_c, d_cu, H, Lq, rows0).contiguous()
        call('tfx_ode_ab_update', Y.t.data_ptr(), K.t.data_ptr(), HS.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, pred.data_ptr(), H, Lq, dl, CFG_SCALE, None,
             ptr(d_rows0))
    got = Y.t.cpu()
    assert Y.intact() and K.intact() and HS.intact() and X.intact()
    assert bool(torch.isnan(got[:, :, dl:]).all()) and bool(torch.isnan(K.t.cpu()[:, :, :, dl:]).all()) and bool(torch.isnan(HS.t.cpu()[:, :, :, dl:]).all())
    assert not bool(torch.isnan(HS.t.cpu()[:, :, :, :dl]).any()), 'every slot was filled'
    err = float((got[:, :, :dl].double() - want).abs().max())
    scale = max(float(y0.abs().max()), float(want.abs().max())) + max(float(c.abs().max()), float(cu.abs().max()))
    bound = AB.solve_bound(method, SOLVE_S, scale)
    print(f'staggered {method} solve H {H} compact {compact}: max |y - ab_solve| {err:.3e}, bound {bound:.3e}')
    assert err <= bound


# ---------------------------------------------------------------------------------------------- 5. short grids: the start-up rule to the bit, end to end
def _equal_samples(a, b, what):
    assert len(a) == len(b), what
    for pa, pb in zip(T.plain(a), T.plain(b)):
        assert pa[0] == pb[0] and torch.equal(pa[-1], pb[-1]) and (pa[0] == 'text' or pa[1] == pb[1]), what


@pytest.mark.parametrize('method,S,start', [('ab4', 4, 'rk4'), ('ab3', 3, 'heun3'), ('ab2', 2, 'heun2')])
def test_short_grids_are_the_start_up_rule_to_the_bit(method, S, start, monkeypatch):
    """N = S - 1 = P - 1 steps: the whole solve is start-up steps, so every sampling path of an `ab` model returns the bits of the same weights under
    the start-up rule - tokens and latents"""
    ab, prompts, noise = T.golden_model(method)
    rk, _, _ = T.golden_model(start)
    kw = dict(T.GOLDEN_KW, init_modality_noise=noise, modality_steps=S)
    n_mod = 0
    for schedule in ('phased', 'continuous'):
        monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', schedule)
        got, want = ab.sample_many([prompts[0], prompts[1]], **kw), rk.sample_many([prompts[0], prompts[1]], **kw)
        for a, b in zip(got, want):
            _equal_samples(a, b, f'{method} sample_many {schedule}')
            n_mod += sum(p[0] == 'mod' for p in T.plain(a))
        _equal_samples(ab.sample_one(prompts[0], **kw), rk.sample_one(prompts[0], **kw), f'{method} sample_one {schedule}')
    assert n_mod >= 2, 'decoded modalities were compared'
    fkw = dict(max_length=14, text_temperature=0., init_modality_noise=noise, modality_steps=S, fixed_modality_shape=(4,), force_modality_at_start=0)
    for cfg_scale, cache_kv in ((1., False), (3., True)):
        _equal_samples(ab._sample_one_through_forward(prompts[0].cuda(), cache_kv=cache_kv, cfg_scale=cfg_scale, **fkw),
                       rk._sample_one_through_forward(prompts[0].cuda(), cache_kv=cache_kv, cfg_scale=cfg_scale, **fkw), f'{method} forward() loop')
    gen_noise = torch.randn(2, 4, ab.md.dim_latents[0], generator=torch.Generator().manual_seed(1))
    ab._gen_noise_override = rk._gen_noise_override = gen_noise
    a, b = (m.generate_modality_only(batch_size=2, modality_steps=S) for m in (ab, rk))
    assert a.shape == b.shape and torch.equal(a, b) and not torch.equal(a, gen_noise.to(a.device)), f'{method} generate_modality_only'


# ---------------------------------------------------------------------------------------------- 6. a longer grid
LONG_S = 8


@pytest.mark.parametrize('method', AB.METHODS)
def test_schedules_and_sample_one_agree_on_a_longer_grid(method, monkeypatch):
    """8 grid points: P - 1 start-up steps, then 8 - P multistep steps.  The continuous schedule (tfx_ode_ab_update), the phased one (tfx_ode_ab_axpy) and
    sample_one return the same text and decoded modalities within the reference's own tolerance"""
    m, prompts, noise = T.golden_model(method)
    kw = dict(T.GOLDEN_KW, init_modality_noise=noise, modality_steps=LONG_S)
    ps = [prompts[0], prompts[1]]
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'phased')
    phased = m.sample_many(ps, **kw)
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'continuous')
    cont = m.sample_many(ps, **kw)
    kept = m._decode_keep
    assert kept is not None and method in kept['key'], 'kept decode plans belong to their method'
    mixed = [p for k, p in kept['plans'].items() if k[0] in ('mix', 'mixc')]
    assert mixed and {p.inst_time.numel() for p in mixed} == {AB.forwards(method, LONG_S) + 1}, 'one conditioning time per evaluation, and t = 1'
    assert all(p.ctl.numel() >= 16 * len(ps) for p in mixed), 'room for the 16-row control block'
    one = m.sample_one(prompts[0], **kw)
    n_mod = 0
    for what, xs, ys in (('continuous vs phased', cont, phased), ('sample_one vs sample_many', [one], cont[:1])):
        for x, y in zip(xs, ys):
            px, py = T.plain(x), T.plain(y)
            assert [p[0] for p in px] == [p[0] for p in py], what
            for a, b in zip(px, py):
                if a[0] == 'text':
                    assert a[1].tolist() == b[1].tolist(), what
                else:
                    d_abs = float((a[2] - b[2]).abs().max()); n_mod += 1
                    print(f'{method}: {what}, modality: max |delta| {d_abs:.3e}')
                    assert a[1] == b[1] and d_abs <= T.SAMPLE_EQ_ATOL, what
    assert n_mod >= 3


@pytest.mark.parametrize('method', AB.METHODS)
def test_schedules_agree_with_two_modality_types(method, monkeypatch):
    """the model of test_ode_solvers_gpu.test_schedules_agree_for_every_method - two modality types of 4 and 9 rows, so the ring grows with the state,
    `sel` picks the samples of a type, samples pass through several blocks out of step with each other - at 6 grid points (every method takes multistep
    steps): phased (tfx_ode_ab_axpy), continuous and compacted (tfx_ode_ab_update) decode schedules give identical text and decoded modalities within the
    project's schedule-agreement gate (2e-2 rel-Frobenius, tests/test_sampling_gpu.py)"""
    from transfusion_pytorch_amd import sampling
    sd, prompts, kw = T.schedule_setup()
    m = T.schedule_model(method, sd)
    kw = {**kw, 'modality_steps': 6}
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'phased')
    phased = m.sample_many(prompts, **kw)
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'continuous')
    cont = m.sample_many(prompts, **kw)
    monkeypatch.setattr(sampling, '_COMPACT', True)
    monkeypatch.setattr(sampling, '_COMPACT_STEP', 64)
    comp = m.sample_many(prompts, **kw)
    n_mod = [sum(isinstance(p, tuple) for p in s) for s in phased]
    types = {p[0] for s in phased for p in s if isinstance(p, tuple)}
    print('modalities per sample:', n_mod, 'types:', sorted(types))
    assert max(n_mod) >= 2 and len(set(n_mod)) > 1 and types == {0, 1}, 'the test needs several blocks of both types, out of step with each other'
    T.compare_samples(f'{method}: continuous vs phased', phased, cont, 2e-2)
    T.compare_samples(f'{method}: compacted vs dense mixed steps', cont, comp, 2e-2)


@pytest.mark.parametrize('method', AB.METHODS)
def test_generate_modality_only_runs_the_method(method):
    """against a host loop of the model's own velocity calls combined in fp64 by `ab_solve`: 2e-2 rel-Frobenius (the tableau rules' gate), and exactly
    stages(start) (P - 1) + 8 - P velocity calls: 8 / 11 / 16"""
    sd, _, _ = T.schedule_setup()
    m = T.schedule_model(method, sd)
    noise = torch.randn(2, 3, 3, 16, generator=torch.Generator().manual_seed(1))
    m._gen_noise_override = noise
    calls = []
    inner = m.forward_modality
    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    m.forward_modality = counted
    got = m.generate_modality_only(batch_size=2, modality_type=1, modality_steps=LONG_S)
    assert len(calls) == AB.forwards(method, LONG_S) == {'ab2': 8, 'ab3': 11, 'ab4': 16}[method]
    f = lambda t, y: inner(y.float(), times=torch.as_tensor(float(t), dtype=torch.float32, device=DEV).expand(2), modality_type=1, encode_modality=False,
                           return_loss=False).double()
    with torch.no_grad():
        want = AB.ab_solve(method, f, noise.to(DEV).double(), torch.linspace(0., 1., LONG_S, dtype=F64))
    rel = float((got.double() - want).norm() / want.norm())
    print(f'{method}: generate_modality_only vs ab_solve over the model\'s own velocity calls: rel-Frobenius {rel:.3e}')
    assert got.shape == want.shape and rel <= 2e-2
