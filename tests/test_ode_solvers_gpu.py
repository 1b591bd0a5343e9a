"""Fixed-grid Runge-Kutta solvers on the device: tfx_ode_rk_stage / tfx_ode_rk_update / tfx_ode_rk_axpy through the C ABI against the fp64 restatement of
tests/_ode_rk_cases.py (pinned on the CPU by tests/test_ode_solvers_cpu.py), a whole staggered solve per method against `rk_solve`, and the four
sampling paths of a model built with each method.

Buffers sit between guard bands of NaN sentinels compared bit for bit afterwards (the `Guarded` pattern of tests/test_decode_loss_kernels_gpu.py);
every k slot and column a call must not read holds a NaN, so a stray read shows up in the result."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _ode_rk_cases as RK  # noqa: E402
from _decode_loss_cases import CFG_SCALE, F64, ODE_SHAPE, SOLVE_OFFSETS, SOLVE_S, solve_field, solve_fields, solve_pred, solve_rows0  # noqa: E402
from transfusion_pytorch_amd import capi  # noqa: E402

DEV = 'cuda'
NAN = float('nan')


def sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    capi.check(getattr(capi.lib(), name)(*args, sp()), name)


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """a device fp32 buffer of `shape` between two bands of NaN (one row, at least 64 elements, a multiple of 8: the body stays 16-byte aligned)"""

    def __init__(self, shape, src=None):
        self.n = math.prod(shape)
        self.g = max(64, (shape[-1] + 7) // 8 * 8)
        self.full = torch.full((self.n + 2 * self.g,), NAN, dtype=torch.float32, device=DEV)
        self.t = self.full[self.g:self.g + self.n].view(shape)
        self.fill_bits = bits(self.full[:1]).clone()
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        iv = bits(self.full)
        return bool((iv[:self.g] == self.fill_bits).all()) and bool((iv[self.g + self.n:] == self.fill_bits).all())


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


# ---------------------------------------------------------------------------------------------- 7. one call of stage + update
MODES = [1, 2, 0, 3, 1]
DTS = [0.25, -0.5, 0.75, 0.125, 1.5]                         # per-sample step sizes: every sample has its own weights


def element_case(method, q, H, compact, use_sel, dl):
    """inputs of one stage + update call.  Sample i sits at stage (q + i) % stages of `method` in mode MODES[i] (a mode-1 sample at stage 3 has no k slot:
    it runs as the step's last stage instead), with the tableau's weights at its own step size."""
    B, Lc, Lq, dmax = (ODE_SHAPE[k] for k in ('B', 'Lc', 'Lq', 'dmax'))
    _, c, A, b = RK.TABLEAUS[method]
    g = torch.Generator().manual_seed(11 + q)
    y, k, = torch.randn(B, Lc, dmax, generator=g), torch.randn(3, B, Lc, dmax, generator=g)
    ctl = torch.zeros(9, B)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    for i in range(B):
        qi = (q + i) % len(c)
        ctl[0, i], ctl[1, i] = (2 if (MODES[i] == 1 and qi == 3) else MODES[i]), qi
        for j, a in enumerate(A[qi]):
            ctl[2 + j, i] = f32(DTS[i] * float(a))
        for j, bj in enumerate(b):
            ctl[5 + j, i] = f32(DTS[i] * float(bj))
    y[:, :, dl:] = NAN; k[:, :, :, dl:] = NAN                # columns the calls must neither read nor write
    k_stage, k_update = k.clone(), k.clone()                 # what each call may not read is a NaN: slots >= q, slots of a zero weight
    for i in range(B):
        qi = int(ctl[1, i])
        k_stage[qi:, i] = NAN; k_update[qi:, i] = NAN
        for j in range(qi):
            if float(ctl[2 + j, i]) == 0.:
                k_stage[j, i] = NAN
            if float(ctl[5 + j, i]) == 0.:
                k_update[j, i] = NAN
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
    return dict(B=B, Lc=Lc, Lq=Lq, dmax=dmax, y=y, k_stage=k_stage, k_update=k_update, ctl=ctl, rows0=rows0, n_rows=n_rows, sel=sel, pred=pred)


@pytest.mark.parametrize('use_sel', [False, True])
@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', RK.METHODS)
def test_rk_stage_and_update_element_by_element(method, H, compact, use_sel):
    """every stage index of the method (and, through the per-sample rotation, every other one next to it) in one stage + update call each; `pred`, y
    and k are random, so a wrong coefficient is an O(1) error: this is the test that pins the tableau arithmetic on the device"""
    cfg, worst, n_exact, n_k = 2.5, 0., 0, 0
    for dl in (12, 5):
        for q in range(RK.stages(method)):
            C = element_case(method, q, H, compact, use_sel, dl)
            B, Lc, Lq, dmax = C['B'], C['Lc'], C['Lq'], C['dmax']
            assert B * Lc * dmax > 256, 'more than one block'
            Y, Ks, Ku, X = Guarded((B, Lc, dmax), C['y']), Guarded((3, B, Lc, dmax), C['k_stage']), Guarded((3, B, Lc, dmax), C['k_update']), Guarded((C['n_rows'], dl))
            d_ctl, d_pred = dev(C['ctl']), dev(C['pred'])
            d_rows0 = dev(None if C['rows0'] is None else torch.tensor(C['rows0'], dtype=torch.int32))
            d_sel = dev(None if C['sel'] is None else torch.tensor(C['sel']))
            geo = (B, Lc, dmax)
            call('tfx_ode_rk_stage', Y.t.data_ptr(), Ks.t.data_ptr(), d_ctl.data_ptr(), *geo, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
            # the reference reads each call's own k: NaNs exactly where that call may not look
            Rs = RK.rk_reference(C['y'], C['k_stage'], C['ctl'], C['pred'], H, Lq, dl, cfg, sel=C['sel'], rows0=C['rows0'], n_rows=C['n_rows'])
            Ru = RK.rk_reference(C['y'], C['k_update'], C['ctl'], C['pred'], H, Lq, dl, cfg, sel=C['sel'], rows0=C['rows0'], n_rows=C['n_rows'])
            x, x_w, xb = X.t.cpu(), Rs['x_w'], Rs['x_bound']
            assert x_w.any() and not x_w.all()
            assert bool(torch.isnan(x[~x_w]).all()) and X.intact(), 'rows no block owns keep their sentinels'
            err = (x.double() - Rs['x'])[x_w].abs()
            assert bool((err <= xb[x_w]).all()), (method, q, 'stage', float(err.max()))
            exact = x_w & (xb == 0)
            assert same_bits(x[exact], Rs['x'].float()[exact]), 'no term added: the input is y to the bit'
            n_exact += int(exact.sum())
            assert same_bits(Y.t, C['y']) and same_bits(Ks.t, C['k_stage']) and Y.intact() and Ks.intact(), 'the stage call writes x alone'
            worst = max(worst, float((err / xb[x_w].clamp(min=1e-300)).max()))

            call('tfx_ode_rk_update', Y.t.data_ptr(), Ku.t.data_ptr(), d_ctl.data_ptr(), *geo, d_pred.data_ptr(), H, Lq, dl, cfg, ptr(d_sel), ptr(d_rows0))
            assert Ru['y_w'].any()
            n_k += int(Ru['k_w'].sum())
            for name, G, before, ref, w, bound in (('y', Y, C['y'], Ru['y'], Ru['y_w'], Ru['y_bound']), ('k', Ku, C['k_update'], Ru['k'], Ru['k_w'], Ru['k_bound'])):
                got = G.t.cpu()
                assert G.intact()
                assert torch.equal(bits(got)[~w], bits(before)[~w]), f'{name}: an element outside the written set changed'
                if w.any():
                    err = (got.double() - ref)[w].abs()
                    assert bool((err <= bound[w]).all()), (method, q, name, float(err.max()))
                    worst = max(worst, float((err / bound[w].clamp(min=1e-300)).max()))
                    if name == 'k' and H == 1:
                        assert same_bits(got[w], ref.float()[w]), 'without guidance the stored derivative is the prediction itself'
    assert n_exact > 0 and n_k > 0, 'inputs without a term and stored derivatives both occur'
    print(f'rk stage + update {method} H {H} compact {compact} sel {use_sel}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------- 8. tfx_ode_rk_axpy
@pytest.mark.parametrize('guided', [False, True])
@pytest.mark.parametrize('method', RK.METHODS)
def test_rk_axpy_against_the_reference_and_the_state_machine(method, guided):
    """the dense form, per stage: n = 1 and n = 5 * 7 * 12 + 3, with / without k_out and out; error bounds of the state-machine test, and - the
    arithmetic being prescribed - bit-equal to what tfx_ode_rk_stage / tfx_ode_rk_update make of the same numbers"""
    B, Lc, dmax = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['dmax']
    _, c, A, b = RK.TABLEAUS[method]
    cfg, dt = 2.5, 0.3
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    worst = 0.
    for n in (1, B * Lc * dmax + 3):
        for q in range(len(c)):
            last = q == len(c) - 1
            w = [f32(dt * float(a)) for a in (b[:q + 1] if last else A[q + 1])]
            g = torch.Generator().manual_seed(7 * q + n)
            y, fc, fu = (torch.randn(n, generator=g) for _ in range(3))
            k = torch.randn(3, n, generator=g)
            k[q:] = NAN
            for j in range(q):
                if w[j] == 0.:
                    k[j] = NAN
            fu_ = fu if guided else None
            gref = (fu.double() + cfg * (fc.double() - fu.double())) if guided else fc.double()
            fb = (fu.double().abs() + cfg * (fc.double().abs() + fu.double().abs())) if guided else fc.double().abs()
            acc, mag, terms = y.double(), y.double().abs(), 0
            for j in range(q):
                if w[j] != 0.:
                    acc = acc + w[j] * k[j].double(); mag = mag + (w[j] * k[j].double()).abs(); terms += 1
            want = acc + w[q] * gref
            bound = (terms + 4) * RK.U24 * (mag + abs(w[q]) * fb)
            d_y, d_fc, d_fu, d_k = dev(y), dev(fc), dev(fu_), dev(k)
            outs = {}
            for with_k, with_out in ((True, True), (False, True), (True, False)):
                K, KO, OUT = Guarded((3, n), k), Guarded((n,)), Guarded((n,))
                call('tfx_ode_rk_axpy', d_y.data_ptr(), K.t.data_ptr(), n, q, *(w + [0.] * (4 - len(w))), d_fc.data_ptr(), ptr(d_fu), cfg,
                     KO.t.data_ptr() if with_k else None, OUT.t.data_ptr() if with_out else None, n)
                assert K.intact() and KO.intact() and OUT.intact() and same_bits(K.t, k), 'k is read-only here'
                ko, out = KO.t.cpu(), OUT.t.cpu()
                if with_k:
                    kerr = (ko.double() - gref).abs()
                    assert bool((kerr <= 3 * RK.U24 * fb).all()) and (guided or same_bits(ko, fc))
                else:
                    assert bool(torch.isnan(ko).all())
                if with_out:
                    err = (out.double() - want).abs()
                    assert bool((err <= bound).all()), (method, q, n, float(err.max()))
                    worst = max(worst, float((err / bound).max()))
                else:
                    assert bool(torch.isnan(out).all())
                outs[(with_k, with_out)] = (ko, out)
            assert same_bits(outs[(True, True)][1], outs[(False, True)][1]) and same_bits(outs[(True, True)][0], outs[(True, False)][0])
            if n == 1:
                continue
            # ---- the same numbers through the state machine: dense rows, Lq == Lc, every sample at stage q
            m = B * Lc * dmax
            H = 2 if guided else 1
            pred = torch.cat([fc[:m], fu[:m]]) if guided else fc[:m]
            ctl = torch.zeros(9, B)
            ctl[1] = q
            for j in range(q + 1):
                ctl[5 + j] = w[j]                            # mode 2 at index q: y + sum_{j<q} w_j k_j + w_q g - what the dense call wrote to `out`
            for j in range(q):
                ctl[2 + j] = w[j]                            # and the stage input of the same weights = the dense call with a zero g weight
            for mode in (2, 1) if q < 3 else (2,):
                ctl[0] = mode
                Y, K, X = Guarded((B, Lc, dmax), y[:m].view(B, Lc, dmax)), Guarded((3, B, Lc, dmax), k[:, :m].reshape(3, B, Lc, dmax)), Guarded((H * B * Lc, dmax))
                d_ctl, d_pred = dev(ctl), dev(pred.view(H * B * Lc, dmax))
                call('tfx_ode_rk_stage', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lc, dmax, None)
                call('tfx_ode_rk_update', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, d_pred.data_ptr(), H, Lc, dmax, cfg, None, None)
                assert Y.intact() and K.intact() and X.intact()
                if mode == 2:
                    assert same_bits(Y.t.view(-1), outs[(True, True)][1][:m]), 'update of the state machine == dense form, to the bit'
                    STG = Guarded((n,))
                    call('tfx_ode_rk_axpy', d_y.data_ptr(), d_k.data_ptr(), n, q, *(w[:q] + [0.] * (4 - q)), d_fc.data_ptr(), ptr(d_fu), cfg, None, STG.t.data_ptr(), n)
                    for h in range(H):
                        assert same_bits(X.t.view(H, -1)[h], STG.t[:m]), 'stage input of the state machine == dense form with a zero last weight'
                else:
                    assert same_bits(K.t[q].reshape(-1), outs[(True, True)][0][:m]), 'stored derivative: the same bits in both forms'
    print(f'rk axpy {method} guided {guided}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------- 9. staggered whole solve
def _yardsticks(H):
    B, Lc, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], 5
    key = ('yard', H)
    if key not in _CACHE:
        y0, c, cu = (t.float() for t in solve_fields(B, Lc, dl))   # the solve starts from fp32 numbers on both sides
        ts = torch.linspace(0, 1, SOLVE_S, dtype=F64)
        want = {m: torch.stack([RK.rk_solve(m, solve_field(c[i].double(), cu[i].double(), H), y0[i].double(), ts) for i in range(B)]) for m in RK.METHODS}
        _CACHE[key] = (y0, c, cu, want)
    return _CACHE[key]


_CACHE = {}


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('method', RK.METHODS)
def test_rk_kernels_staggered_whole_solve_against_rk_solve(method, H, compact):
    """SOLVE_S grid points, sample i starting at global step SOLVE_OFFSETS[i], the toy field evaluated with torch on the device between stage and update,
    against fp64 `rk_solve` of every sample on its own.  Bound (RK.solve_bound): stages (S - 1) updates of at most stages + 7 fp32 roundings each,
    amplified by at most e^0.9, times max|y| + max|c|.  The yardsticks of euler, midpoint and heun2 lie more than 10 bounds away from rk4's, so a solve
    that ran another of those tableaus fails here; heun3 and rk4 are only 2 - 4e-4 apart at this step size - telling those two apart rests on
    the element-by-element tests above."""
    B, Lc, Lq, dmax, dl = ODE_SHAPE['B'], ODE_SHAPE['Lc'], ODE_SHAPE['Lq'], ODE_SHAPE['dmax'], 5
    y0, c, cu, wants = _yardsticks(H)
    want = wants[method]
    ts, evals = RK.rk_evals(method, SOLVE_S)
    assert len(evals) == RK.stages(method) * (SOLVE_S - 1)
    Y, K, X = Guarded((B, Lc, dmax)), Guarded((3, B, Lc, dmax)), Guarded((H * B * Lq, dl))
    Y.t[:, :, :dl] = dev(y0)
    d_c, d_cu = dev(c), dev(cu)
    for step in range(max(SOLVE_OFFSETS) + len(evals) + 1):
        sched = RK.rk_schedule(step, evals)
        d_ctl = dev(RK.rk_ctl(sched))
        rows0 = solve_rows0(B, H, Lc, sched, seed=step)[0] if compact else None
        d_rows0 = None if rows0 is None else dev(torch.tensor(rows0, dtype=torch.int32))
        X.t.fill_(NAN)
        call('tfx_ode_rk_stage', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, X.t.data_ptr(), H, Lq, dl, ptr(d_rows0))
        pred = solve_pred(X.t, sched, d_c, d_cu, H, Lq, rows0).contiguous()
        call('tfx_ode_rk_update', Y.t.data_ptr(), K.t.data_ptr(), d_ctl.data_ptr(), B, Lc, dmax, pred.data_ptr(), H, Lq, dl, CFG_SCALE, None, ptr(d_rows0))
    got = Y.t.cpu()
    assert Y.intact() and K.intact() and X.intact()
    assert bool(torch.isnan(got[:, :, dl:]).all()) and bool(torch.isnan(K.t.cpu()[:, :, :, dl:]).all()), 'columns >= dl stay untouched'
    err = float((got[:, :, :dl].double() - want).abs().max())
    scale = max(float(y0.abs().max()), float(want.abs().max())) + max(float(c.abs().max()), float(cu.abs().max()))
    bound = RK.solve_bound(method, SOLVE_S, scale)
    print(f'staggered {method} solve H {H} compact {compact}: max |y - rk_solve| {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    for other in ('euler', 'midpoint', 'heun2'):
        gap = float((wants[other][0] - wants['rk4'][0]).abs().max())
        assert gap > 10 * RK.solve_bound('rk4', SOLVE_S, scale), (other, gap)


# ---------------------------------------------------------------------------------------------- 10. end to end
def schedule_model(method=None, sd=None):
    """the model of test_sampling_gpu.test_schedules_and_null_text_cache_forms_agree; `method` None = the default constructor arguments"""
    from transfusion_pytorch_amd import Transfusion
    kw = {} if method is None else dict(odeint_kwargs=dict(atol=1e-5, rtol=1e-5, method=method))
    m = Transfusion(num_text_tokens=16, dim_latent=(8, 16), modality_default_shape=((4,), (3, 3)), transformer=dict(dim=128, depth=2, dim_head=16, heads=4), **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda().eval()


def schedule_setup():
    if 'sched' not in _CACHE:
        torch.manual_seed(0)
        base = schedule_model()
        with torch.no_grad():
            base.to_text_logits.weight[base.som_ids[0]] *= 3.; base.to_text_logits.weight[base.som_ids[1]] *= 3.
            base.store.mark_dirty()
        sd = {k: v.detach().cpu().clone() for k, v in base.state_dict().items()}
        prompts = [[torch.randint(0, 16, (5,)).cuda()], [torch.randint(0, 16, (2,)).cuda(), (1, torch.randn(3, 3, 16).cuda())], None, [torch.randint(0, 16, (9,)).cuda()]]
        kw = dict(max_length=48, text_temperature=0., init_modality_noise=torch.randn(16, 16).cuda(), modality_steps=3, cfg_scale=3., force_modality_at_start=0)
        _CACHE['sched'] = (sd, prompts, kw)
    return _CACHE['sched']


def compare_samples(what, ref, other, tol):
    worst = 0.
    for a, b in zip(ref, other):
        assert [isinstance(p, tuple) for p in a] == [isinstance(p, tuple) for p in b], what
        for pa, pb in zip(a, b):
            if isinstance(pa, tuple):
                assert pa[0] == pb[0] and pa[1].shape == pb[1].shape
                worst = max(worst, float((pa[1] - pb[1]).norm() / (pa[1].norm() + 1e-20)))
            else:
                assert torch.equal(pa, pb), what
    print(f'decoded modalities, {what}: worst relative distance {worst:.2e}')
    assert worst <= tol, what


@pytest.mark.parametrize('method', RK.NEW_METHODS)
def test_schedules_agree_for_every_method(method, monkeypatch):
    """phased (tfx_ode_rk_axpy), continuous and compacted (tfx_ode_rk_stage / tfx_ode_rk_update) decode schedules of one model, with and without guidance:
    identical text, decoded modalities within the project's schedule-agreement gate (2e-2 rel-Frobenius, tests/test_sampling_gpu.py)"""
    from transfusion_pytorch_amd import sampling
    sd, prompts, kw = schedule_setup()
    m = schedule_model(method, sd)
    nocfg = {**kw, 'cfg_scale': 1.}
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'phased')
    phased, phased_nocfg = m.sample_many(prompts, **kw), m.sample_many(prompts, **nocfg)
    monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', 'continuous')
    cont, cont_nocfg = m.sample_many(prompts, **kw), m.sample_many(prompts, **nocfg)
    monkeypatch.setattr(sampling, '_COMPACT', True)
    monkeypatch.setattr(sampling, '_COMPACT_STEP', 64)
    comp, comp_nocfg = m.sample_many(prompts, **kw), m.sample_many(prompts, **nocfg)
    n_mod = [sum(isinstance(p, tuple) for p in s) for s in phased]
    print('modalities per sample:', n_mod)
    assert max(n_mod) >= 3 and len(set(n_mod)) > 1, 'the test needs samples that pass through several modality phases, out of step with each other'
    for what, ref, other in (('continuous vs phased', phased, cont), ('continuous vs phased, no guidance', phased_nocfg, cont_nocfg),
                             ('compacted vs dense mixed steps', cont, comp), ('compacted vs dense, no guidance', cont_nocfg, comp_nocfg)):
        compare_samples(f'{method}: {what}', ref, other, 2e-2)


def test_midpoint_named_is_the_default_model_to_the_bit(monkeypatch):
    sd, prompts, kw = schedule_setup()
    named, default = schedule_model('midpoint', sd), schedule_model(None, sd)
    for schedule in ('phased', 'continuous'):
        monkeypatch.setenv('TFX_SAMPLE_SCHEDULE', schedule)
        for a, b in zip(named.sample_many(prompts, **kw), default.sample_many(prompts, **kw)):
            assert len(a) == len(b)
            for pa, pb in zip(a, b):
                assert (pa[0] == pb[0] and torch.equal(pa[1], pb[1])) if isinstance(pa, tuple) else torch.equal(pa, pb)
    noise = torch.randn(2, 3, 3, 16, generator=torch.Generator().manual_seed(1))
    named._gen_noise_override = default._gen_noise_override = noise
    assert torch.equal(named.generate_modality_only(batch_size=2, modality_type=1, modality_steps=4), default.generate_modality_only(batch_size=2, modality_type=1, modality_steps=4))


def golden_model(method):
    from oracle.make_golden_sampling import sampling_case
    from transfusion_pytorch_amd import Transfusion
    cfg, sd, prompts, noise = sampling_case(False, False)
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=cfg.dim_latents[0], modality_default_shape=(4,), eps=cfg.eps,
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), odeint_kwargs=dict(method=method))
    m.load_state_dict(sd)
    return m.cuda().eval(), prompts, noise


def plain(sample):
    return [('mod', int(p[0]), p[1].float().cpu()) if isinstance(p, tuple) else ('text', p.cpu().long()) for p in sample]


SAMPLE_EQ_ATOL = 1e-4                                        # the reference's own tolerance (tests/test_sampling_gpu.py)
GOLDEN_KW = dict(max_length=10, text_temperature=0., modality_steps=4, fixed_modality_shape=(4,), cfg_scale=3., force_modality_at_start=0)


@pytest.mark.parametrize('method', RK.NEW_METHODS)
def test_sample_one_equals_sample_many(method):
    m, prompts, noise = golden_model(method)
    kw = dict(GOLDEN_KW, init_modality_noise=noise)
    many = m.sample_many([prompts[0], prompts[1]], **kw)
    one = m.sample_one(prompts[0], **kw)
    n_mod = 0
    for a, b in zip(plain(many[0]), plain(one)):
        assert a[0] == b[0]
        if a[0] == 'text':
            assert a[1].tolist() == b[1].tolist()
        else:
            d_abs = float((a[2] - b[2]).abs().max()); n_mod += 1
            print(f'{method}: sample_one vs sample_many modality: max |delta| {d_abs:.3e}')
            assert d_abs <= SAMPLE_EQ_ATOL
    assert n_mod >= 1


@pytest.mark.parametrize('method', RK.NEW_METHODS)
def test_single_sample_loop_through_forward(method):
    """the loop written against the public decode contract of forward() (one tfx_ode_rk_axpy per evaluation, the kv cache handed on is the one the last
    evaluation of the last step returned) against the batched decoder, as tests/test_decode_contract_gpu.py compares them for midpoint: the first
    decoded modality within that test's 3e-2, without guidance cached and un-cached, with guidance cached"""
    m, prompts, noise = golden_model(method)
    kw = dict(max_length=14, text_temperature=0., init_modality_noise=noise, modality_steps=3, fixed_modality_shape=(4,), force_modality_at_start=0)
    mod = lambda parts: next(p for p in parts if isinstance(p, tuple))[1].float()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for cfg_scale, cache_kv in ((1., True), (1., False), (3., True)):
        want = mod(m.sample_one(prompts[0].cuda(), cfg_scale=cfg_scale, **kw))
        got = mod(m._sample_one_through_forward(prompts[0].cuda(), cache_kv=cache_kv, cfg_scale=cfg_scale, **kw))
        e = rel(got, want)
        print(f'{method}: forward() loop cfg {cfg_scale} cache_kv {cache_kv} vs sample_one, first modality: {e:.2e}')
        assert got.shape == want.shape and e <= 3e-2


@pytest.mark.parametrize('method', RK.NEW_METHODS)
def test_generate_modality_only_runs_the_method(method):
    """against `rk_solve`'s loop in fp32 on the device with the model's own forward_modality as f: 2e-2 rel-Frobenius, and exactly stages x 3 evaluations"""
    sd, _, _ = schedule_setup()
    m = schedule_model(method, sd)
    noise = torch.randn(2, 3, 3, 16, generator=torch.Generator().manual_seed(1))
    m._gen_noise_override = noise
    calls = []
    inner = m.forward_modality
    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    m.forward_modality = counted
    got = m.generate_modality_only(batch_size=2, modality_type=1, modality_steps=4)
    assert len(calls) == RK.stages(method) * 3
    f = lambda t, y: inner(y, times=torch.as_tensor(t, dtype=torch.float32, device=DEV).expand(2), modality_type=1, encode_modality=False, return_loss=False).float()
    with torch.no_grad():
        want = RK.rk_solve(method, f, noise.to(DEV), torch.linspace(0., 1., 4, device=DEV))
    rel = float((got - want).norm() / want.norm())
    print(f'{method}: generate_modality_only vs rk_solve on the device: rel-Frobenius {rel:.3e}')
    assert got.shape == want.shape and rel <= 2e-2


# ---------------------------------------------------------------------------------------------- 11. plans kept between calls
def test_kept_decode_plans_belong_to_their_method():
    rk4, prompts, noise = golden_model('rk4')
    kw = dict(GOLDEN_KW, init_modality_noise=noise)
    ps = [prompts[0], prompts[1]]
    def same(x, y):
        for sa, sb in zip(x, y):
            for a, b in zip(plain(sa), plain(sb)):
                assert a[0] == b[0] and (torch.equal(a[1], b[1]) if a[0] == 'text' else torch.equal(a[2], b[2]))
    first = rk4.sample_many(ps, **kw)
    kept = rk4._decode_keep
    assert kept is not None and len(kept['plans']) > 0 and 'rk4' in kept['key']
    ids = {k: id(p) for k, p in kept['plans'].items()}
    second = rk4.sample_many(ps, **kw)
    assert rk4._decode_keep['joint'] is kept['joint']
    assert all(id(rk4._decode_keep['plans'][k]) == v for k, v in ids.items()), 'the second call must run on the plans of the first'
    same(first, second)
    n_inst = lambda m: {p.inst_time.numel() for k, p in m._decode_keep['plans'].items() if k[0] in ('mix', 'mixc')}
    assert n_inst(rk4) == {4 * 3 + 1}
    mid, _, _ = golden_model('midpoint')
    mid.sample_many(ps, **kw)
    assert n_inst(mid) == {2 * 3 + 1} and mid._decode_keep['joint'] is not kept['joint']
    # the same weights under another solver: handed the rk4 model's kept plans, the call must not take them (other conditioning times, other control block)
    euler, _, _ = golden_model('euler')
    cold = euler.sample_many(ps, **kw)
    euler._decode_keep = dict(rk4._decode_keep, key=(*rk4._decode_keep['key'][:3], euler.store.params_version(), *rk4._decode_keep['key'][4:]))
    assert euler._decode_keep['key'][:-1] == (*kept['key'][:3], euler.store.params_version(), *kept['key'][4:-1])
    again = euler.sample_many(ps, **kw)
    assert euler._decode_keep['joint'] is not kept['joint'] and n_inst(euler) == {3 + 1}
    same(cold, again)
    same(second, rk4.sample_many(ps, **kw))
