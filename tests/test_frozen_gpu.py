"""Frozen parameters (`p.requires_grad_(False)` on native parameters) on the MI355X.

The reference runs on autograd, so a frozen run there gives the unfrozen run's loss and the unfrozen run's gradients on the trainable parameters, and
`.grad is None` on the frozen ones: the existing goldens (small2, head8, text1, flow1, f4b_unet, selfflow_taps_small2) hold the expected numbers.

  kernels     NULL parameter-gradient outputs (tfx.h): every other output of the call bit-identical where no atomic is involved, the remaining sums
              inside the bounds of tests/_tokenwise_cases.py, guard bands intact, the buffer that would have been the output untouched
  model       per freeze set (tests/_frozen_cases.py): loss, `.grad is None` exactly on the frozen parameters, all-zero bits in their segments of the
              gradient buffer, trainable gradients under the bounds of tests/test_model_gpu.py
  lists       what the backward list of a set holds and where it ends
  optimizers  three steps of the four fused optimizers: frozen values and moments bit-equal to the initial ones, trainable elements bit-equal to an
              unfrozen twin that was fed the same gradient bits
  hazards     user encoder / decoder around a frozen trunk, a hidden tap over frozen layers, accumulation, a frozen EMA teacher"""
import ctypes
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _frozen_cases as F                                         # noqa: E402
import _tokenwise_cases as C                                      # noqa: E402
from transfusion_pytorch_amd import capi                          # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16
GOLDEN = os.path.join(HERE, 'golden')
LOGIT_TOL, GRAD_TOL, GRAD_MEAN_TOL, GRAD_HEAD_TOL = 1e-2, 4e-2, 1.2e-2, 8e-2      # tests/test_model_gpu.py
LOSS_TOL = 1e-3
MARGIN = 1.5                                                      # the project's margin over a measured figure (tests/test_model_gpu.py docstring)


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ================================================================================================ kernels: NULL parameter-gradient outputs
D_SMALL, T_TRIP = 64, 4101            # the smallest width class (NC = 1) and the token count that sends five tokens through a second grid-stride trip


def _untouched(o):
    return torch.equal(o.buf, o.before)


def _null_runs(build_outs, make_args, launch, nullable, atomic, exact, refill=None):
    """the full call, the call with each pointer of `nullable` NULL, and with all of them NULL.  `exact`: outputs no atomic touches - bit-equal to the
    full call's; `atomic`: accumulated sums - inside their derived bounds (check_outs also proves the guard bands); a NULLed output's buffer is untouched"""
    def run(nulls):
        o = build_outs()
        a = make_args(o)
        for holder, field in nulls:
            setattr(a[holder], field, None)
        launch(*a); sync()
        if refill is not None:
            refill(o)
        names = {f for _, f in nulls}
        C.check_outs(f'NULL {sorted(names)}', [getattr(o, n) for n in exact + atomic if n not in names])
        for n in names:
            assert _untouched(getattr(o, n)), f'{n} was NULL and its would-be buffer changed'
        return o
    full = run([])
    for nulls in [[n] for n in nullable] + ([list(nullable)] if len(nullable) > 1 else []):
        o = run(nulls)
        for n in exact:
            if n in {f for _, f in nulls}:
                continue                                          # (that output was NULL in this run: untouched, checked above)
            assert torch.equal(getattr(o, n).view, getattr(full, n).view), f'{n} differs from the full call with {nulls} NULL'


def _ns(**kw):
    from types import SimpleNamespace
    return SimpleNamespace(**kw)


def _pre_args(c, o, seg):
    return capi.make_args('tfx_adaln_pre_args', T=c.T, d=c.d, x=c.x, tok_inst=c.tok, table=c.table, ld_table=c.ld, gamma_text=c.gamma_text, mean=c.mean32, rstd=c.rstd32,
                          du=c.du, dx=o.dx.view, dtable=o.dtable.view, dgamma_text=o.dgamma_text.view,
                          **(dict(seg_start=c.seg_start, seg_len=c.seg_len, n_seg=c.lay.n_seg) if seg else {}))


def _post_args(c, o, seg, g=None, dtable=None):
    return capi.make_args('tfx_adaln_post_args', T=c.T, d=c.d, x=c.x, y=c.y, tok_inst=c.tok, table=c.table.data_ptr() + 4 * c.post_col0, ld_table=c.ld,
                          layerscale=c.layerscale, g=c.g if g is None else g, dy=o.dy.view,
                          dtable=(o.dtable.view if dtable is None else dtable).data_ptr() + 4 * c.post_col0, dlayerscale=o.dlayerscale.view, dbias=o.dbias.view,
                          **(dict(seg_start=c.seg_start, seg_len=c.seg_len, n_seg=c.lay.n_seg) if seg else {}))


@pytest.mark.parametrize('seg', (False, True), ids=('per_token', 'segments'))
def test_adaln_pre_bwd_null_dgamma_text_and_dtable(seg):
    c = C.build_adaln(C.layout('scatter' if not seg else 'runs', T_TRIP), D_SMALL, DEV)
    call = lambda a: capi.call('tfx_adaln_pre_bwd', a, stream())
    _null_runs(lambda: C.outs_pre_bwd(c, seg), lambda o: [_pre_args(c, o, seg)], call, [(0, 'dgamma_text'), (0, 'dtable')],
               atomic=['dgamma_text'] + ([] if seg else ['dtable']), exact=['dx'] + (['dtable'] if seg else []))


@pytest.mark.parametrize('seg', (False, True), ids=('per_token', 'segments'))
def test_adaln_post_bwd_null_dlayerscale_dbias_and_dtable(seg):
    c = C.build_adaln(C.layout('scatter' if not seg else 'runs', T_TRIP), D_SMALL, DEV)
    call = lambda a: capi.call('tfx_adaln_post_bwd', a, stream())
    _null_runs(lambda: C.outs_post_bwd(c, seg), lambda o: [_post_args(c, o, seg)], call, [(0, 'dlayerscale'), (0, 'dbias'), (0, 'dtable')],
               atomic=['dlayerscale', 'dbias'] + ([] if seg else ['dtable']), exact=['dy'] + (['dtable'] if seg else []))


def test_adaln_pre_post_bwd_fused_null_outputs():
    """the fused launch of two wrapper sides (segment mode): the input side's dgamma_text and the output side's dlayerscale, each alone and both; then
    the two sides' dtable pointers, which are independent"""
    c = C.build_adaln(C.layout('runs', 1001, balance=True), D_SMALL, DEV, wrappers=2)

    def outs():
        op, oq = C.outs_pre_bwd(c, True), C.outs_post_bwd(c, True)
        return _ns(dx=op.dx, dtable=op.dtable, dgamma_text=op.dgamma_text, dy=oq.dy, dlayerscale=oq.dlayerscale, q=oq, p=op)

    def args(o):
        b = _post_args(c, o.q, True, g=o.dx.view, dtable=o.dtable.view)
        b.dbias = None                                            # (the fused entry takes no bias gradient)
        return [_pre_args(c, o.p, True), b]

    def launch(a, b):
        capi.check(capi.lib().tfx_adaln_pre_post_bwd(ctypes.byref(a), ctypes.byref(b), stream()), 'tfx_adaln_pre_post_bwd')

    def refill(o):
        C.refill_post_bwd(c, o.q, True, o.dx.view)
        o.tab = C.merge_tables(o.p.dtable, o.q.dtable)

    _null_runs(outs, args, launch, [(0, 'dgamma_text'), (1, 'dlayerscale')], atomic=['dgamma_text', 'dlayerscale'], exact=['dx', 'dy', 'tab'], refill=refill)
    # the two sides' table gradients, each NULL alone and both: the other side's columns are the full call's bits (stored, no atomics), the NULL side's
    # columns and everything around them keep what the buffer held
    d = D_SMALL
    zc = slice(c.post_col0 + 2 * d, c.post_col0 + 3 * d)

    def run(null_pre, null_post):
        o = outs()
        a, b = args(o)
        if null_pre:
            a.dtable = None
        if null_post:
            b.dtable = None
        launch(a, b); sync()
        return o

    full = run(False, False)
    before = full.dtable.before
    inner = lambda o: o.dtable.view
    for null_pre, null_post in ((True, False), (False, True), (True, True)):
        o = run(null_pre, null_post)
        assert torch.equal(o.dx.view, full.dx.view) and torch.equal(o.dy.view, full.dy.view), (null_pre, null_post)
        want = inner(full).clone()
        held = o.dtable.before[C.GUARD:C.GUARD + want.shape[0]]
        if null_pre:
            want[:, :2 * d] = held[:, :2 * d]
        if null_post:
            want[:, zc] = held[:, zc]
        assert torch.equal(inner(o), want), f'table gradient with pre NULL={null_pre}, post NULL={null_post}'
        guard = torch.ones(o.dtable.buf.shape[0], dtype=torch.bool, device=DEV); guard[C.GUARD:C.GUARD + want.shape[0]] = False
        assert torch.equal(o.dtable.buf[guard], o.dtable.before[guard]), 'guard bands'
        assert torch.equal(before, o.dtable.before)


@pytest.mark.parametrize('d', (D_SMALL, 1032), ids=('d64', 'd1032-NC4'))
def test_rmsnorm_bwd_null_dgamma(d):
    c = C.build_rmsnorm(T_TRIP, d, DEV)

    def args(o):
        return [capi.make_args('tfx_rmsnorm_args', T=c.T if hasattr(c, 'T') else T_TRIP, d=d, x=c.x, y=o.y.view, gamma=c.gamma, dy=c.dy, dx=o.dx.view, dgamma=o.dgamma.view)]

    def launch(a):
        capi.call('tfx_rmsnorm_fwd', a, stream()); capi.call('tfx_rmsnorm_bwd', a, stream())

    _null_runs(lambda: C.outs_rmsnorm(c), args, launch, [(0, 'dgamma')], atomic=['dgamma'], exact=['y', 'dx'])


@pytest.mark.parametrize('first', (0, 1))
def test_attnres_push_bwd_null_dgamma_and_dpq(first):
    c = C.build_attnres(T_TRIP, D_SMALL, 3, DEV, zero_row=False)

    def args(o):
        return [capi.make_args('tfx_attnres_args', T=c.T, d=c.d, L=c.L, hiddens=c.H, stride_h=c.T * c.d, gamma=c.gamma, pq=c.pq, g=c.g, g2=None if first else c.g2,
                               dhiddens=o.dhiddens.view, stride_dh=c.T * c.d, first=first, dgamma=o.dgamma.view, dpq=o.dpq.view)]

    _null_runs(lambda: C.outs_attnres_bwd(c, first), args, lambda a: capi.call('tfx_attnres_bwd', a, stream()), [(0, 'dgamma'), (0, 'dpq')],
               atomic=['dgamma', 'dpq'], exact=['dhiddens'])


def test_attnres_pull_bwd_null_wrapper_outputs_and_finish_null_records():
    """the pull form with its fused wrapper side (segments and one token per wave): dlayerscale / dbias NULL leave dh, dy and the stored table gradient
    bit-identical; tfx_attnres_finish with a NULL dgamma or dpq in a source record adds the other and touches nothing else"""
    import test_tokenwise_rows_gpu as R
    for kind, segs in (('model', True), ('runs', False)):
        c = C.build_adaln(C.layout(kind, 130, balance=True), D_SMALL, DEV)
        p = R._pull_case(c)

        def outs():
            oq = C.outs_post_bwd(c, segs)
            return _ns(dh=C.new_out('dh', c.T, D_SMALL, BF, DEV), dy=oq.dy, dtable=oq.dtable, dlayerscale=oq.dlayerscale, dbias=oq.dbias, q=oq)

        def args(o):
            a = capi.make_args('tfx_attnres_pull_args', T=c.T, d=D_SMALL, l=1, n_src=2, h=p.H[1], src=p.tab.data_ptr(), out_own=p.outs[0], out_err=p.errs[0], dh=o.dh.view,
                               **R.seg_kw(c, segs))
            return [a, _post_args(c, o.q, segs, g=o.dh.view)]

        def launch(a, b):
            capi.check(capi.lib().tfx_attnres_prep(p.tab.data_ptr(), 2, D_SMALL, stream()), 'prep')
            R.call2('tfx_attnres_pull_bwd', a, b)

        def refill(o):
            o.dh.ref, o.dh.tol, _, _ = C.pull_ref(p.H[1], [p.G[0], p.G[1]], p.saves, 1, p.own, [p.wtab[0, 0], p.wtab[0, 1]])
            C.refill_post_bwd(c, o.q, segs, o.dh.view)

        _null_runs(outs, args, launch, [(1, 'dlayerscale'), (1, 'dbias'), (1, 'dtable')], atomic=['dlayerscale', 'dbias'] + ([] if segs else ['dtable']),
                   exact=['dh', 'dy'] + (['dtable'] if segs else []), refill=refill)
    # finish: records with one or both parameter gradients NULL
    d, Dn = D_SMALL, 2
    g = C.gen(d, Dn, 77)
    gm, pq, dw = ((torch.randn(Dn, d, generator=g) * 0.5).to(DEV) for _ in range(3))
    w = torch.zeros(Dn, d, device=DEV)
    SRC = capi.STRUCTS['tfx_attnres_src']

    def finish(null):
        dgm, dpq = torch.full((Dn, d + 16), 3., device=DEV), torch.full((Dn, d + 16), 5., device=DEV)
        recs = (SRC * Dn)()
        for j in range(Dn):
            for k, v in dict(w=w[j], dw=dw[j], gamma=gm[j], pq=pq[j], dgamma=dgm[j], dpq=dpq[j]).items():
                setattr(recs[j], k, None if (j, k) in null else v.data_ptr())
            recs[j].L = j + 2
        tab = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(recs), ctypes.sizeof(recs))), dtype=torch.uint8).to(DEV)
        capi.check(capi.lib().tfx_attnres_finish(tab.data_ptr(), Dn, d, stream()), 'finish'); sync()
        return dgm, dpq

    full = finish(())
    assert torch.allclose(full[0][:, :d], 3. + dw * pq, rtol=1e-6, atol=1e-6) and torch.allclose(full[1][:, :d], 5. + dw * (1. + gm), rtol=1e-6, atol=1e-6)
    assert bool((full[0][:, d:] == 3.).all()) and bool((full[1][:, d:] == 5.).all())
    for null in ([(0, 'dgamma')], [(1, 'dpq')], [(0, 'dgamma'), (0, 'dpq'), (1, 'dgamma')]):
        got = finish(set(null))
        for which, name in enumerate(('dgamma', 'dpq')):
            for j in range(Dn):
                want = torch.full_like(full[which][j], (3., 5.)[which]) if (j, name) in null else full[which][j]
                assert torch.equal(got[which][j], want), (null, j, name)


# ================================================================================================ model
def _golden(name):
    return torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)


def _build(cfg, sd):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, step) of a golden case, built once and shared by the freeze sets: `step()` runs forward + backward and returns the loss"""
    from oracle import cases as OC
    if name == 'text1':
        cfg, sd, text = OC.build_text_case(name)
        model = _build(cfg, sd)
        return model, lambda: model.forward_text(text)
    if name == 'flow1':
        cfg, sd, x, times, noise, ty = OC.build_modality_case(name)
        model = _build(cfg, sd)
        model._noise_override = {ty: noise.cuda()}
        return model, lambda: model.forward_modality(x, times=times, modality_type=ty)
    cfg, sd, batch, times, noise = OC.build_case(name)
    model = _build(cfg, sd)
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    return model, lambda: model(batch, times=times)


def _step(name):
    model, fwd = _case(name)
    for p in model.parameters():
        p.grad = None
    loss = fwd()
    loss.backward()
    sync()
    return model, float(loss.detach())


def _grad_errors(model, g, names):
    """per-parameter error of the gradients of `names` against golden `g` by the rule of the golden's own test (tests/test_model_gpu.py): full gradients
    (small2, head8) rel-Frobenius <= GRAD_TOL; norms + heads (text1, flow1) norm <= GRAD_TOL, 1024-element head <= GRAD_HEAD_TOL.  Returns {name: (error, norm)}."""
    named = dict(model.named_parameters())
    out = {}
    for k in names:
        gn = float(g['grad_norms'].get(k, 0.))
        if gn < 1e-7:
            continue
        grad = named[k].grad
        assert grad is not None, f'no gradient for trainable {k}'
        if 'grads' in g:
            e = rel(grad.float(), g['grads'][k])
            assert e <= GRAD_TOL, f'gradient {k}: rel err {e:.3e}'
        else:
            e_norm = abs(float(grad.double().norm()) - gn) / gn
            assert e_norm <= GRAD_TOL, f'gradient norm {k}: rel err {e_norm:.3e}'
            head = g['grad_head'][k]
            e = rel(grad.float().reshape(-1)[:head.numel()], head) if float(head.norm()) > 1e-3 * gn else 0.      # (a head of a small-norm gradient is noise: tests/test_model_gpu.py)
            assert e <= GRAD_HEAD_TOL, f'gradient head {k}: rel err {e:.3e}'
            e = max(e, e_norm)
        out[k] = (e, gn)
    return out


def _mean(errs):
    den = sum(gn for _, gn in errs.values())
    return sum(e * gn for e, gn in errs.values()) / den if den else 0.


@functools.lru_cache(maxsize=None)
def _unfrozen_errors(name):
    """the unfrozen run of the case, measured once: its per-parameter gradient errors (for the norm-weighted mean over a set's trainable subset)"""
    model, _ = _case(name)
    F.unfreeze(model)
    model, loss = _step(name)
    return _grad_errors(model, _golden(name), list(model.store.params)), loss


@pytest.mark.parametrize('set_name', list(F.SETS))
@pytest.mark.parametrize('name', ['small2', 'head8', 'text1', 'flow1'])
def test_frozen_run_gives_the_unfrozen_gradients_on_the_trainable_parameters(name, set_name):
    """GRAD_MEAN_TOL is the bound of the norm-weighted mean over ALL parameters; over a set's trainable subset the same quantity is measured on the
    unfrozen run of the case and the frozen run held to 1.5 x that where it exceeds GRAD_MEAN_TOL (both are printed; profiles/frozen_params.txt)"""
    g = _golden(name)
    base, base_loss = _unfrozen_errors(name)
    model, _ = _case(name)
    ps = model.store
    frozen, train = F.freeze(model, set_name)
    try:
        model, loss = _step(name)
        ref = float(g['loss'])
        print(f'  [{name} / {set_name}] loss {loss:.6f} reference {ref:.6f} (unfrozen run {base_loss:.6f}); {len(train)} of {len(ps.params)} parameters train')
        assert abs(loss - ref) <= LOSS_TOL * max(1., abs(ref))
        for n, p in ps.params.items():
            assert (p.grad is None) == (n in frozen), f'{n}: .grad is {"None" if p.grad is None else "set"}'
        for a, b in ps.frozen_ranges():
            assert not bool(ps.grad[a:b].view(torch.int32).any()), f'frozen range [{a}, {b}) of the gradient buffer is not all-zero bits'
        errs = _grad_errors(model, g, train)
        if errs:
            sub = {k: base[k] for k in errs}
            bound = max(GRAD_MEAN_TOL, MARGIN * _mean(sub))
            print(f'  trainable gradients: norm-weighted mean {_mean(errs):.3e} (unfrozen run, same subset: {_mean(sub):.3e}; bound {bound:.3e}); '
                  f'worst {max(errs, key=lambda k: errs[k][0])} {max(e for e, _ in errs.values()):.3e}')
            assert _mean(errs) <= bound
        plan = model._live[0]
        if set_name == 'all_frozen':
            assert plan.bwd_end == 0
    finally:
        F.unfreeze(model)


# ================================================================================================ backward lists
def _tn_records(plan, lst=None):
    """every weight-gradient product of a list: the structs of single launches, `group_next` chains and table records"""
    REC = capi.STRUCTS['tfx_gemm_tn_args']
    out = []
    for item in (plan.bwd if lst is None else lst):
        fn, a = item
        if fn != 'tfx_gemm_tn':
            continue
        if a.table_count:
            host = a._table[0]
            out += [REC.from_buffer_copy(host, k * ctypes.sizeof(REC)) for k in range(a.table_count)]
        else:
            out += [a] + list(getattr(a, '_chain', []))
    return out


def _written_ranges(ps, rec):
    """element ranges of the gradient buffer a product writes: rows rowmap[n] >= 0 (or every row) x k_valid columns, and its colsum"""
    base, nb = ps.grad.data_ptr(), ps.numel * 4
    if not rec.C or not (base <= rec.C < base + nb):
        return []
    c0 = (rec.C - base) // 4
    kcols = rec.k_valid if not rec.k_group else (rec.k_valid // 64) * rec.k_group
    rows = range(rec.N)
    if rec.rowmap:
        m = next(t for t in ps._maps.values() if t.data_ptr() == rec.rowmap).cpu().tolist()
        rows = sorted({r for r in m[:rec.N] if r >= 0})
    out = [(c0 + r * rec.ldc, c0 + r * rec.ldc + kcols) for r in rows]
    if rec.colsum and base <= rec.colsum < base + nb:
        out.append(((rec.colsum - base) // 4, (rec.colsum - base) // 4 + 1))
    return out


def _ops(lst):
    return [fn if isinstance(fn, str) else fn.__name__ for fn, _ in lst]


@pytest.mark.parametrize('set_name', list(F.SETS))
def test_no_weight_gradient_product_targets_a_frozen_parameter(set_name):
    model, _ = _case('small2')
    ps = model.store
    frozen, train = F.freeze(model, set_name)
    try:
        _step('small2')
        plan = model._live[0]
        assert plan._frozen == frozenset(frozen)
        mask = torch.zeros(ps.numel, dtype=torch.bool)
        for a, b in ps.frozen_ranges():
            mask[a:b] = True
        recs = _tn_records(plan)
        for rec in recs:
            for a, b in _written_ranges(ps, rec):
                assert not bool(mask[a:b].any()), f'a weight-gradient product writes [{a}, {b}) of a frozen segment'
        ops = _ops(plan.bwd)
        assert 'tfx_embed_bwd' not in ops
        if 'text_embed.weight' in frozen:
            emb = ps.grad_ptr('text_embed.weight')
            assert all(rec.C != emb for rec in recs) and 'tfx_onehot_bf16' not in ops
        print(f'  [{set_name}] {len(plan.bwd)} launches ({len(recs)} weight-gradient products), the backward ends at {plan.bwd_end}')
    finally:
        F.unfreeze(model)


def test_the_chain_stops_at_the_lowest_consumer():
    """top_half: the list ends behind layer depth / 2 (and what is left of the AttentionResidual parameter sums runs as its own short list); heads: behind the
    output projections' products; all_frozen: nothing runs; a hidden tap or rows for PyTorch put the whole chain back (hazard tests below)"""
    model, _ = _case('small2')
    ps, D = model.store, model.md.depth
    try:
        F.freeze(model, 'top_half')
        _step('small2')
        plan = model._live[0]
        assert plan.bwd_end is not None and 0 < plan.bwd_end < len(plan.bwd)
        prefix = plan.bwd[:plan.bwd_end]
        low_ptrs = set()
        for i in range(D // 2):
            low_ptrs |= {plan.yf[i].data_ptr(), plan.ya[i].data_ptr(), plan.ag[i].data_ptr(), plan.xb[i].data_ptr(), plan.og[i].data_ptr()}
        def touches(a):
            vals = []
            for f, _ in getattr(a, '_fields_', []):
                v = getattr(a, f)
                if isinstance(v, int):
                    vals.append(v)
            return low_ptrs & set(vals)
        for fn, a in prefix:
            if isinstance(fn, str) and hasattr(a, '_fields_'):
                assert not touches(a), f'{fn} in the truncated list reads an activation of a layer below depth / 2'
        per_layer = [op for op in _ops(prefix) if op == 'tfx_attn_bwd']
        assert len(per_layer) == D - D // 2, 'one attention backward per trainable layer, none below'
        assert plan.ar_tail is not None and _ops(plan.ar_tail).count('tfx_attnres_pull_bwd') == D // 2 + 1
        F.freeze(model, 'heads')
        _step('small2')
        plan = model._live[0]
        ops = _ops(plan.bwd[:plan.bwd_end])
        assert ops and set(ops) == {'tfx_gemm_tn'} and plan.ar_tail is None
        F.freeze(model, 'all_frozen')
        for p in model.parameters():
            p.grad = None
        loss = _case('small2')[1]()
        plan = model._live[0]
        mark = torch.full_like(plan.dembed, 7.)
        plan.dembed.copy_(mark)
        seeds = plan.dlogits.clone()
        (loss * 3.).backward(); sync()
        assert plan.bwd_end == 0 and torch.equal(plan.dembed, mark) and torch.equal(plan.dlogits, seeds), 'a backward with nothing trainable launched something'
        assert all(p.grad is None for p in ps.params.values()) and not bool(ps.grad.view(torch.int32).any())
    finally:
        F.unfreeze(model)


def test_unfreezing_returns_the_list_of_a_run_that_never_froze():
    """freeze, step, unfreeze: the plan's current list is the object it was before, with the fingerprint (every byte a graph capture would freeze) it had"""
    from transfusion_pytorch_amd.optim import FusedAdam
    model, _ = _case('head8')
    F.unfreeze(model)

    def fingerprint(lst):
        fp = ctypes.c_int64()
        assert capi.lib().tfx_list_fingerprint(lst.native(), len(lst), ctypes.byref(fp)) == 0
        return fp.value

    _step('head8')
    plan = model._live[0]
    lst0, fp0, cuts0 = plan.bwd, fingerprint(plan.bwd), list(plan.bwd_cuts)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        for s in ('v_only', 'bias_gain', 'heads', 'top_half', 'text_frozen', 'all_frozen'):      # more sets than a plan keeps lists for
            F.freeze(model, s)
            _step('head8')
            assert model._live[0] is plan and plan.bwd is not lst0
        opt = FusedAdam(model, lr=1e-4)
        F.freeze(model, 'v_only')
        _step('head8')
        opt.step()
        F.unfreeze(model)
        _step('head8')
        assert plan.bwd is lst0 and fingerprint(plan.bwd) == fp0 and plan.bwd_cuts == cuts0 and plan.bwd_end is None
        assert len(plan._bwd_sets) <= plan._BWD_SETS + 1
    finally:
        F.unfreeze(model)
        model.load_state_dict(sd)


def test_frozen_lists_replay_as_graphs_and_unfreezing_returns_to_the_first_capture(monkeypatch):
    """TFX_TRAIN_GRAPH=1 (LaunchList.replay_auto): the truncated list of a frozen set is captured as its own graph over [0, bwd_end), its results equal the
    list replay's to atomic-ordering noise (the bound of that mode's own test, 2e-3), and after unfreezing the plan is back on the first list"""
    from oracle.cases import build_case
    from transfusion_pytorch_amd import engine
    cfg, sd, batch, times, noise = build_case('small2')

    def fresh():
        m = _build(cfg, sd)
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        return m

    def steps(model, n):
        outs = []
        for _ in range(n):
            for p in model.parameters():
                p.grad = None
            loss = model(batch, times=times)
            loss.backward(); sync()
            outs.append((float(loss), {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}))
        return outs

    ref = fresh()
    F.freeze(ref, 'top_half')
    ref_loss, ref_grads = steps(ref, 1)[0]
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    model = fresh()
    full = steps(model, 4)
    plan = model._live[0]
    lst0 = plan.bwd
    assert lst0._auto[(0, len(lst0))][1], 'the unfrozen loop must be on graph replays'
    frozen, train = F.freeze(model, 'top_half')
    outs = steps(model, 5)
    assert plan.bwd is not lst0 and plan.bwd_end is not None
    st = plan.bwd._auto[(0, plan.bwd_end)]
    assert st[1] and st[2] >= 4, 'the truncated list must end up on graph replays'
    for i, (l, g) in enumerate(outs):
        assert abs(l - ref_loss) <= 1e-6 * max(1., abs(ref_loss)) and set(g) == set(ref_grads), i
        for k in ref_grads:
            assert rel(g[k], ref_grads[k]) <= 2e-3, (i, k)
    for a, b in model.store.frozen_ranges():
        assert not bool(model.store.grad[a:b].view(torch.int32).any())
    F.unfreeze(model)
    again = steps(model, 2)
    assert plan.bwd is lst0 and lst0._auto[(0, len(lst0))][1], 'unfreezing returns to the first list and its capture'
    for k, v in full[-1][1].items():
        assert rel(again[-1][1][k], v) <= 2e-3, k


# ================================================================================================ optimizers
def _small(seed=0):
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(seed)
    return Transfusion(num_text_tokens=32, dim_latent=16, add_pos_emb=True, modality_num_dim=1, transformer=dict(dim=64, depth=2, heads=2, dim_head=8)).cuda().train()


def _grads(model, seed, scale=0.05):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ps = model.store
    flat = torch.randn(ps.numel, device=DEV, generator=gen) * scale
    real = torch.zeros(ps.numel, dtype=torch.bool, device=DEV)
    for n, p in ps.params.items():
        real[ps.offsets[n][0]:ps.offsets[n][0] + p.numel()] = True
    ext = [torch.randn(p.shape, device=DEV, generator=gen) * scale for p in model.external_parameters()]
    return flat * real, ext


def _inject(model, grads, frozen_mask):
    model.store.grad.copy_(grads[0] * ~frozen_mask)                # the frozen segments carry zeros, as a frozen backward leaves them
    for p, g in zip(model.external_parameters(), grads[1]):
        p.grad = g.clone()


def _mask(ps):
    m = torch.zeros(ps.numel, dtype=torch.bool, device=DEV)
    for a, b in ps.frozen_ranges():
        m[a:b] = True
    return m


def _make(kind, model, **kw):
    from transfusion_pytorch_amd import optim as O
    cls = getattr(O, kind)
    opt = cls(model, max_grad_norm=0.5, **kw)
    opt.deterministic_norm = True
    return opt


OPTS = ('FusedAdam', 'FusedAdamAtan2', 'FusedMuon', 'FusedMuonAdamAtan2')


@pytest.mark.parametrize('decay', (False, True), ids=('plain', 'decay_groups'))
@pytest.mark.parametrize('set_name', ['top_half', 'bias_gain', 'v_only', 'heads', 'all_frozen'])
@pytest.mark.parametrize('kind', OPTS)
def test_fused_optimizers_leave_frozen_parameters_and_their_state_alone(kind, set_name, decay):
    """fails on a tree without the skip table: Adam's moments and the weight decay move a frozen parameter (the gradient there is zero, the update is not)"""
    from transfusion_pytorch_amd.optim import decay_groups
    a, b = _small(), _small()
    assert torch.equal(a.store.flat, b.store.flat)
    F.freeze(a, set_name)
    fm = _mask(a.store)
    kw = lambda m: dict(param_groups=decay_groups(m, 0.1)) if decay else dict(weight_decay=0.05)
    oa, ob = _make(kind, a, **kw(a)), _make(kind, b, **kw(b))
    p0 = a.store.flat.clone()
    for step in range(3):
        g = _grads(a, 10 + step)
        _inject(a, g, fm); _inject(b, g, fm)
        oa.step(); ob.step()
        if step == 0:
            m0, v0 = oa.m.clone(), oa.v.clone()
            assert not bool(m0[fm].any()) and not bool(v0[fm].any())
    sync()
    assert torch.equal(a.store.flat[fm], p0[fm]), 'a frozen value moved'
    assert torch.equal(oa.m[fm], m0[fm]) and torch.equal(oa.v[fm], v0[fm]) and not bool(oa.m[fm].any()), 'a frozen moment moved'
    if set_name != 'all_frozen':
        assert not torch.equal(a.store.flat[~fm], p0[~fm])
    assert torch.equal(a.store.flat[~fm], b.store.flat[~fm]), 'trainable elements differ from the unfrozen twin'
    assert torch.equal(oa.m[~fm], ob.m[~fm]) and torch.equal(oa.v[~fm], ob.v[~fm])
    for p, q in zip(a.external_parameters(), b.external_parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize('kind', OPTS)
def test_resume_and_a_set_that_changes_between_steps(kind):
    """state_dict() -> a fresh optimizer continues bit-identically with frozen members; the skip table follows a set changed between steps"""
    a, b = _small(), _small()
    F.freeze(a, 'v_only'); F.freeze(b, 'v_only')
    oa, ob = _make(kind, a), _make(kind, b)
    fm = _mask(a.store)
    for step in range(2):
        g = _grads(a, 20 + step)
        _inject(a, g, fm); _inject(b, g, fm)
        oa.step(); ob.step()
    sd = oa.state_dict()
    oc = _make(kind, a)
    oc.load_state_dict(sd)
    assert set(sd['state']) == set(ob.state_dict()['state'])          # the format does not know about frozen parameters
    # the set changes: bias_gain from here on, in both
    F.freeze(a, 'bias_gain'); F.freeze(b, 'bias_gain')
    fm2 = _mask(a.store)
    assert not torch.equal(fm, fm2)
    before = a.store.flat.clone()
    g = _grads(a, 30)
    _inject(a, g, fm2); _inject(b, g, fm2)
    oc.step(); ob.step(); sync()
    assert torch.equal(a.store.flat, b.store.flat) and torch.equal(oc.m, ob.m) and torch.equal(oc.v, ob.v), 'the resumed optimizer left the continued one'
    assert torch.equal(a.store.flat[fm2], before[fm2]) and not torch.equal(a.store.flat[~fm2], before[~fm2])
    assert bool((a.store.flat[fm & ~fm2] != before[fm & ~fm2]).any()), 'a parameter that was unfrozen between the steps did not move'


# ================================================================================================ hazards
def test_user_encoder_decoder_train_around_a_frozen_trunk():
    """f4b_unet with every native parameter frozen: the rows PyTorch receives keep the whole chain, the conv pair's and the positional MLP's gradients are the
    golden's (tests/test_f4b_gpu.py: norms under GRAD_TOL, 64-element heads under GRAD_HEAD_TOL)"""
    from oracle.make_golden_f4b import unet_case, unet_modules
    from transfusion_pytorch_amd import Transfusion
    g = _golden('f4b_unet')
    cfg, sd, batch, times, noises, xm, nm, tm, g0 = unet_case()
    enc, dec = unet_modules(cfg.dim)
    model = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=4, modality_default_shape=(8, 8), channel_first_latent=True,
                        pre_post_transformer_enc_dec=(enc, dec), add_pos_emb=True, modality_num_dim=2, prob_uncond=0.,
                        transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads))
    model.load_state_dict({**sd, **g['ext_sd']}, strict=True)
    model = model.cuda().train()
    model._noise_override = {0: [n.cuda() for n in noises]}
    frozen, train = F.freeze(model, 'all_frozen')
    cu = [[(p[0], p[1].cuda()) if isinstance(p, tuple) else p.cuda() for p in s] for s in batch]
    loss = model(cu, times=times)
    loss.backward(); sync()
    plan = model._live[0]
    assert abs(float(loss) - float(g['loss'])) <= 2e-3 * max(1., abs(float(g['loss'])))        # (that test's loss bound for this fixture)
    assert plan.bwd_end == 0 and plan.rows_in, 'nothing native trains, yet the step hands rows back to PyTorch'
    assert all(p.grad is None for p in model.store.params.values()) and not bool(model.store.grad.view(torch.int32).any())
    ext = {k: p for k, p in model.named_parameters() if k not in model.store.params and p.requires_grad}
    assert ext
    checked = 0
    for k, p in ext.items():
        gn = float(g['grad_norms'].get(k, 0.))
        if gn < 1e-6:
            continue
        assert p.grad is not None, k
        e_norm = abs(float(p.grad.double().norm()) - gn) / gn
        assert e_norm <= GRAD_TOL, (k, e_norm)
        if k in g['grad_heads']:
            e = rel(p.grad.float().reshape(-1)[:64], g['grad_heads'][k])
            assert e <= GRAD_HEAD_TOL, (k, e)
        checked += 1
    print(f'  {checked} external gradients match the golden with the trunk frozen')
    assert checked >= 4


def test_a_hidden_tap_over_frozen_layers_still_delivers_its_gradient():
    """selfflow_taps_small2: the layers below the tap are frozen; what the tap adds to the gradients of the parameters that still train (the embeddings and
    input projections under it, which only the whole chain reaches) is the golden's share, by that fixture's own rule"""
    import _self_flow_cases as SF
    from oracle.cases import build_case
    import test_self_flow_gpu as TS
    g = _golden(SF.TAPS_FIXTURE)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    model = _build(cfg, sd)
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    k = max(i for i in SF.tap_indices(cfg.depth) if 1 <= i <= cfg.depth)
    below = lambda n: n.startswith('transformer.layers.') and int(n.split('.')[2]) < k
    for n, p in model.store.params.items():
        p.requires_grad_(not below(n))
    frozen = [n for n in model.store.params if below(n)]
    assert frozen
    _, gp = TS._plain_grads(model, batch, times)
    t = g['taps'][k]
    model.zero_grad()
    loss, hiddens = model(batch, times=times, return_hiddens=True)
    (loss + t['w'] * hiddens[k].pow(2).mean()).backward(); sync()
    plan = model._live[0]
    named = dict(model.named_parameters())
    assert all(named[n].grad is None for n in frozen)
    share = {nm: named[nm].grad.float() - gp[nm].float() for nm in g['names'] if nm not in frozen}
    live = [nm for nm in share if float(t['share_norms'].get(nm, 0.)) >= 1e-6 * max(t['share_norms'].values())]
    assert live, 'the tap must reach a trainable parameter under the frozen layers'
    TS._share_match(share, t['share_norms'], t['share_head'], t['floor_mean'], t['floor_worst'], f'tap {k} over frozen layers < {k}')


def test_accumulation_over_two_micro_batches_with_modality1():
    from transfusion_pytorch_amd.optim import FusedAdam
    g = _golden('small2')
    model, fwd = _case('small2')
    frozen, train = F.freeze(model, 'modality1')
    try:
        opt = FusedAdam(model, lr=1e-4)
        for p in model.parameters():
            p.grad = None
        with opt.no_sync():
            fwd().backward()
        fwd().backward(); sync()
        named = dict(model.named_parameters())
        for n in frozen:
            assert named[n].grad is None
        for a, b in model.store.frozen_ranges():
            assert not bool(model.store.grad[a:b].view(torch.int32).any())
        for n in train:
            gn = 2. * float(g['grad_norms'][n])
            e_norm = abs(float(named[n].grad.double().norm()) - gn) / gn
            e = rel(named[n].grad.float().reshape(-1)[:g['grad_head'][n].numel()], 2. * g['grad_head'][n])
            print(f'  {n}: two accumulated micro-batches against 2 x golden: norm {e_norm:.3e}, head {e:.3e}')
            assert e_norm <= GRAD_TOL and e <= GRAD_HEAD_TOL
    finally:
        F.unfreeze(model)


@pytest.mark.parametrize('set_name', ['top_half', 'v_only'])
def test_overlapped_exchange_keeps_its_groups_with_a_frozen_set_rccl_world1(set_name):
    """the method of tests/test_model_gpu.py::test_overlapped_gradient_exchange_equals_plain_step_rccl_world1 with a frozen set: the list of the set is cut
    at the same layer groups (a group below the stop goes out as zeros), every element is reduced once, loss, gradients and the stepped parameters equal
    the plain path's (fp32 atomic ordering noise only: that test's 2e-3 / 1e-5), frozen parameters do not move"""
    import torch.distributed as dist
    from oracle.cases import build_case
    from transfusion_pytorch_amd.optim import FusedAdam
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29543')
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        cfg, sd, batch, times, noise = build_case('small2')
        res = []
        for overlap in (False, True):
            model = _build(cfg, sd)
            model._noise_override = {t: v.cuda() for t, v in noise.items()}
            frozen, train = F.freeze(model, set_name)
            opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
            opt.always_sync = True
            if overlap:
                opt.overlap_grad_sync(groups=3)
            before = model.store.flat.clone()
            loss = model(batch, times=times)
            loss.backward()
            plan = model._live[0]
            assert plan._frozen == frozenset(frozen) and bool(plan.bwd_cuts) == overlap and (not overlap or len(plan.bwd_cuts) == 2)
            grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}
            assert set(grads) == set(train)
            opt.step(); sync()
            fm = _mask(model.store)
            assert torch.equal(model.store.flat[fm], before[fm]) and not torch.equal(model.store.flat[~fm], before[~fm])
            res.append((float(loss), grads, model.store.flat.clone()))
        (l0, g0, p0), (l1, g1, p1) = res
        assert abs(l0 - l1) <= 1e-6 * max(1., abs(l0))
        for k in g0:
            assert rel(g1[k], g0[k]) <= 2e-3, k
        assert rel(p1, p0) <= 1e-5
    finally:
        if own:
            dist.destroy_process_group()


def test_velocity_consistency_with_a_frozen_ema_teacher_is_unchanged():
    from oracle import cases as OC, detdata as D
    cfg, sd, x, times, noise, ty = OC.build_modality_case('flow1')
    g = _golden('flow1')
    model, _ = _case('flow1')
    F.unfreeze(model)
    teacher = _build(cfg, D.det_state_dict(cfg.state_dict_shapes(), tag='flow1/teacher')).eval()
    teacher.requires_grad_(False)
    for p in model.parameters():
        p.grad = None
    vloss, (vflow, vvel, _) = model.forward_modality(x, times=times, modality_type=ty, velocity_consistency_ema_model=teacher,
                                                     velocity_consistency_delta_time=g['vc_delta'], return_loss_breakdown=True)
    vloss.backward(); sync()
    for a, r in ((vloss.detach(), g['vc_loss']), (vflow, g['vc_flow']), (vvel, g['vc_velocity'])):
        assert abs(float(a) - float(r)) <= 3e-3 * max(1., abs(float(r)))                       # (tests/test_model_gpu.py's bound for this path)
    assert all(p.grad is None for p in teacher.parameters()) and all(p.grad is not None for p in model.store.params.values())
