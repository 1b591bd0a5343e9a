"""Text loss terms on the GPU (Transfusion.set_text_loss_terms_, engine.Plan `text_terms`): the kernels tfx_ce_reg_fwd / tfx_ce_reg_bwd / tfx_ce_reg_fwd_bwd per
element against float64 (cases, restatement and bounds: tests/_text_loss_terms_cases.py), the training step against the live oracle with the two terms added in
PyTorch, chunked against unchunked steps, "off means off", and one step each under the plan features the launches have to pass through.

The step-against-step comparisons use the figures of tests/test_text_head_gpu.py: GAP / GAP_TEXT for a chunked step against the plain one (the terms change what a
row contributes, not which launches differ between the two steps), GRAD_EQ per parameter for the same launches under another order of the fp32 atomics."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case                                    # noqa: E402

import _text_loss_terms_cases as C                                     # noqa: E402
import test_model_gpu as TM                                            # noqa: E402  (build_native, rel and the tolerances)
import test_text_head_gpu as TH                                        # noqa: E402  (_fixture_step, _snap, _assert_gap, _fingerprint, _clear and the gaps)
from _gemm_cases import BF, GUARD, assert_elementwise, assert_untouched, guarded          # noqa: E402

DEV = 'cuda'
TERMS = (1e-2, 0.1)          # the model tests' setting: both terms, z large enough to be seen through bf16 (tests/_text_loss_terms_cases.py)
GAP, GAP_TEXT, GRAD_EQ = TH.GAP, TH.GAP_TEXT, TH.GRAD_EQ
rel, sync, _stream = TM.rel, TH.sync, TH._stream
BOTH = [(c, s) for c in C.CASES for s in C.SETTINGS]
FUSED_BOTH = [(c, s) for c in C.FUSED_CASES for s in C.SETTINGS]
both_id = lambda v: C.case_id(v) if len(v) == 3 else C.setting_id(v)


# ================================================================================================ 1. the kernels
@functools.lru_cache(maxsize=None)
def _kcase(case):
    T, V, ld = case
    return C.inputs(T, V, ld, DEV)


@functools.lru_cache(maxsize=None)
def _kref(case, setting, scale=1.0):
    lg, lab = _kcase(case)
    return C.reg_ref(lg, lab, case[1], *setting, scale)


def _args(case, setting, lg, lab, lse, acc, aux, dl=None, grad_scale=1.0, scale_dev=None):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    return capi.make_args('tfx_ce_reg_chunk_args', T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse, acc=acc, grad_scale=grad_scale, scale_dev=scale_dev,
                          dlogits=dl, ld_d=ld, z_weight=setting[0], smoothing=setting[1], aux=aux)


def _fresh_sums():
    """acc and aux with what they hold before a launch (the kernels add), each with two floats behind it that no kernel may touch"""
    acc = torch.tensor(C.ACC_INIT + (9.0, 9.0), device=DEV, dtype=torch.float32)
    aux = torch.tensor(C.AUX_INIT + (7.0, 7.0), device=DEV, dtype=torch.float32)
    return acc, aux


def _run_fwd(case, setting, lg, lab):
    from transfusion_pytorch_amd import capi
    buf, lse = guarded(case[0], 1, torch.float32, DEV, 0)
    acc, aux = _fresh_sums()
    capi.call('tfx_ce_reg_fwd', _args(case, setting, lg, lab, lse, acc, aux), _stream())
    sync()
    return buf, lse, acc, aux


def _check_sums(what, acc, aux, r, tols):
    """acc[0], aux[0], aux[1] against float64 under their bounds, the count exact, the floats behind them untouched; returns the three error / bound ratios"""
    _, tol_loss, tol_ce, tol_sq, _ = tols
    got = (float(acc[0].double()), float(aux[0].double()), float(aux[1].double()))
    want = (C.ACC_INIT[0] + float(r.loss), C.AUX_INIT[0] + float(r.ce_sum), C.AUX_INIT[1] + float(r.sq_sum))
    ratios = [abs(g - w) / float(t) for g, w, t in zip(got, want, (tol_loss, tol_ce, tol_sq))]
    print(f'  {what}: acc[0] {got[0]:.6f} aux[0] {got[1]:.6f} aux[1] {got[2]:.6f}; error / bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}; count {float(acc[1])}')
    assert max(ratios) <= 1, (what, got, want, ratios)
    assert float(acc[1]) == C.ACC_INIT[1] + float(r.count) and acc[2:].tolist() == [9.0, 9.0] and aux[2:].tolist() == [7.0, 7.0]
    return ratios


@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_reg_fwd_lse_and_sums_against_float64(case, setting):
    T, V, ld = case
    lg, lab = _kcase(case)
    r = _kref(case, setting)
    tols = C.reg_bounds(r)
    keep = lg.clone()
    buf0, _ = guarded(T, 1, torch.float32, DEV, 0)
    buf, lse, acc, aux = _run_fwd(case, setting, lg, lab)
    worst = assert_elementwise(f'tfx_ce_reg_fwd {case} lse', lse.double(), r.lse[:, None], tols[0][:, None], tile=(4, 1))
    assert bool((lse[~r.valid] == 0).all()), 'ignored rows get lse 0'
    assert_untouched(f'tfx_ce_reg_fwd {case} lse', buf, buf0, TH._written(buf, T))
    print(f'  {C.case_id(case)} {C.setting_id(setting)}: lse worst error / bound {worst:.3f}')
    _check_sums(f'tfx_ce_reg_fwd {C.case_id(case)} {C.setting_id(setting)}', acc, aux, r, tols)
    assert torch.equal(lg.view(torch.int32), keep.view(torch.int32)), 'the forward writes lse, acc and aux only'


@pytest.mark.parametrize('scale_dev', [None, 0.37], ids=['no_scale_dev', 'scale_dev_0.37'])
@pytest.mark.parametrize('case,setting', BOTH, ids=both_id)
def test_reg_bwd_dlogits_per_element_against_float64(case, setting, scale_dev):
    """the product's chain: tfx_ce_reg_fwd's own lse feeds tfx_ce_reg_bwd; every element of d logits against the float64 gradient"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg, lab = _kcase(case)
    gs = 0.0031
    sd = None if scale_dev is None else torch.tensor([scale_dev, 55.0], device=DEV, dtype=torch.float32)
    scale = float(torch.tensor(gs, dtype=torch.float32).double()) * (1.0 if sd is None else float(sd[0].double()))
    r = _kref(case, setting, scale)
    tol_d = C.reg_bounds(r, scale)[4]
    _, lse, acc, aux = _run_fwd(case, setting, lg, lab)
    acc0, aux0, lse0 = acc.clone(), aux.clone(), lse.clone()
    buf, dl = guarded(T, ld, BF, DEV, 0)
    before = buf.clone()
    capi.call('tfx_ce_reg_bwd', _args(case, setting, lg, lab, lse, None, None, dl, grad_scale=gs, scale_dev=sd), _stream())      # (the backward takes no acc / aux)
    sync()
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tol_d
    worst = assert_elementwise(f'tfx_ce_reg_bwd {case} {setting} dlogits', dl.double(), ref, tol, tile=(4, 512))
    assert not bool(dl[:, V:].view(torch.int16).any()) and not bool(dl[~r.valid].view(torch.int16).any()), 'pad columns and ignored rows: zero bits'
    assert_untouched(f'tfx_ce_reg_bwd {case} dlogits', buf, before, TH._written(buf, T))
    assert torch.equal(acc, acc0) and torch.equal(aux, aux0) and torch.equal(lse, lse0), 'the backward writes d logits only'
    print(f'  {C.case_id(case)} {C.setting_id(setting)} scale_dev {scale_dev}: d logits worst error / bound {worst:.3f}')


@pytest.mark.parametrize('case,setting', FUSED_BOTH, ids=both_id)
def test_reg_fused_kernel_against_float64(case, setting):
    """tfx_ce_reg_fwd_bwd at the widths of both its paths (448: rows in registers, 1024: strided passes): d logits per element, the four sums, guards"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg, lab = _kcase(case)
    lg = torch.where(torch.isnan(lg), torch.zeros_like(lg), lg)             # (the fused kernel's fast path loads an ignored row's logits)
    gs = 0.0031
    scale = float(torch.tensor(gs, dtype=torch.float32).double())
    r = C.reg_ref(lg, lab, V, *setting, scale)
    tols = C.reg_bounds(r, scale)
    ref = torch.zeros(T, ld, dtype=torch.float64, device=DEV); ref[:, :V] = r.d
    tol = torch.zeros(T, ld, dtype=torch.float64, device=DEV); tol[:, :V] = tols[4]
    buf, dl = guarded(T, ld, BF, DEV, 0)
    before = buf.clone()
    acc, aux = _fresh_sums()
    capi.call('tfx_ce_reg_fwd_bwd', capi.make_args('tfx_ce_reg_args', T=T, V=V, logits=lg, ld=ld, labels=lab, grad_scale=gs, dlogits=dl, ld_d=ld, acc=acc,
                                                   z_weight=setting[0], smoothing=setting[1], aux=aux), _stream())
    sync()
    worst = assert_elementwise(f'tfx_ce_reg_fwd_bwd {case} {setting}', dl.double(), ref, tol, tile=(4, 512))
    assert not bool(dl[:, V:].view(torch.int16).any()) and not bool(dl[~r.valid].view(torch.int16).any()), 'pad columns and ignored rows: zero bits'
    assert_untouched(f'tfx_ce_reg_fwd_bwd {case} dlogits', buf, before, TH._written(buf, T))
    print(f'  {C.case_id(case)} {C.setting_id(setting)}: fused d logits worst error / bound {worst:.3f}')
    _check_sums(f'tfx_ce_reg_fwd_bwd {C.case_id(case)} {C.setting_id(setting)}', acc, aux, r, tols)


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_all_ignored_launch_leaves_acc_and_aux_untouched(case):
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    setting = C.SETTINGS[2]
    lg = torch.full((T, ld), float('nan'), device=DEV)
    lab = torch.full((T,), -1, device=DEV, dtype=torch.int32)
    _, lse, acc, aux = _run_fwd(case, setting, lg, lab)
    assert acc.tolist() == list(C.ACC_INIT) + [9.0, 9.0] and aux.tolist() == list(C.AUX_INIT) + [7.0, 7.0] and not bool(lse.view(torch.int32).any())
    buf, dl = guarded(T, ld, BF, DEV, 0)
    before = buf.clone()
    capi.call('tfx_ce_reg_bwd', _args(case, setting, lg, lab, lse, None, None, dl), _stream())
    sync()
    assert not bool(dl.view(torch.int16).any())
    assert_untouched(f'tfx_ce_reg_bwd {case} all ignored', buf, before, TH._written(buf, T))
    if case in C.FUSED_CASES:
        lg0 = torch.zeros(T, ld, device=DEV)
        acc, aux = _fresh_sums()
        buf, dl = guarded(T, ld, BF, DEV, 0)
        before = buf.clone()
        capi.call('tfx_ce_reg_fwd_bwd', capi.make_args('tfx_ce_reg_args', T=T, V=V, logits=lg0, ld=ld, labels=lab, grad_scale=1.0, dlogits=dl, ld_d=ld, acc=acc,
                                                       z_weight=setting[0], smoothing=setting[1], aux=aux), _stream())
        sync()
        assert acc.tolist() == list(C.ACC_INIT) + [9.0, 9.0] and aux.tolist() == list(C.AUX_INIT) + [7.0, 7.0] and not bool(dl.view(torch.int16).any())
        assert_untouched(f'tfx_ce_reg_fwd_bwd {case} all ignored', buf, before, TH._written(buf, T))


@pytest.mark.parametrize('case', C.CASES, ids=C.case_id)
def test_zero_weights_return_the_plain_kernels_bits(case):
    """z = e = 0: lse and d logits of the new entry points equal the old entry points' to the bit, acc too where one block sums the rows in one order
    (elsewhere within a rounding of the atomics' order), and aux[0] is then the same sum as acc[0]"""
    from transfusion_pytorch_amd import capi
    T, V, ld = case
    lg, lab = _kcase(case)
    gs, off = 0.0031, (0.0, 0.0)
    sd = torch.tensor([0.37], device=DEV, dtype=torch.float32)
    _, lse, acc, aux = _run_fwd(case, off, lg, lab)
    _, dl = guarded(T, ld, BF, DEV, 0)
    capi.call('tfx_ce_reg_bwd', _args(case, off, lg, lab, lse, None, None, dl, grad_scale=gs, scale_dev=sd), _stream())
    _, lse_p = guarded(T, 1, torch.float32, DEV, 0)
    _, dl_p = guarded(T, ld, BF, DEV, 0)
    acc_p = torch.tensor(C.ACC_INIT, device=DEV, dtype=torch.float32)
    plain = capi.make_args('tfx_ce_chunk_args', T=T, V=V, logits=lg, ld=ld, labels=lab, lse=lse_p, acc=acc_p, grad_scale=gs, scale_dev=sd, dlogits=dl_p, ld_d=ld)
    capi.call('tfx_ce_fwd', plain, _stream())
    capi.call('tfx_ce_bwd', plain, _stream())
    sync()
    assert torch.equal(lse.view(torch.int32), lse_p.view(torch.int32)) and torch.equal(dl.view(torch.int16), dl_p.view(torch.int16))
    r = C.ce_ref(lg, lab, V)
    tol = float(C.bounds(r, V)[1])
    assert abs(float(acc[0]) - float(acc_p[0])) <= 2 * tol and float(acc[1]) == float(acc_p[1])
    assert abs((float(aux[0]) - C.AUX_INIT[0]) - (float(acc[0]) - C.ACC_INIT[0])) <= 2 * tol
    if case in C.FUSED_CASES:
        lg0 = torch.where(torch.isnan(lg), torch.zeros_like(lg), lg)
        outs = []
        for fn, st, extra in (('tfx_ce_fwd_bwd', 'tfx_ce_args', {}), ('tfx_ce_reg_fwd_bwd', 'tfx_ce_reg_args', dict(z_weight=0., smoothing=0., aux=aux))):
            _, d = guarded(T, ld, BF, DEV, 0)
            a = torch.tensor(C.ACC_INIT, device=DEV, dtype=torch.float32)
            capi.call(fn, capi.make_args(st, T=T, V=V, logits=lg0, ld=ld, labels=lab, grad_scale=gs, dlogits=d, ld_d=ld, acc=a, **extra), _stream())
            outs.append(d)
        sync()
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ================================================================================================ 2. the model against the live oracle
def _reg_torch(logits, labels, z, e):
    """mean over the valid rows of F.cross_entropy(label_smoothing=e) + z logsumexp^2: the terms in PyTorch, at the fp32 weights the kernels receive"""
    z, e = C.f32(z), C.f32(e)
    valid = labels != -1
    lse = torch.logsumexp(logits, dim=-1)
    return torch.nn.functional.cross_entropy(logits, labels, ignore_index=-1, label_smoothing=e) + z * (lse[valid] ** 2).mean()


def _compare_with_oracle(model, loss, ref_loss, sdg):
    lo, lr = float(loss.detach()), float(ref_loss.detach())
    assert abs(lo - lr) <= 2e-3 * max(1., abs(lr)), (lo, lr)
    wsum = nsum = 0.
    for k, p in model.named_parameters():
        gr = sdg[k].grad if sdg[k].requires_grad else None
        if gr is None or float(gr.norm()) < 1e-7:
            continue
        e = rel(p.grad, gr)
        assert e <= TM.GRAD_HEAD_TOL, (k, e)
        wsum += e * float(gr.norm()); nsum += float(gr.norm())
    print(f'  loss native {lo:.6f} oracle {lr:.6f}; gradients: norm-weighted mean rel err {wsum / nsum:.3e}')
    assert wsum / nsum <= TM.GRAD_MEAN_TOL


def _oracle_setup(vocab):
    from oracle import detdata as D
    from oracle.cases import with_grad
    from oracle.transfusion_oracle import OracleConfig
    cfg = OracleConfig(num_text_tokens=vocab, dim=128, depth=2, dim_latents=(16,), heads=2, dim_head=64)
    sd = D.det_state_dict(cfg.state_dict_shapes(), tag=f'textreg{vocab}')
    return D, cfg, sd, with_grad(sd)


WIDTHS = [(256, None), (5000, 128)]          # a narrow vocabulary unchunked (the fused kernel's register path) | the wide kernels on ragged chunks
width_id = lambda v: f'vocab{v[0]}_rows{v[1]}'


@pytest.mark.parametrize('width', WIDTHS, ids=width_id)
def test_interleaved_step_matches_live_oracle_with_the_terms_added(width):
    """tests/test_text_head_gpu.py::test_wider_vocabulary_matches_live_oracle with the terms on: the oracle's loss with its text term replaced by the regularised
    one (over the WHOLE vocabulary, specials included), loss' = loss + text_loss_weight w_text (reg - text_loss), and its autograd gradients"""
    from oracle.transfusion_oracle import forward_train
    vocab, rows = width
    D, cfg, sd, sdg = _oracle_setup(vocab)
    tx = lambda key, n: D.det_randint(f'textreg/{key}', (n,), 0, vocab)
    batch = [[tx('a', 60), (0, D.det_normalish('textreg/m0', (2, 3, 16))), tx('b', 70)],
             [tx('c', 100), (0, D.det_normalish('textreg/m1', (5, 16))), tx('d', 40)],
             [tx('e', 120)]]                                                 # 3 x 192 rows: four chunks of 128 and a ragged one of 64
    times = D.det_uniform('textreg/t', (3, 1), 0.05, 0.95)
    noise = {0: D.det_normalish('textreg/n0', (11, 16))}
    ref = forward_train(sdg, cfg, batch, times, noise, return_all=True)
    lab = ref['labels'].reshape(-1)
    reg = _reg_torch(ref['logits'].reshape(lab.numel(), -1), lab, *TERMS)
    w_text = (lab != cfg.ignore_index).sum() / ref['packed'].total_tokens
    ref_loss = ref['loss'] + cfg.text_loss_weight * w_text * (reg - ref['text_loss'])
    ref_loss.backward()
    model = TH._native(cfg, sd, rows).set_text_loss_terms_(*TERMS)
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss, bd = model(batch, times=times, return_breakdown=True)
    loss.backward()
    sync()
    plan = model._live[0]
    assert plan.reg == TERMS
    assert plan.chunk == rows and (plan.md.vp > C.WIDE_LD) == (vocab == 5000) and (rows is None or plan.T % rows)
    assert abs(float(bd.text) - float(reg.detach())) <= 2e-3 * max(1., abs(float(reg.detach())))
    assert abs(float(reg.detach()) - float(ref['text_loss'].detach())) > 0.05, 'the terms are visible in the loss'
    _compare_with_oracle(model, loss, ref_loss, sdg)


@pytest.mark.parametrize('width', WIDTHS, ids=width_id)
def test_forward_text_matches_live_oracle_with_the_terms_added(width):
    """forward_text smooths over the text tokens only (it narrows V to num_text_tokens): the oracle's forward_text with the same prefix of the logits"""
    from oracle.transfusion_oracle import forward_text
    vocab, rows = width
    D, cfg, sd, sdg = _oracle_setup(vocab)
    text = D.det_randint('textreg/text', (3, 98), 0, vocab)
    text[0, 90:] = -1; text[2, 70:] = -1                                     # padded tails: ignored labels
    ref = forward_text(sdg, cfg, text, return_all=True)
    lab = text[:, 1:].reshape(-1)
    ref_loss = _reg_torch(ref['logits'][..., :cfg.num_text_tokens].reshape(lab.numel(), -1), lab, *TERMS)
    ref_loss.backward()
    model = TH._native(cfg, sd, rows and 64).set_text_loss_terms_(*TERMS)
    loss = model.forward_text(text)
    loss.backward()
    sync()
    plan = model._live[0]
    assert plan.reg is not None and plan.chunk == (rows and 64) and (rows is None or plan.T % 64)
    assert abs(float(ref_loss.detach()) - float(ref['loss'].detach())) > 0.05, 'the terms are visible in the loss'
    _compare_with_oracle(model, loss, ref_loss, sdg)
    t = model.text_loss_terms()
    assert abs(float(t.text) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    assert abs(float(t.ce) - float(ref['loss'].detach())) <= 2e-3 * max(1., abs(float(ref['loss'].detach())))


# ================================================================================================ 3. chunked against unchunked, the terms' read-out
def _make(name, rows=None, terms=TERMS):
    make, step, g = TH._fixture_step(name)
    m = make(rows)
    if terms is not None:
        m.set_text_loss_terms_(*terms)
    return m, step


@functools.lru_cache(maxsize=None)
def _terms_on(name):
    """the plain (unchunked) step of a fixture with the terms on: (snapshot, breakdown.text or None, text_loss_terms() as floats)"""
    m, step = _make(name)
    loss, bd = step(m)
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.reg is not None and plan.chunk is None
    t = m.text_loss_terms()
    assert float(t.text) == float(plan.acc[0] / plan.acc[1]) and float(t.ce) == float(plan.aux[0] / plan.acc[1]) and float(t.lse_sq) == float(plan.aux[1] / plan.acc[1])
    return s, (float(bd.text) if bd is not None else None), tuple(float(v) for v in t)


@pytest.mark.parametrize('name,rows', [('text1', 64), ('small2', 64), ('small2', 'ragged'), ('head8', 64)])
def test_chunked_and_unchunked_steps_with_terms_agree(name, rows):
    on, text_on, (t_text, t_ce, t_sq) = _terms_on(name)
    m0, step0 = _make(name, terms=None)
    l0, bd0 = step0(m0); sync()
    assert m0.text_loss_terms() is None and m0._live[0].reg is None
    off, T = dict(loss=float(l0.detach())), m0._live[0].T
    ce_off = float(bd0.text) if bd0 is not None else float(l0.detach())
    assert abs(t_ce - ce_off) <= 2e-3 * max(1., abs(ce_off)), 'ce is the plain mean cross entropy'
    if text_on is not None:
        assert t_text == text_on, 'text is LossBreakdown.text'
    z, e = C.f32(TERMS[0]), C.f32(TERMS[1])
    assert t_text > t_ce and t_sq > 0 and t_text - (1 - e) * t_ce - z * t_sq > 0, 'both terms are in the regularised mean'
    assert abs(on['loss'] - off['loss']) > 1e-3 * abs(off['loss']), 'the step with the terms is another step'
    if rows == 'ragged':
        rows = TH._ragged_rows(T)
    m, step = _make(name, rows)
    loss, bd = step(m)
    s = TH._snap(m, loss)
    plan = m._live[0]
    assert plan.chunk == rows and plan.reg is not None and len(plan._chunks()) >= 2
    TH._assert_gap(s, on, f'{name} rows {rows}, terms {TERMS}', GAP_TEXT if name == 'text1' else GAP)
    t = m.text_loss_terms()
    assert float(t.text) == float(plan.acc[0] / plan.acc[1])
    assert abs(float(t.ce) - t_ce) <= 1e-5 * abs(t_ce) and abs(float(t.lse_sq) - t_sq) <= 1e-5 * t_sq


# ================================================================================================ 4. off means off
@pytest.mark.parametrize('how', ['cleared', 'zeros'])
def test_terms_set_and_cleared_leave_every_list_as_it_was(how):
    """fingerprints hash buffer addresses, so they are compared on ONE model: its lists before the terms were ever set, and after they were set and cleared"""
    make, step, _ = TH._fixture_step('small2')
    m = make(None)
    l0, _ = step(m); sync()
    F = m._live[0]
    lists = ('fwd', 'bwd', 'vel', 'rec', 'clean_bwd')
    fp0 = tuple(TH._fingerprint(getattr(F, k)) for k in lists)
    assert F.reg is None and F.aux is None and m.text_loss_terms() is None
    m.set_text_loss_terms_(*TERMS)
    TH._clear(m); l1, _ = step(m); sync()
    Q = m._live[0]
    assert Q is not F and Q.reg == TERMS and m.text_loss_terms() is not None and float(l1.detach()) != float(l0.detach())
    m.set_text_loss_terms_(0., 0.) if how == 'zeros' else m.set_text_loss_terms_()
    assert m.text_loss_terms() is None
    TH._clear(m); l2, _ = step(m); sync()
    assert m._live[0] is F and tuple(TH._fingerprint(getattr(F, k)) for k in lists) == fp0
    assert m.text_loss_terms() is None and abs(float(l2.detach()) - float(l0.detach())) <= 1e-6 * abs(float(l0.detach()))


# ================================================================================================ 5. one step each under the plan features
def _per_param_worst(a, b, skip=()):
    assert set(a) == set(b)
    return max((rel(a[k], b[k]), k) for k in b if k not in skip and float(b[k].norm()) > 1e-7)


def test_with_activation_checkpointing():
    on, _, _ = _terms_on('small2')
    m, step = _make('small2')
    m.set_activation_checkpointing_(True)
    loss, _ = step(m)
    plan = m._live[0]
    assert plan.ckpt and plan.reg is not None and plan._recompute
    TH._assert_gap(TH._snap(m, loss), on, 'checkpointing + terms')


def test_frozen_text_head_keeps_the_trunk_gradient():
    on, _, _ = _terms_on('small2')
    m, step = _make('small2')
    m.store.params['to_text_logits.weight'].requires_grad_(False)
    loss, _ = step(m)
    s = TH._snap(m, loss)
    plan = m._live[0]
    head = m.store.grad_ptr('to_text_logits.weight')
    assert plan.reg is not None and m.store.params['to_text_logits.weight'].grad is None and not bool(m.store.grad_view('to_text_logits.weight').view(torch.int32).any())
    assert not any((fn if isinstance(fn, str) else fn.__name__) == 'tfx_gemm_tn' and a.C == head for fn, a in plan.bwd if isinstance(fn, str)), 'no head product'
    assert abs(s['loss'] - on['loss']) <= 1e-6 * abs(on['loss'])
    grads_on = {k: v for k, v in on['grads'].items() if k != 'to_text_logits.weight'}
    worst = _per_param_worst(s['grads'], grads_on)
    print(f'  trunk gradients, head frozen against unfrozen: worst {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= GRAD_EQ


def test_two_accumulated_backward_passes_then_fused_adam():
    from transfusion_pytorch_amd.optim import FusedAdam
    on, _, _ = _terms_on('small2')
    _, _, batch, times, _ = build_case('small2')
    m, _ = _make('small2')
    opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
    before = m.store.flat.clone()
    with opt.no_sync():
        m(batch, times=times).backward()
    m(batch, times=times).backward()
    sync()
    g = m.store.grad.clone()
    opt.step(); sync()
    assert m._live[0].reg is not None
    print(f'  accumulated gradient against twice the single step: {rel(g, 2. * on["flat"]):.3e}')
    assert rel(g, 2. * on['flat']) <= GRAD_EQ
    assert bool(torch.isfinite(m.store.flat).all()) and not torch.equal(m.store.flat, before)


def test_half_loss_backward_halves_every_gradient():
    on, _, _ = _terms_on('small2')
    _, _, batch, times, _ = build_case('small2')
    for rows in (None, 64):
        m, _ = _make('small2', rows)
        (0.5 * m(batch, times=times)).backward()
        sync()
        g = {k: 2. * v for k, v in TH._grads(m).items()}
        worst = _per_param_worst(g, on['grads'])
        print(f'  rows {rows}: 2 x gradients of (0.5 loss) against those of loss: worst {worst[0]:.3e} ({worst[1]})')
        assert worst[0] <= GRAD_EQ


@pytest.mark.parametrize('rows', [None, 64], ids=['whole_head', 'rows64'])
def test_training_graph_replay(rows, monkeypatch):
    """TFX_TRAIN_GRAPH: from the third identical step both lists replay as graphs - the `_reg` launches and the memset of acc | aux are ordinary captured items -
    and every step equals the list-replayed step with the terms on"""
    from transfusion_pytorch_amd import engine
    on, _, _ = _terms_on('small2')
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    m, step = _make('small2', rows)
    for k in range(5):
        TH._clear(m)
        loss, _ = step(m); sync()
        plan = m._live[0]
        if k >= 2:
            st_f, st_b = plan.fwd._auto[(0, len(plan.fwd))], plan.bwd._auto[(0, len(plan.bwd))]
            assert st_f[1] and st_b[1], 'from the third identical step both lists replay as graphs'
        TH._assert_gap(TH._snap(m, loss), on, f'TFX_TRAIN_GRAPH step {k}, rows {rows}')
        t = m.text_loss_terms()
        assert float(t.text) == float(plan.acc[0] / plan.acc[1]) and abs(float(t.ce) - _terms_on('small2')[2][1]) <= 1e-5
    assert plan.reg is not None and plan.chunk == rows


def test_toy_example_trains_with_the_flags_on():
    """examples/toy_text_latent.py --z-loss 1e-4 --label-smoothing 0.1: the loop runs with the terms on, logs their parts and the loss stays finite"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import toy_text_latent as train_toy
    lines = []
    losses = train_toy.main(steps=40, sample_every=1000, log=lines.append, z_loss=1e-4, label_smoothing=0.1)
    assert len(losses) == 40 and all(l == l and abs(l) < float('inf') for l in losses)
    assert len(lines) == 2 and all('ce ' in l and 'lse^2' in l for l in lines)


def test_hidden_taps():
    """a loss on hidden taps next to the regularised text loss (tests/test_text_head_gpu.py::test_hidden_taps with the terms on): chunked against unchunked"""
    import os
    import _self_flow_cases as SF
    g = torch.load(os.path.join(TM.GOLDEN, f'{SF.TAPS_FIXTURE}.pt'), weights_only=False)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    taps = list(SF.tap_indices(cfg.depth))
    res = []
    for rows in (None, 64):
        m = TH._native(cfg, sd, rows).set_text_loss_terms_(*TERMS)
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        loss, hiddens = m(batch, times=times, return_hiddens=True)
        total = loss
        for k in taps:
            total = total + g['taps'][k]['w'] * hiddens[k].pow(2).mean()
        total.backward()
        res.append(TH._snap(m, loss))
        assert m._live[0].chunk == rows and m._live[0].reg == TERMS
    TH._assert_gap(res[1], res[0], f'hidden taps {taps}, terms {TERMS}')
