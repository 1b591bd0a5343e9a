"""Model-level tests of the plans outside the region every other model test sits in (dim <= 1024, depth <= 24): the PUSH form of the AttentionResidual
backward (engine.Plan.pull False: one tfx_attnres_bwd sweep per layer with its `first` flag, the U-Net skip share as `g2`, tfx_adaln_post_bwd as its own
launch, dx0 = g + dH[0] (+ dskip[0]) from tfx_add_bf16), the single-stream list of deep or wide plans, and the deepest pull plans (depth 30: the last one
with a side stream; depth 32: the last pull plan).

A. the natural region - tests/_wide_deep_cases.py - against the live CPU oracle, by the rule and the constants of
   tests/test_model_gpu.py::test_odd_configurations_match_live_oracle
B. the push form forced on the reference goldens (engine.pull_form_ok patched to refuse): the goldens come from the unmodified reference, so they
   judge the push list exactly as they judge the pull list - everything tests/test_model_gpu.py::test_training_step_matches_reference_golden asserts
C. activation checkpointing, frozen sets, LoRA, accumulation, graph replay and the overlapped exchange on push plans, each by the criterion its own
   test file holds pull plans to

Every test first asserts the form it claims to run (Plan.pull, Plan.side, the launch counts of the backward list) and prints it as a `PUSHFORM` line;
parts A and B print their figures the same way: profiles/push_form_parity.txt keeps a copy."""
import contextlib
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _frozen_cases as F                                          # noqa: E402
import _wide_deep_cases as WD                                      # noqa: E402
import test_checkpointing_gpu as CK                                # noqa: E402  (_fixture, _native, _grads, _same_step, LOSS_EQ, GRAD_EQ)
import test_frozen_gpu as FZ                                       # noqa: E402  (_ops, _grad_errors, _mean, _golden, MARGIN)
import test_lora_gpu as TL                                         # noqa: E402
import test_model_gpu as TM                                        # noqa: E402  (run_native, check_step_against_golden, rel and the tolerances)

rel, sync = TM.rel, CK.sync
PUSH_OPS = ('tfx_attnres_bwd', 'tfx_adaln_post_bwd')
PULL_OPS = ('tfx_attnres_pull_bwd', 'tfx_attnres_prep', 'tfx_attnres_finish')


@contextlib.contextmanager
def form(monkeypatch, push):
    """push=True: the forced push - engine.pull_form_ok refuses every model for as long as the block runs (a plan reads it when it is built, at the
    model's first step); push=False: the function as it is"""
    from transfusion_pytorch_amd import engine
    with monkeypatch.context() as m:
        if push:
            m.setattr(engine, 'pull_form_ok', lambda md: False)
        yield


def assert_form(plan, what, push, side):
    """the plan runs the form the test claims: Plan.pull / Plan.side and what its CURRENT backward list launches"""
    D, ops = plan.md.depth, FZ._ops(plan.bwd)
    n = {k: ops.count(k) for k in PUSH_OPS + PULL_OPS}
    print(f'PUSHFORM form {what}: pull {plan.pull} side {plan.side} depth {D} dim {plan.md.dim} launches ' + ' '.join(f'{k[4:]}={v}' for k, v in n.items()))
    assert plan.pull is (not push) and plan.side is side, (what, plan.pull, plan.side)
    if push:
        assert [n[k] for k in PUSH_OPS] == [D, D] and not any(n[k] for k in PULL_OPS), (what, n)
        assert ops.count('tfx_add_bf16') == 2                       # dx0 = g + dH[0], + dskip[0]: every model of depth >= 2 pops x_0's skip
    else:
        assert not any(n[k] for k in PUSH_OPS) and n['tfx_attnres_pull_bwd'] >= D + 1 and n['tfx_attnres_prep'] == 1 and n['tfx_attnres_finish'] == 1, (what, n)
    return n


def _inputs(name):
    """(cfg, state dict, batch, times, noise, transformer switches) of a wide / deep case or of a fixture of tests/test_checkpointing_gpu.py"""
    return (*WD.build(name), {}) if name in WD.CASES else CK._fixture(name)


def _model(name, ckpt=False):
    cfg, sd, batch, times, noise, sw = _inputs(name)
    m = CK._native(cfg, sd, ckpt, **sw)
    m._noise_override = {t: v.cuda() for t, v in noise.items()}
    return m, batch, times


def _step(model, batch, times):
    """one step from empty gradients -> (loss, {name: gradient})"""
    for p in model.parameters():
        p.grad = None
    loss = model(batch, times=times)
    loss.backward()
    sync()
    return float(loss.detach()), CK._grads(model)


def _expected(name):
    """(forced, side) of a test's model: the wide / deep cases run their natural form, everything else the forced push on a side-stream plan"""
    return (False, WD.CASES[name].side) if name in WD.CASES else (True, True)


# ================================================================================================ A. the natural region against the live oracle
# The norm-weighted mean gradient error grows with depth whatever the form: measured 1.197e-2 at `d30` and 1.226e-2 at `d32` - PULL plans, code no older
# test reaches at that depth (the goldens stop at depth 24) - against GRAD_MEAN_TOL = 1.2e-2; the push cases sit beside them (d33 1.297e-2, d34 1.189e-2,
# d33h32 1.217e-2).  So depth is the cause, not the form, and the depth 30 - 34 cases are held to d32's figure times what the push form may cost on top:
# the largest push / pull ratio of the same quantity on the four reference goldens, where the reference judges both forms (part B: tiny1 1.014,
# small2 1.021, mid2 1.015, head8 0.999), rounded up to the next 0.5.  (Push adds into dH in bf16 once per layer, pull forms each hidden's gradient once:
# that ratio is what the difference costs.)  Every other bound of the deep cases, and every bound of the two wide ones, is the constant.
# A wiring mistake - a dropped skip share, a wrong `first`, a missing dskip[0] - moves the lower layers' gradients by O(1) relative.
D32_GRAD_MEAN, PUSH_OVER_PULL = 1.226e-2, 1.5
DEEP_GRAD_MEAN_TOL = D32_GRAD_MEAN * PUSH_OVER_PULL               # 1.839e-2


@pytest.mark.parametrize('name', list(WD.CASES))
def test_natural_region_matches_live_oracle(name):
    """Bounds: the constants tests/test_model_gpu.py applies to live-oracle configurations - loss 2e-3 max(1, |ref|), LOGIT_TOL, GRAD_HEAD_TOL per
    parameter, GRAD_MEAN_TOL norm-weighted - with one exception, DEEP_GRAD_MEAN_TOL for the depth 30 - 34 cases (above; profiles/push_form_parity.txt)"""
    c = WD.CASES[name]
    cfg, sd, batch, times, noise = WD.build(name)
    ref = WD.oracle_step(name)
    model = TM.build_native(cfg, sd).train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss = model(batch, times=times)
    loss.backward()
    sync()
    plan = model._live[0]
    assert_form(plan, name, push=not c.pull, side=c.side)
    loss = float(loss.detach())
    e_log = rel(plan.logits.view(plan.b, plan.n, -1)[:, :model._live_n_true, :cfg.vocab].float().cpu(), ref.logits)
    errs = {}
    for k, p in model.named_parameters():
        gr = ref.grads.get(k)
        if gr is None or float(gr.norm()) < WD.NORM_FLOOR:
            continue
        assert p.grad is not None, k
        errs[k] = (rel(p.grad, gr), float(gr.norm()))
    assert len(errs) == len(ref.grads), 'every parameter with an oracle gradient is compared (tests/test_wide_deep_cpu.py keeps them above the floor)'
    worst = max(errs, key=lambda k: errs[k][0])
    mean = FZ._mean(errs)
    print(f'PUSHFORM A {name}: loss native {loss:.6f} oracle {ref.loss:.6f} delta {loss - ref.loss:+.2e}; logits rel {e_log:.3e}; {len(errs)} gradients, '
          f'norm-weighted mean {mean:.3e}, worst {errs[worst][0]:.3e} ({worst})')
    assert abs(loss - ref.loss) <= 2e-3 * max(1., abs(ref.loss))
    assert e_log <= TM.LOGIT_TOL
    for k, (e, _) in errs.items():
        assert e <= TM.GRAD_HEAD_TOL, (k, e)
    assert mean <= (DEEP_GRAD_MEAN_TOL if c.depth >= 30 else TM.GRAD_MEAN_TOL)


# ================================================================================================ B. forced push against the reference goldens
@pytest.mark.parametrize('name', ['tiny1', 'small2', 'mid2', 'head8'])
def test_forced_push_matches_reference_golden(name, monkeypatch):
    from oracle.cases import build_case
    monkeypatch.setattr(TM, '_log_parity', lambda *a, **k: None)          # (the parity log is about the default path)
    g = torch.load(os.path.join(TM.GOLDEN, f'{name}.pt'), weights_only=False)
    figs = {}
    for push in (False, True):
        with form(monkeypatch, push):
            cfg, model, out = TM.run_native(name)
            plan = model._live[0]
            assert_form(plan, f'{name} {"forced push" if push else "pull"}', push=push, side=True)
            figs[push] = TM.check_step_against_golden(name, g, out)
            if push:
                _, _, batch, times, _ = build_case(name)
                with pytest.raises(NotImplementedError, match='pull-form'):
                    model(batch, times=times, return_hiddens=True)          # hidden taps ride in the pull launches: the push form has none
    pl, ps = figs[False], figs[True]
    print(f'PUSHFORM B {name}: gradient norm-weighted mean pull {pl["grad_mean_rel"]:.3e} push {ps["grad_mean_rel"]:.3e} ratio '
          f'{ps["grad_mean_rel"] / pl["grad_mean_rel"]:.3f}; worst pull {pl["grad_worst_rel"]:.3e} ({pl["grad_worst_name"]}) push {ps["grad_worst_rel"]:.3e} '
          f'({ps["grad_worst_name"]}) ratio {ps["grad_worst_rel"] / pl["grad_worst_rel"]:.3f}; logits rel {ps["logits_rel"]:.3e}')


# ================================================================================================ C. the features on push plans
@pytest.mark.parametrize('name', ['small2', 'odd5', 'd33'])
def test_checkpointed_step_on_a_push_plan_equals_the_plain_step(name, monkeypatch):
    """tests/test_checkpointing_gpu.py: logits, final embed and predictions bit-equal (test_forward_is_unchanged), loss and gradients by _same_step"""
    forced, side = _expected(name)
    res = []
    with form(monkeypatch, forced):
        for ckpt in (False, True):
            model, batch, times = _model(name, ckpt)
            loss, grads = _step(model, batch, times)
            plan = model._live[0]
            assert plan.ckpt == ckpt
            assert_form(plan, f'{name} {"checkpointed" if ckpt else "plain"}', push=True, side=side)
            res.append((plan, loss, grads))
    (P, lp, gp), (C, lc, gc) = res
    assert C.n_slots == (2 if side else 1) and len(C._recompute) == max(C.md.depth - C.n_slots, 0) and not P._recompute
    assert torch.equal(C.logits, P.logits) and torch.equal(C.embed, P.embed)
    for t in P.lat:
        assert torch.equal(C.lat[t]['pred'], P.lat[t]['pred']), t
    CK._same_step((lc, gc), (lp, gp), f'{name} push form, checkpointed against plain')


@functools.lru_cache(maxsize=None)
def _push_small2():
    """small2 on a forced-push plan (built, and run for the first time, inside form(push=True)), shared by the freeze sets; with nothing frozen: its
    per-parameter gradient errors against the golden and its loss"""
    model, batch, times = _model('small2')
    loss, _ = _step(model, batch, times)
    return model, batch, times, FZ._grad_errors(model, FZ._golden('small2'), list(model.store.params)), loss


@pytest.mark.parametrize('set_name', list(F.SETS))
def test_frozen_sets_on_a_forced_push_plan(set_name, monkeypatch):
    """the rule of tests/test_frozen_gpu.py::test_frozen_run_gives_the_unfrozen_gradients_on_the_trainable_parameters, the unfrozen run being the
    forced-push run of the same model"""
    g = FZ._golden('small2')
    with form(monkeypatch, True):
        model, batch, times, base, base_loss = _push_small2()
        ps = model.store
        frozen, train = F.freeze(model, set_name)
        try:
            loss, _ = _step(model, batch, times)
            plan = model._live[0]
            assert plan._frozen == frozenset(frozen)
            assert_form(plan, f'small2 forced push / {set_name}', push=True, side=True)
            ref = float(g['loss'])
            print(f'  [small2 forced push / {set_name}] loss {loss:.6f} reference {ref:.6f} (unfrozen run {base_loss:.6f}); {len(train)} of {len(ps.params)} train; '
                  f'the backward ends at {plan.bwd_end} of {len(plan.bwd)}')
            assert abs(loss - ref) <= FZ.LOSS_TOL * max(1., abs(ref))
            for n, p in ps.params.items():
                assert (p.grad is None) == (n in frozen), f'{n}: .grad is {"None" if p.grad is None else "set"}'
            for a, b in ps.frozen_ranges():
                assert not bool(ps.grad[a:b].view(torch.int32).any()), f'frozen range [{a}, {b}) of the gradient buffer is not all-zero bits'
            errs = FZ._grad_errors(model, g, train)
            if errs:
                sub = {k: base[k] for k in errs}
                bound = max(FZ.GRAD_MEAN_TOL, FZ.MARGIN * FZ._mean(sub))
                print(f'  trainable gradients: norm-weighted mean {FZ._mean(errs):.3e} (unfrozen forced-push run, same subset: {FZ._mean(sub):.3e}; bound {bound:.3e})')
                assert FZ._mean(errs) <= bound
            if set_name == 'all_frozen':
                assert plan.bwd_end == 0
            assert plan.ar_tail is None                                  # (a push sweep forms its layer's d pseudo_queries / d norm_keys.gamma whole)
        finally:
            F.unfreeze(model)


@pytest.mark.parametrize('name,low', [('d33', 17), ('w1088x2', 1)])
def test_frozen_lower_layers_on_a_natural_push_plan(name, low):
    """layers 0 .. low - 1 and everything under them (the embeddings, the time conditioning) frozen, layers low .. depth - 1, the final norm and the heads
    train - the `top_half` rule of tests/_frozen_cases.py with its own boundary: the backward list stops behind layer `low`, in front of every launch
    of a frozen layer, and the trainable gradients are those of the unfrozen run of the same model (GRAD_EQ: the same launches on the same operands)"""
    model, batch, times = _model(name)
    l0, g0 = _step(model, batch, times)
    plan = model._live[0]
    D = plan.md.depth
    assert_form(plan, f'{name} unfrozen', push=True, side=False)
    assert plan.bwd_end is None
    trains = lambda n: n.startswith(F.HEADS) or n == 'transformer.norm.gamma' or (F._layer(n) is not None and F._layer(n) >= low)
    for n, p in model.store.params.items():
        p.requires_grad_(trains(n))
    frozen = {n for n in model.store.params if not trains(n)}
    l1, g1 = _step(model, batch, times)
    assert model._live[0] is plan and plan._frozen == frozenset(frozen)
    assert_form(plan, f'{name} layers 0..{low - 1} frozen', push=True, side=False)
    assert plan.bwd_end is not None and 0 < plan.bwd_end < len(plan.bwd)
    head, tail = FZ._ops(plan.bwd[:plan.bwd_end]), FZ._ops(plan.bwd[plan.bwd_end:])
    print(f'  [{name}] the backward ends at {plan.bwd_end} of {len(plan.bwd)}: {head.count("tfx_attnres_bwd")} push sweeps in front, {tail.count("tfx_attnres_bwd")} behind')
    for op in PUSH_OPS + ('tfx_attn_bwd',):
        assert head.count(op) == D - low and tail.count(op) == low, op
    below = set()
    for i in range(low):
        below |= {plan.yf[i].data_ptr(), plan.ya[i].data_ptr(), plan.ag[i].data_ptr(), plan.xb[i].data_ptr(), plan.og[i].data_ptr()}
    for fn, a in plan.bwd[:plan.bwd_end]:
        if isinstance(fn, str) and hasattr(a, '_fields_'):
            vals = {getattr(a, f) for f, _ in a._fields_ if isinstance(getattr(a, f), int)}
            assert not (below & vals), f'{fn} in the truncated list reads an activation of a frozen layer'
    assert abs(l1 - l0) <= CK.LOSS_EQ * max(1., abs(l0))
    assert set(g1) == {n for n in model.store.params if trains(n)}
    for a, b in model.store.frozen_ranges():
        assert not bool(model.store.grad[a:b].view(torch.int32).any())
    worst = max((rel(g1[k], g0[k]), k) for k in g1)
    print(f'  [{name}] {len(g1)} trainable gradients against the unfrozen run: worst rel difference {worst[0]:.2e} ({worst[1]})')
    for k in g1:
        assert rel(g1[k], g0[k]) <= CK.GRAD_EQ, k


def test_lora_step_on_a_forced_push_plan_matches_reference_golden(monkeypatch):
    """tests/test_lora_gpu.py::test_adapted_step_matches_reference_golden itself, its gates and its code, on `lora_small2` with the push form forced"""
    made = []
    adapted = TL.adapted

    def keep(name, *a, **k):
        made.append(adapted(name, *a, **k))
        return made[-1]
    monkeypatch.setattr(TL, 'adapted', keep)
    with form(monkeypatch, True):
        TL.test_adapted_step_matches_reference_golden('lora_small2')
    assert len(made) == 1
    plan = made[0][2]._live[0]
    assert_form(plan, 'lora_small2 forced push', push=True, side=True)
    assert FZ._ops(plan.bwd).count('tfx_lora_grad') > 0


def test_accumulation_over_two_micro_batches_on_d33():
    """two micro-batches (the case's batch at its times t and at 1 - t): the accumulated gradients are the sum of the two single runs (GRAD_EQ), and an
    accumulation after `.grad = None` starts from zero"""
    model, batch, times = _model('d33')
    other = 1. - times
    l1, g1 = _step(model, batch, times)
    assert_form(model._live[0], 'd33 accumulation', push=True, side=False)
    l2, g2 = _step(model, batch, other)
    assert abs(l1 - l2) > 1e-4, 'the two micro-batches differ'
    for p in model.parameters():
        p.grad = None
    model(batch, times=times).backward()
    model(batch, times=other).backward()
    sync()
    acc = CK._grads(model)
    assert set(acc) == set(g1) == set(g2)
    worst = max((rel(acc[k], g1[k] + g2[k]), k) for k in acc)
    print(f'  [d33] two accumulated micro-batches against the sum of the single runs: worst rel difference {worst[0]:.2e} ({worst[1]})')
    for k in acc:
        assert rel(acc[k], g1[k] + g2[k]) <= CK.GRAD_EQ, k
    l3, g3 = _step(model, batch, times)                               # (_step starts from `.grad = None`)
    assert abs(l3 - l1) <= CK.LOSS_EQ * max(1., abs(l1))
    for k in g1:
        assert rel(g3[k], g1[k]) <= CK.GRAD_EQ, k


@pytest.mark.parametrize('name', ['d33', 'small2'])
def test_push_lists_replay_as_graphs(name, monkeypatch):
    """tests/test_model_gpu.py::test_training_lists_replay_as_graphs_while_their_fingerprint_holds on a push plan - `d33`: the single-stream list;
    `small2` forced: the push list with its weight-gradient GEMMs on the side stream"""
    from transfusion_pytorch_amd import engine
    forced, side = _expected(name)

    def steps(model, batch, times, n):
        return [_step(model, batch, times) for _ in range(n)]

    with form(monkeypatch, forced):
        ref, batch, times = _model(name)
        ref_loss, ref_grads = steps(ref, batch, times, 1)[0]
        assert_form(ref._live[0], f'{name} list replay', push=True, side=side)
        monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
        model, batch, times = _model(name)
        outs = steps(model, batch, times, 5)
        plan = model._live[0]
        assert_form(plan, f'{name} graph replay', push=True, side=side)
        st_f, st_b = plan.fwd._auto[(0, len(plan.fwd))], plan.bwd._auto[(0, len(plan.bwd))]
        assert st_f[1] and st_b[1] and st_f[2] >= 4, 'the fixed-shape loop must end up on graph replays'
        for i, (l, g) in enumerate(outs):
            assert abs(l - ref_loss) <= 1e-6 * max(1., abs(ref_loss)), i
            for k in ref_grads:
                assert rel(g[k], ref_grads[k]) <= 2e-3, (i, k)
        # a changed scalar: other loss seeds -> another fingerprint -> list replay, then a new capture
        model.flow_loss_weight = 2.0 * model.flow_loss_weight
        l2 = steps(model, batch, times, 1)[0][0]
        assert plan.fwd._auto[(0, len(plan.fwd))][1] is None and abs(l2 - ref_loss) > 1e-4
        l3 = [o[0] for o in steps(model, batch, times, 3)]
        assert plan.fwd._auto[(0, len(plan.fwd))][1] and all(abs(x - l2) <= 1e-6 * max(1., abs(l2)) for x in l3)


@pytest.mark.parametrize('name', ['small2', 'd33'])
def test_overlapped_exchange_on_a_push_plan_equals_the_plain_step_rccl_world1(name, monkeypatch):
    """tests/test_model_gpu.py::test_overlapped_gradient_exchange_equals_plain_step_rccl_world1 on a push plan, one process: one cut per exchange group -
    also on `d33`, whose list has no side stream to join - and loss, gradients and the stepped parameters of the plain path"""
    import torch.distributed as dist
    from transfusion_pytorch_amd.optim import FusedAdam
    forced, side = _expected(name)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29549')
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        res = []
        with form(monkeypatch, forced):
            for overlap in (False, True):
                model, batch, times = _model(name)
                opt = FusedAdam(model, lr=3e-4, max_grad_norm=0.5)
                opt.always_sync = True
                if overlap:
                    opt.overlap_grad_sync(groups=3)
                loss = model(batch, times=times)
                loss.backward()
                plan = model._live[0]
                assert_form(plan, f'{name} {"overlapped exchange" if overlap else "plain exchange"}', push=True, side=side)
                D = plan.md.depth
                per = -(-D // 3)
                cuts = [(lo, min(lo + per, D) - 1) for lo in range((D - 1) // per * per, -1, -per)]          # layer groups, top group first
                print(f'  [{name}] cuts {[(c[1], c[2]) for c in plan.bwd_cuts]}')
                assert [(c[1], c[2]) for c in plan.bwd_cuts] == (cuts if overlap else [])
                assert all(0 < c[0] <= len(plan.bwd) for c in plan.bwd_cuts) and [c[0] for c in plan.bwd_cuts] == sorted(c[0] for c in plan.bwd_cuts)
                grads = CK._grads(model)
                opt.step()
                sync()
                res.append((float(loss), grads, model.store.flat.clone()))
        (l0, g0, p0), (l1, g1, p1) = res
        assert abs(l0 - l1) <= 1e-6 * max(1., abs(l0))
        for k in g0:
            assert rel(g1[k], g0[k]) <= 2e-3, k
        assert rel(p1, p0) <= 1e-5
    finally:
        if own:
            dist.destroy_process_group()
