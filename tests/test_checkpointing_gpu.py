"""Activation checkpointing on the GPU (Transfusion.set_activation_checkpointing_, engine.Plan `ckpt`): the forward is unchanged, the backward's recompute
segments rebuild every layer's saved activations bit for bit, and the gradients are those of the plain step.

Bounds: losses of identical launches 1e-6 max(1, |loss|) and gradients rel-Frobenius 2e-3 - the figures of
tests/test_model_gpu.py::test_side_stream_weight_gradients_equal_single_stream for identical launch sets whose fp32 atomics arrive in another order; the
reference goldens under the gates of tests/test_model_gpu.py::test_training_step_matches_reference_golden, run through that test's own code."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import build_case, build_modality_case, build_text_case          # noqa: E402

import test_model_gpu as TM                                                         # noqa: E402  (run_native, build_native, rel and the golden gates)

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
LOSS_EQ, GRAD_EQ = 1e-6, 2e-3
FAMILY = ('ua', 'uf', 'qkvg', 'qkr', 'og', 'lse', 'ya', 'xb', 'yf', 'ag', 'hm')        # + stats (layer axis second), xa (skip layers), vl (LASER)
rel = TM.rel


def sync():
    torch.cuda.synchronize()


def _native(cfg, sd, ckpt, **switches):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    m = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                    transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, **switches), prob_uncond=0.)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    return m.set_activation_checkpointing_(True) if ckpt else m


def _fixture(name):
    """(cfg, state dict, batch, times, noise, transformer switches) of a fixture name: the oracle cases, their LASER / ablation variants (same weights and
    inputs, the switch set; without value gates the state dict has no `to_gates`), and the odd-depth configuration of test_odd_configurations_match_live_oracle"""
    import _ablation_cases as AB
    if name == 'odd5':
        from oracle import detdata as D
        from oracle.transfusion_oracle import OracleConfig
        cfg = OracleConfig(num_text_tokens=96, dim=320, depth=5, dim_latents=(24, 72), heads=2, dim_head=64)
        tag = 'odd/320/5/2'
        batch = D.ragged_batch(f'{tag}/b', 3, cfg.num_text_tokens, cfg.dim_latents)
        return cfg, D.det_state_dict(cfg.state_dict_shapes(), tag=tag), batch, D.det_times(f'{tag}/t', batch), D.det_noise(f'{tag}/n', batch, cfg.num_modalities), {}
    sw = {'laser_small2': dict(attn_laser=True), 'ablate_both_small2': AB.BOTH}.get(name, {})
    cfg, sd, batch, times, noise = build_case('small2' if sw else name)
    return cfg, AB.strip_state(sd, sw), batch, times, noise, sw


def _forward(name, ckpt, model=None):
    cfg, sd, batch, times, noise, sw = _fixture(name)
    if model is None:
        model = _native(cfg, sd, ckpt, **sw)
        model._noise_override = {t: v.cuda() for t, v in noise.items()}
    loss = model(batch, times=times)
    sync()
    return model, loss, model._live[0]


def _grads(model):
    return {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}


def _same_step(a, b, what=''):
    """(loss, gradients) of the checkpointed run `a` against the plain run `b` of the same step"""
    (la, ga), (lb, gb) = a, b
    assert abs(la - lb) <= LOSS_EQ * max(1., abs(lb)), (what, la, lb)
    assert set(ga) == set(gb) and ga, what
    worst = max(((rel(ga[k], gb[k]) if float(gb[k].norm()) > 0 else float(ga[k].norm())), k) for k in gb)
    print(f'  {what}: loss {la:.6f} / {lb:.6f}; {len(gb)} gradients, worst rel difference {worst[0]:.2e} ({worst[1]})')
    for k in gb:
        if float(gb[k].norm()) == 0.:
            assert float(ga[k].norm()) == 0., (what, k)
        else:
            assert rel(ga[k], gb[k]) <= GRAD_EQ, (what, k)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ================================================================================================ 1. forward unchanged
@pytest.mark.parametrize('name', ['small2', 'head8', 'laser_small2'])
def test_forward_is_unchanged(name):
    mp, lp, P = _forward(name, False)
    mc, lc, C = _forward(name, True)
    assert C.ckpt and C.n_slots in (1, 2) and not P.ckpt
    assert torch.equal(C.logits, P.logits) and torch.equal(C.embed, P.embed)
    for t in P.lat:
        assert torch.equal(C.lat[t]['pred'], P.lat[t]['pred']), t
    lc, lp = float(lc.detach()), float(lp.detach())
    print(f'  [{name}] loss checkpointed {lc:.8f} plain {lp:.8f}')
    assert abs(lc - lp) <= LOSS_EQ * max(1., abs(lp))


# ================================================================================================ 2. the recompute reproduces every layer
def _layer_views(plan, i, nt):
    """layer i's saved activations over the step's real rows (b, n real columns, ...): name -> tensor"""
    b, n, s, lk = plan.b, plan.n, plan._li(i), plan._lkv(i)
    out = {}
    for k in FAMILY:
        t = getattr(plan, k)[lk if k in ('qkvg', 'qkr') else s]
        out[k] = t[:, :, :nt] if k == 'lse' else t.view(b, n, -1)[:, :nt]
    out['stats'] = plan.stats[:, s].view(4, b, n)[:, :, :nt]
    if i in plan.xa:
        out['xa'] = plan.xa[i].view(b, n, -1)[:, :nt]
    if plan.vl is not None:
        out['vl'] = plan.vl[s].view(b, n, -1)[:, :nt]
    return out


def _zero_family(plan):
    """what a launch leaves unwritten (column padding of the row strides) is whatever the allocator handed out: zero in both plans, so that equality is
    about what the launches write.  A segment that failed to write something would leave another layer's values there."""
    for k in FAMILY + ('stats',):
        getattr(plan, k).zero_()
    for t in plan.xa.values():
        t.zero_()
    if plan.vl is not None:
        plan.vl.zero_()


@pytest.mark.parametrize('side', ['1', '0'])
@pytest.mark.parametrize('name', ['small2', 'odd5', 'laser_small2', 'ablate_both_small2'])
def test_recompute_reproduces_every_layer_bit_for_bit(name, side, monkeypatch):
    from transfusion_pytorch_amd.engine import Plan
    monkeypatch.setenv('TFX_SIDE_STREAM', side)                      # read per Plan: 1 = weight gradients on the side stream, two slots; 0 = one
    plans = []
    for ckpt in (False, True):
        model, _, plan = _forward(name, ckpt)
        _zero_family(plan)
        _, _, again = _forward(name, ckpt, model)
        assert again is plan
        plans.append((model, plan))
    (mp, P), (mc, C) = plans
    D, ns, nt = P.md.depth, (2 if side == '1' else 1), mc._live_n_true
    assert C.n_slots == ns and all(getattr(C, k).shape[0] == ns for k in FAMILY) and all(getattr(P, k).shape[0] == D for k in FAMILY)
    kept = [C.hid] + C.xres[1:] + C.arsave + [C.arerr]
    before = [_bits(t).clone() for t in kept]
    stream = torch.cuda.current_stream().cuda_stream
    replayed = 0
    for i in range(D - 1, -1, -1):
        rng = C.recompute_range(i)
        assert (rng is None) == (i >= D - ns), i                    # the top n_slots layers are as the forward left them
        if rng is not None:
            names = [it[0] if isinstance(it[0], str) else it[0].__name__ for it in C.bwd[rng[0]:rng[1]]]
            assert 'tfx_layer_end_fwd' not in names and names[-1] == 'tfx_gemm_nt'
            Plan.run(C.bwd, stream, *rng)
            sync()
            replayed += 1
        want, got = _layer_views(P, i, nt), _layer_views(C, i, nt)
        assert set(want) == set(got)
        for k in want:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f'{name}: layer {i} {k} differs from the plain forward'
    assert replayed == max(D - ns, 0)
    for t, b in zip(kept, before):
        assert torch.equal(_bits(t), b), 'a recompute segment wrote hid / xres / arsave / arerr'
    assert torch.equal(C.hid, P.hid)


# ================================================================================================ 3. gradients
@functools.lru_cache(maxsize=None)
def _plain_run(name):
    return TM.run_native(name)[2]


@pytest.mark.parametrize('name', ['tiny1', 'small2', 'mid2', 'head8', 'canon512'])
def test_gradients_match_reference_golden_and_the_plain_step(name, monkeypatch):
    """(a) tests/test_model_gpu.py::test_training_step_matches_reference_golden itself - its gates LOSS_TOL, LOGIT_TOL, GRAD_TOL, GRAD_MEAN_TOL,
    GRAD_HEAD_TOL, its code - on a model with the switch on; (b) the same run against the plain run of the step"""
    plain = _plain_run(name)
    built, runs = [], []
    build, run = TM.build_native, TM.run_native

    def build_ckpt(cfg, sd):
        built.append(build(cfg, sd).set_activation_checkpointing_(True))
        return built[-1]

    def run_keep(nm):
        runs.append(run(nm))
        return runs[-1]
    monkeypatch.setattr(TM, 'build_native', build_ckpt)
    monkeypatch.setattr(TM, 'run_native', run_keep)
    monkeypatch.setattr(TM, '_log_parity', lambda *a, **k: None)      # (the parity log is about the default path)
    TM.test_training_step_matches_reference_golden(name)
    assert len(built) == 1 and len(runs) == 1
    plan = built[0]._live[0]
    assert plan.ckpt and len(plan._recompute) == max(plan.md.depth - plan.n_slots, 0)
    out = runs[0][2]
    assert torch.equal(out['logits'], plain['logits'])
    _same_step((out['loss'], out['grads']), (plain['loss'], plain['grads']), name)


# ================================================================================================ 4. interactions
def _pair(make, step, what):
    """`step(model)` -> loss on a plain and a checkpointed `make(ckpt)`; the two steps compared; returns the models"""
    res = []
    for ckpt in (False, True):
        model = make(ckpt)
        loss = step(model)
        sync()
        assert model._live[0].ckpt == ckpt
        res.append((model, (float(loss), _grads(model))))
    _same_step(res[1][1], res[0][1], what)
    return res[0][0], res[1][0]


def _small2(ckpt, name='small2'):
    cfg, sd, batch, times, noise = build_case(name)
    m = _native(cfg, sd, ckpt)
    m._noise_override = {t: v.cuda() for t, v in noise.items()}
    return m, batch, times


def _step_small2(model, batch, times):
    loss = model(batch, times=times)
    loss.backward()
    return loss


def test_frozen_trunk_trainable_heads_never_recompute():
    heads = lambda n: n == 'to_text_logits.weight' or n.startswith('model_to_latent_projs.')
    batch_times = {}

    def make(ckpt):
        m, batch, times = _small2(ckpt)
        batch_times['bt'] = (batch, times)
        for n, p in m.store.params.items():
            p.requires_grad_(heads(n))
        return m
    mp, mc = _pair(make, lambda m: _step_small2(m, *batch_times['bt']), 'frozen trunk')
    C = mc._live[0]
    assert C.bwd_end is not None and 0 < C.bwd_end < len(C.bwd)
    segs = [C.recompute_range(i) for i in range(C.md.depth - C.n_slots)]
    assert segs and all(s is not None and s[0] >= C.bwd_end for s in segs), 'the truncated list must hold no recompute segment'
    assert all((p.grad is None) != heads(n) for n, p in mc.store.params.items())


def test_lora_adapters_on_lora_small2():
    import test_lora_gpu as TL
    g = TL.fixture('lora_small2')
    cfg, sd, batch, times, noise = build_case(g['base_case'])

    def make(ckpt):
        m = TL.attach(_native(cfg, sd, ckpt), g).train()
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        return m
    mp, mc = _pair(make, lambda m: _step_small2(m, batch, times), 'lora_small2')
    got = _grads(mc)
    assert all(f'lora.{k}' in got for k in g['grads']), 'dA and dB of every adapter'
    assert any(it[0] == 'tfx_lora_grad' for it in mc._live[0].bwd)


def test_hidden_tap_on_selfflow_taps_small2():
    import _self_flow_cases as SF
    g = torch.load(os.path.join(GOLDEN, f'{SF.TAPS_FIXTURE}.pt'), weights_only=False)
    cfg, sd, batch, times, noise = build_case(g['base_case'])
    taps = [k for k in SF.tap_indices(cfg.depth)]

    def step(model):
        loss, hiddens = model(batch, times=times, return_hiddens=True)
        total = loss
        for k in taps:
            total = total + g['taps'][k]['w'] * hiddens[k].pow(2).mean()
        total.backward()
        return loss

    def make(ckpt):
        m = _native(cfg, sd, ckpt)
        m._noise_override = {t: v.cuda() for t, v in noise.items()}
        return m
    _pair(make, step, f'hidden taps {taps}')


def test_self_flow_wrapper_with_the_switch_on_its_student():
    """SelfMaskedRepTraining: the switch is set on `wrapper.student`; the teacher's no-grad pass runs on its hiddens-only plan either way"""
    import test_self_flow_gpu as TS
    name = 'selfflow_small2_m3_m1'
    g = torch.load(os.path.join(GOLDEN, f'{name}.pt'), weights_only=False)
    res = []
    for ckpt in (False, True):
        w, cfg, batch, times = TS._wrapper(g)
        assert w.student.activation_checkpointing is False
        if ckpt:
            assert w.student.set_activation_checkpointing_(True) is w.student
        total, (student_loss, rep) = w(batch, num_modalities_to_times_fn=lambda n: times.cuda())
        total.backward(); sync()
        assert w.student._live[0].ckpt == ckpt and not w._teacher_plan.ckpt
        grads = {k: p.grad.detach().float().clone() for k, p in w.named_parameters() if p.grad is not None}
        res.append((float(total.detach()), grads))
    _same_step(res[1], res[0], name)


def test_accumulation_under_no_sync_then_fused_adam_step():
    from transfusion_pytorch_amd.optim import FusedAdam
    res = []
    for ckpt in (False, True):
        m, batch, times = _small2(ckpt)
        opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
        with opt.no_sync():
            m(batch, times=times).backward()
        m(batch, times=times).backward()
        g = m.store.grad.clone()
        opt.step(); sync()
        assert m._live[0].ckpt == ckpt
        res.append((g, m.store.flat.clone()))
    (g0, p0), (g1, p1) = res
    print(f'  accumulated gradient buffer rel {rel(g1, g0):.2e}; parameters after the step rel {rel(p1, p0):.2e}')
    # gradients: GRAD_EQ; the stepped parameters: the 1e-5 tests/test_model_gpu.py holds two identical-launch steps to after one FusedAdam step
    assert rel(g1, g0) <= GRAD_EQ and rel(p1, p0) <= 1e-5


def test_forward_text_and_forward_modality_training_plans():
    cfg, sd, text = build_text_case('text1')
    _pair(lambda ckpt: _native(cfg, sd, ckpt), lambda m: (lambda l: (l.backward(), l)[1])(m.forward_text(text)), 'forward_text text1')
    cfg, sd, x, times, noise, ty = build_modality_case('flow1')

    def make(ckpt):
        m = _native(cfg, sd, ckpt)
        m._noise_override = {ty: noise.cuda()}
        return m
    _pair(make, lambda m: (lambda l: (l.backward(), l)[1])(m.forward_modality(x, times=times, modality_type=ty)), 'forward_modality flow1')


def test_overlapped_exchange_rccl_world1_keeps_its_cuts():
    import torch.distributed as dist
    from transfusion_pytorch_amd.optim import FusedAdam
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29547')
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        res = []
        for ckpt in (False, True):
            m, batch, times = _small2(ckpt)
            opt = FusedAdam(m, lr=3e-4, max_grad_norm=0.5)
            opt.always_sync = True
            opt.overlap_grad_sync(groups=3)
            loss = m(batch, times=times)
            loss.backward()
            plan = m._live[0]
            assert plan.ckpt == ckpt and len(plan.bwd_cuts) == 2                       # depth 4 in groups of 2 layers
            grads = _grads(m)
            opt.step(); sync()
            res.append((plan, (float(loss), grads), m.store.flat.clone()))
        (P, sp, p0), (C, sc, p1) = res
        _same_step(sc, sp, 'overlapped exchange, world 1')
        assert [c[1:] for c in C.bwd_cuts] == [c[1:] for c in P.bwd_cuts]
        # a layer's segment stands behind the cut that hands the group above it over: the exchange starts before the recompute of the next group
        for idx, first, last in C.bwd_cuts:
            for i in range(first):
                assert C.recompute_range(i) is None or C.recompute_range(i)[0] >= idx
        assert rel(p1, p0) <= 1e-5
    finally:
        if own:
            dist.destroy_process_group()


def test_training_graph_replay_from_the_third_step(monkeypatch):
    from transfusion_pytorch_amd import engine
    m, batch, times = _small2(False)
    loss = _step_small2(m, batch, times); sync()
    ref = (float(loss), _grads(m))
    monkeypatch.setattr(engine, 'TRAIN_GRAPH', True)
    m, batch, times = _small2(True)
    for step in range(5):
        for p in m.parameters():
            p.grad = None
        loss = _step_small2(m, batch, times); sync()
        plan = m._live[0]
        if step >= 2:
            st_f, st_b = plan.fwd._auto[(0, len(plan.fwd))], plan.bwd._auto[(0, len(plan.bwd))]
            assert st_f[1] and st_b[1], 'from the third identical step both lists replay as graphs'
        _same_step((float(loss), _grads(m)), ref, f'TFX_TRAIN_GRAPH step {step}')
    assert plan.ckpt and plan.bwd._auto[(0, len(plan.bwd))][2] >= 4


def test_second_backward_of_the_same_loss_still_raises():
    m, batch, times = _small2(True)
    loss = m(batch, times=times)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()


# ================================================================================================ 5. memory and switching
def _fingerprint(lst):
    from transfusion_pytorch_amd import capi
    fp = ctypes.c_int64()
    assert capi.lib().tfx_list_fingerprint(lst.native(), len(lst), ctypes.byref(fp)) == 0
    return fp.value


def _shape_key(lst):
    """a list without its addresses: entry points, streams and every non-pointer argument (sizes, strides, counts, scalars)"""
    from transfusion_pytorch_amd import capi
    out = []
    for item in lst:
        fn, a = item
        name = fn if isinstance(fn, str) else fn.__name__
        if isinstance(a, ctypes.Structure):
            vals = tuple((f, getattr(a, f)) for f, ty in a._fields_ if ty in (ctypes.c_int32, ctypes.c_int, ctypes.c_float))
        elif isinstance(a, (tuple, list)):
            vals = tuple(v for v, ty in zip(a, capi.FUNCTIONS[name][1]) if ty is not ctypes.c_void_p)
        else:
            vals = a
        out.append((type(item).__name__, name, vals))
    return out


@pytest.mark.parametrize('side', ['1', '0'])
def test_memory_and_switching(side, monkeypatch):
    """The byte condition is the allocation arithmetic, not a measurement: the plain plan holds `depth` entries of the family and one `xa` per skip layer, the
    checkpointed one `n_slots` entries and at most `n_slots` `xa` buffers (so `xa` saves by the skip layers' count, not by `depth`).  `tfx_list_fingerprint`
    hashes buffer addresses, so the lists "of a model that never had the switch on" are this model's before its first switch; a fresh model's lists are
    compared without their addresses."""
    monkeypatch.setenv('TFX_SIDE_STREAM', side)
    ns = 2 if side == '1' else 1
    m, batch, times = _small2(False)
    assert m.activation_checkpointing is False
    l0 = _step_small2(m, batch, times); sync()
    P = m._live[0]
    fp0 = (_fingerprint(P.fwd), _fingerprint(P.bwd))                   # the model has never had the switch on
    m.set_activation_checkpointing_(True)
    _step_small2(m, batch, times); sync()
    C = m._live[0]
    assert C is not P and C.ckpt and not P.ckpt
    assert sum(p is P for p in m._plans.values()) == 1 and sum(p is C for p in m._plans.values()) == 1, 'both plans sit in the cache'
    # the family's leading dimension, and the bytes by the allocation arithmetic: D entries against n_slots, one xa per skip layer against at most n_slots
    D = P.md.depth
    fam = [getattr(C, k) for k in FAMILY] + ([C.vl] if C.vl is not None else [])
    assert C.n_slots == ns and all(t.shape[0] == ns for t in fam) and C.stats.shape[1] == ns
    nb = lambda t: t.numel() * t.element_size()
    slot_bytes = sum(nb(t) for t in fam + [C.stats]) // ns
    xa_c = {t.data_ptr(): t for t in C.xa.values()}
    assert len(xa_c) <= ns
    xa_saved = sum(nb(t) for t in P.xa.values()) - sum(nb(t) for t in xa_c.values())
    print(f'  n_slots {ns}: plan bytes plain {P.nbytes} checkpointed {C.nbytes}; slot bytes {slot_bytes}, xa bytes saved {xa_saved}')
    assert xa_saved >= 0 and C.nbytes <= P.nbytes - (D - ns) * slot_bytes - xa_saved
    # switching back: the plan that never saw the switch, its lists byte for byte what they were
    m.set_activation_checkpointing_(False)
    for p in m.parameters():
        p.grad = None
    l2 = _step_small2(m, batch, times); sync()
    assert m._live[0] is P
    assert (_fingerprint(P.fwd), _fingerprint(P.bwd)) == fp0
    assert abs(float(l2) - float(l0)) <= LOSS_EQ * max(1., abs(float(l0)))
    # ... and item for item those of a fresh model that never had it (addresses aside)
    f, batch, times = _small2(False)
    _step_small2(f, batch, times); sync()
    F = f._live[0]
    assert _shape_key(F.fwd) == _shape_key(P.fwd) and _shape_key(F.bwd) == _shape_key(P.bwd) and F.nbytes == P.nbytes
    assert _shape_key(C.fwd) == _shape_key(P.fwd) and len(C.bwd) > len(P.bwd)
