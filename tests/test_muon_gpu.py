"""optim.FusedMuon on the MI355X: the grouped Newton-Schulz kernels alone, the orthogonalisation against torch's rule, whole optimizer steps
against clip_grad_norm_ + torch.optim.Muon + torch.optim.Adam, determinism, and the plumbing around it (csrc/muon.hip, optim.py).

Tolerances are derived, not measured:
  * a grouped product rounds its fp32 result to bf16 once (relative 2^-9) on top of fp32 accumulation error, so an element may deviate from the
    fp64 product of the bf16-rounded operands by 2^-8 of the magnitude sum  |alpha||Z| + |beta| sum_k |P_ik||Q_jk|;
  * Newton-Schulz in bf16 deviates from its fp64 restatement by 1e-2 (well-conditioned) ... 1.5e-1 (low rank) in BOTH implementations, so the
    native result is held to 1.5 x the deviation of `torch.optim._muon._zeropower_via_newtonschulz` on the same matrix (the project's standing
    margin over the reference's own bf16 deviation), per matrix, never to an absolute figure.
"""
import os
import sys

import pytest
import torch

from oracle.cases import build_case
from transfusion_pytorch_amd import capi

pytestmark = pytest.mark.gpu
DEV, BF = 'cuda', torch.bfloat16
NS = (3.4445, -4.775, 2.0315)
MARGIN = 1.5
WORST = {}          # measured worst native / torch deviation ratios of this run (printed; quoted in README)


def stream():
    return torch.cuda.current_stream().cuda_stream


def build_native(cfg, sd):
    from transfusion_pytorch_amd import Transfusion
    dl = cfg.dim_latents if len(cfg.dim_latents) > 1 else cfg.dim_latents[0]
    model = Transfusion(num_text_tokens=cfg.num_text_tokens, dim_latent=dl,
                        transformer=dict(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads), prob_uncond=0.)
    model.load_state_dict(sd, strict=True)
    return model.cuda()


def falling(losses, k=10):
    first, last = sum(losses[:k]) / k, sum(losses[-k:]) / k
    print(f'  loss: first {k} steps {first:.3f} -> last {k} steps {last:.3f}')
    return last < 0.9 * first


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def pad128(v):
    return -(-v // 128) * 128


# ---------------------------------------------------------------------------------------------------------------- 1. grouped products alone
def run_group(problems, alpha, beta):
    """problems: dicts with P (M x K), Q (N x K), optional Z (M x N), ct (also write the transpose), sz / sa (device-side scales).  Operands are
    zero-padded to the tile by the caller's contract (here), the whole group is ONE launch.  Returns per problem the padded C (and Ct)."""
    S = capi.STRUCTS['tfx_muon_gemm_problem']
    arr, keep, tile_prob, tile0 = (S * len(problems))(), [], [], 0
    for i, (a, pr) in enumerate(zip(arr, problems)):
        M, K = pr['P'].shape
        N = pr['Q'].shape[0]
        Mp, Np, Kp = pad128(M), pad128(N), pad128(K) if not pr.get('k64') else -(-K // 64) * 64      # k64: K padded to the kernel's own multiple (tfx.h)

        def padded(t, r, c):
            o = torch.zeros(r, c, dtype=BF, device=DEV)
            o[:t.shape[0], :t.shape[1]] = t.to(BF)
            return o
        P, Q = padded(pr['P'], Mp, Kp), padded(pr['Q'], Np, Kp)
        Z = padded(pr['Z'], Mp, Np) if pr.get('Z') is not None else None
        C = torch.full((Mp, Np), float('nan'), dtype=BF, device=DEV)                # every element must be written
        Ct = torch.full((Np, Mp), float('nan'), dtype=BF, device=DEV) if pr.get('ct') else None
        sz = torch.tensor([pr['sz']], device=DEV) if pr.get('sz') is not None else None
        sa = torch.tensor([pr['sa']], device=DEV) if pr.get('sa') is not None else None
        a.P, a.Q, a.C = P.data_ptr(), Q.data_ptr(), C.data_ptr()
        a.Z = Z.data_ptr() if Z is not None else None
        a.Ct = Ct.data_ptr() if Ct is not None else None
        a.scale_z = sz.data_ptr() if sz is not None else None
        a.scale_acc = sa.data_ptr() if sa is not None else None
        a.M, a.N, a.K, a.ldp, a.ldq, a.ldz, a.ldc, a.ldct, a.tile0 = Mp, Np, Kp, Kp, Kp, Np, Np, Mp, tile0
        nt = (Mp // 128) * (Np // 128)
        tile_prob += [i] * nt; tile0 += nt
        keep.append(dict(P=P, Q=Q, Z=Z, C=C, Ct=Ct, sz=sz, sa=sa))
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    tp = torch.tensor(tile_prob, dtype=torch.int32, device=DEV)
    capi.check(capi.lib().tfx_muon_gemm(tab.data_ptr(), tp.data_ptr(), tile0, alpha, beta, stream()), 'tfx_muon_gemm')
    torch.cuda.synchronize()
    return keep


def check_group(tag, problems, alpha, beta):
    out = run_group(problems, alpha, beta)
    for i, (pr, o) in enumerate(zip(problems, out)):
        M, N = pr['P'].shape[0], pr['Q'].shape[0]
        P, Q = o['P'].double(), o['Q'].double()                                  # the bf16-rounded, padded operands
        sz, sa = pr.get('sz') or 1., pr.get('sa') or 1.
        sz, sa = float(torch.tensor(sz, dtype=torch.float32)), float(torch.tensor(sa, dtype=torch.float32))
        want = beta * sa * (P @ Q.T)
        mag = abs(beta * sa) * (P.abs() @ Q.abs().T)
        if o['Z'] is not None:
            want = want + alpha * sz * o['Z'].double()
            mag = mag + abs(alpha * sz) * o['Z'].double().abs()
        got = o['C'].double()
        assert torch.isfinite(got).all(), f'{tag}[{i}]: an output element was not written'
        err = (got - want).abs()
        worst = float((err / (mag + 1e-300))[:M, :N].max())
        print(f'  {tag}[{i}] {M} x {N} x {pr["P"].shape[1]}: max |err| / magnitude sum {worst:.3e} (bound {2 ** -8:.3e})')
        assert bool((err <= 2 ** -8 * mag).all()), f'{tag}[{i}]: {worst}'
        pad = got.clone(); pad[:M, :N] = 0
        assert float(pad.abs().max()) == 0., f'{tag}[{i}]: padding is not exactly zero'
        if o['Ct'] is not None:
            assert torch.equal(o['Ct'], o['C'].T.contiguous()), f'{tag}[{i}]: the transposed copy differs from the result'


def test_grouped_products_asymmetric_ragged():
    """ASYMMETRIC operands (inside Newton-Schulz A and B are symmetric, which would hide a transposed store), ragged sizes from
    {32, 96, 128, 340, 512, 1365, 2730}, several problems of different sizes in ONE launch, for each of the three product forms"""
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    # gram form: C = P . Q^T (no addend), K = the long side
    check_group('gram', [dict(P=rn(512, 2730), Q=rn(340, 2730)), dict(P=rn(32, 128), Q=rn(96, 128)), dict(P=rn(128, 1365), Q=rn(512, 1365)),
                         dict(P=rn(340, 96), Q=rn(32, 96), sa=0.37)], 0., 1.)
    # poly form: C = b Z + c P . Q^T, square
    check_group('poly', [dict(P=rn(512, 512), Q=rn(512, 512), Z=rn(512, 512)), dict(P=rn(96, 96), Q=rn(96, 96), Z=rn(96, 96)),
                         dict(P=rn(340, 340), Q=rn(340, 340), Z=rn(340, 340)), dict(P=rn(128, 128), Q=rn(128, 128), Z=rn(128, 128))], NS[1], NS[2])
    # update form: C (n x m) = a Z + P . Q^T and its transpose, device-side scales as in the first iteration
    check_group('update', [dict(P=rn(2730, 512), Q=rn(512, 512), Z=rn(2730, 512), ct=True), dict(P=rn(128, 32), Q=rn(32, 32), Z=rn(128, 32), ct=True),
                           dict(P=rn(1365, 340), Q=rn(340, 340), Z=rn(1365, 340), ct=True, sz=0.61, sa=0.61),
                           dict(P=rn(96, 96), Q=rn(96, 96), Z=rn(96, 96), ct=True)], NS[0], 1.)
    # the 2-slot K ring: the groups above walk 2, 6, 8, 22 and 44 K-tiles (workspace matrices are padded to 128).  One tile = no refill; three = the
    # shortest odd walk, which ends on slot 0
    check_group('ring', [dict(P=rn(96, 64), Q=rn(128, 64), k64=True), dict(P=rn(128, 180), Q=rn(340, 180), k64=True, sa=0.37)], 0., 1.)


# ---------------------------------------------------------------------------------------------------------------- 2. orthogonalisation
def ns_fp64(u, coefficients=NS, steps=5, eps=1e-7):
    """the rule of torch/optim/_muon.py:24-62 restated in fp64"""
    a, b, c = coefficients
    X = u.double()
    flip = X.shape[0] > X.shape[1]
    if flip:
        X = X.T
    X = X / X.norm().clamp(min=eps)
    for _ in range(steps):
        A = X @ X.T
        B = b * A + c * (A @ A)
        X = a * X + B @ X
    return X.T if flip else X


def check_orthogonalisation(tag, mats, got, steps=5):
    from torch.optim._muon import _zeropower_via_newtonschulz
    worst = 0.
    for i, (u, o) in enumerate(zip(mats, got)):
        ref = ns_fp64(u, steps=steps)
        tor = _zeropower_via_newtonschulz(u, NS, steps, 1e-7)
        assert o.shape == u.shape and torch.isfinite(o.float()).all()
        en, et = rel(o, ref), rel(tor, ref)
        worst = max(worst, en / et)
        print(f'  {tag}[{i}] {tuple(u.shape)}: native vs fp64 {en:.3e}, torch vs fp64 {et:.3e}, ratio {en / et:.3f}')
        assert en <= MARGIN * et, f'{tag}[{i}] {tuple(u.shape)}: native {en} > {MARGIN} x torch {et}'
    WORST[tag] = max(WORST.get(tag, 0.), worst)
    print(f'  {tag}: worst native / torch deviation ratio {worst:.3f}')


def canon_gradients():
    cfg, sd, batch, times, noise = build_case('canon512')
    model = build_native(cfg, sd)
    model.train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    model(batch, times=times).backward()
    torch.cuda.synchronize()
    return model


def test_orthogonalisation_against_torch_rule():
    from transfusion_pytorch_amd.optim import newton_schulz
    model = canon_gradients()
    real = [p.grad.detach().float().clone() for p in model.muon_parameters()]
    assert len(real) == 32
    check_orthogonalisation('canon512 gradients', real, newton_schulz(real))
    g = torch.Generator(device=DEV).manual_seed(1)
    shapes = [(512, 512), (2730, 512), (512, 1365), (128, 128), (340, 128), (32, 128), (128, 32), (64, 16)]
    gauss = [torch.randn(r, c, device=DEV, generator=g) * 1e-3 for r, c in shapes]
    check_orthogonalisation('gaussian', gauss, newton_schulz(gauss))
    low = []
    for r, c in shapes:
        k = min(8, r, c)
        m = torch.randn(r, k, device=DEV, generator=g) @ torch.randn(k, c, device=DEV, generator=g)
        low.append(m + 0.05 * m.std() * torch.randn(r, c, device=DEV, generator=g))
    check_orthogonalisation('rank 8 + 5 % noise', low, newton_schulz(low))
    check_orthogonalisation('gaussian, 1 iteration', gauss, newton_schulz(gauss, ns_steps=1), steps=1)


# ---------------------------------------------------------------------------------------------------------------- 3. full steps against torch
def fresh_model(name):
    cfg, sd, batch, times, noise = build_case(name)
    model = build_native(cfg, sd)
    model.train()
    return model, batch


def record_gradients(name, n=3):
    model, batch = fresh_model(name)
    grads = []
    for k in range(n):
        torch.manual_seed(100 + k)
        model.store.grad.zero_()
        model(batch).backward()
        torch.cuda.synchronize()
        grads.append(model.store.grad.clone())
    assert not model.external_parameters()
    return grads


STEP_CASES = [('canon512', {}), ('head8', {}), ('head8', dict(nesterov=False)), ('small2', dict(muon_weight_decay=0.)),
              ('small2', dict(adjust_lr_fn='original')), ('head8', dict(adjust_lr_fn='match_rms_adamw')), ('small2', dict(ns_steps=1))]


@pytest.mark.parametrize('name,kw', STEP_CASES, ids=[f'{n}-{"-".join(f"{k}={v}" for k, v in kw.items()) or "default"}' for n, kw in STEP_CASES])
def test_steps_against_torch_muon_and_adam(name, kw):
    """path A: clip_grad_norm_(0.5) + torch.optim.Muon(muon_parameters) + torch.optim.Adam(rest); path B: FusedMuon(max_grad_norm=0.5); path C: FusedAdam
    from the same state (same fixed-order clip norm).  Three steps on the SAME recorded gradients."""
    from transfusion_pytorch_amd.optim import FusedAdam, FusedMuon
    grads = record_gradients(name)
    mb, _ = fresh_model(name)
    mc, _ = fresh_model(name)
    muon_kw = dict(muon_lr=1e-3, muon_weight_decay=0.1, momentum=0.95, nesterov=True, ns_steps=5, adjust_lr_fn=None)
    muon_kw.update(kw)
    ob = FusedMuon(mb, lr=3e-4, max_grad_norm=0.5, **muon_kw)
    oc = FusedAdam(mc, lr=3e-4, max_grad_norm=0.5)
    oc.deterministic_norm = True                                  # the same clip coefficient, bit for bit, as path B
    ps = mb.store
    names = list(ps.params)
    muon_ids = {id(p) for p in mb.muon_parameters()}
    is_muon = [id(ps.params[n]) in muon_ids for n in names]
    ref = [ps.params[n].detach().clone().requires_grad_(True) for n in names]
    t_muon = torch.optim.Muon([r for r, m in zip(ref, is_muon) if m], lr=muon_kw['muon_lr'], weight_decay=muon_kw['muon_weight_decay'],
                              momentum=muon_kw['momentum'], nesterov=muon_kw['nesterov'], ns_coefficients=NS, eps=1e-7, ns_steps=muon_kw['ns_steps'],
                              adjust_lr_fn=muon_kw['adjust_lr_fn'])
    t_adam = torch.optim.Adam([r for r, m in zip(ref, is_muon) if not m], lr=3e-4)
    mask = torch.zeros(ps.numel, dtype=torch.bool, device=DEV)
    for n, m in zip(names, is_muon):
        if m:
            o, shape = ps.offsets[n]
            mask[o:o + ps.params[n].numel()] = True
    lr, wd = muon_kw['muon_lr'], muon_kw['muon_weight_decay']
    worst = 0.
    for step, g in enumerate(grads):
        for m_ in (mb, mc):
            m_.store.grad.copy_(g)
        for n, r in zip(names, ref):
            o, shape = ps.offsets[n]
            r.grad = g[o:o + r.numel()].view(shape).clone()
        before_a = [r.detach().clone() for r in ref]
        before_b = ps.flat.clone()
        torch.nn.utils.clip_grad_norm_(ref, 0.5)
        t_muon.step(); t_adam.step()
        ob.step(); oc.step()
        torch.cuda.synchronize()
        # everything that is not a Muon matrix: bit-identical to FusedAdam, and torch Adam's result to fp32 rounding
        assert torch.equal(ps.flat[~mask], mc.store.flat[~mask]), f'step {step}: non-Muon elements differ from FusedAdam.step()'
        assert torch.equal(ob.v[~mask], oc.v[~mask]) and torch.equal(ob.m[~mask], oc.m[~mask])
        assert float(ob.v[mask].abs().max()) == 0., 'Adam touched a Muon range'
        for n, r, m in zip(names, ref, is_muon):
            if not m:
                assert torch.allclose(r.detach(), ps.params[n].detach(), rtol=1e-5, atol=1e-6), (step, n)
        for n, r, m, pa0 in zip(names, ref, is_muon, before_a):
            if not m:
                continue
            p = ps.params[n]
            o, shape = ps.offsets[n]
            buf_t = t_muon.state[r]['momentum_buffer']
            eb = rel(ob.momentum_buffer(p), buf_t)
            assert eb <= 1e-6, f'step {step} {n}: momentum buffer rel {eb}'
            # the fp64 update from torch's momentum and the clipped gradient torch used
            gt = r.grad.double()
            u = gt + muon_kw['momentum'] * (buf_t.double() - gt) if muon_kw['nesterov'] else buf_t.double()
            O = ns_fp64(u, steps=muon_kw['ns_steps'])
            adj = torch.optim._muon._adjust_lr(lr, muon_kw['adjust_lr_fn'], torch.Size(shape))      # torch's own factor, not the code under test's
            pb0 = before_b[o:o + p.numel()].view(shape)
            d_ref_a = -lr * wd * pa0.double() - adj * O
            d_ref_b = -lr * wd * pb0.double() - adj * O
            en, et = rel(p.detach().double() - pb0.double(), d_ref_b), rel(r.detach().double() - pa0.double(), d_ref_a)
            worst = max(worst, en / et)
            print(f'  step {step} {n} {tuple(shape)}: delta native vs fp64 {en:.3e}, torch vs fp64 {et:.3e}, ratio {en / et:.3f}')
            assert en <= MARGIN * et, f'step {step} {n}: native {en} > {MARGIN} x torch {et}'
    print(f'  {name} {kw}: worst weight-delta deviation ratio native / torch {worst:.3f}')


# ---------------------------------------------------------------------------------------------------------------- launches per step
class _CountingLib:
    """proxy of the loaded library that counts the calls of every entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_entry_point_calls_of_a_step_do_not_depend_on_depth(monkeypatch):
    """the calls one `step()` really makes, counted at the library boundary, at depth 2 and depth 6: the same, one launch per entry-point call (two
    for tfx_sumsq_det), and what `launches_per_step()` reports"""
    from transfusion_pytorch_amd import Transfusion
    from transfusion_pytorch_amd.optim import FusedMuon
    counts = {}
    for depth in (2, 6):
        torch.manual_seed(0)
        model = Transfusion(num_text_tokens=64, dim_latent=16, transformer=dict(dim=128, depth=depth, dim_head=64, heads=2)).cuda().train()
        opt = FusedMuon(model, lr=3e-4, max_grad_norm=0.5)
        model.store.grad.normal_(generator=torch.Generator(device=DEV).manual_seed(depth))
        opt.step()                                                # builds the tables, allocates the state
        proxy = _CountingLib(capi.lib())
        with monkeypatch.context() as mp:
            mp.setattr(capi, 'lib', lambda proxy=proxy: proxy)
            opt.step()
        torch.cuda.synchronize()
        counts[depth] = proxy.calls
        launches = sum(n * (2 if name == 'tfx_sumsq_det' else 1) for name, n in proxy.calls.items())
        print(f'  depth {depth}: {len(opt.muon_params)} matrices, calls {proxy.calls}, launches {launches}')
        assert launches == opt.launches_per_step() == 21
    assert counts[2] == counts[6] == dict(tfx_sumsq_det=1, tfx_muon_prep=1, tfx_muon_norm=1, tfx_muon_gemm=15, tfx_muon_apply=1, tfx_adam_step=1)


# ---------------------------------------------------------------------------------------------------------------- 4. determinism
def test_two_instances_are_bit_identical():
    from transfusion_pytorch_amd.optim import FusedMuon
    grads = record_gradients('small2')
    models = [fresh_model('small2')[0] for _ in range(2)]
    opts = [FusedMuon(m, lr=3e-4, max_grad_norm=0.5) for m in models]
    for g in grads:
        for m, o in zip(models, opts):
            m.store.grad.copy_(g)
            o.step()
    torch.cuda.synchronize()
    assert torch.equal(models[0].store.flat, models[1].store.flat)
    assert torch.equal(opts[0].m, opts[1].m) and torch.equal(opts[0].v, opts[1].v)
    for p0, p1 in zip(models[0].muon_parameters(), models[1].muon_parameters()):
        assert torch.equal(opts[0].momentum_buffer(p0), opts[1].momentum_buffer(p1))
    assert not torch.equal(models[0].store.flat, fresh_model('small2')[0].store.flat)


# ---------------------------------------------------------------------------------------------------------------- adam skip table
def test_adam_skip_table_null_empty_and_ranges():
    """tfx_adam_step on identical p, g, m, v: a NULL skip table and a table of zero ranges give the same bits, and torch Adam's values; a real table
    (ranges are whole groups of the kernel's 4 elements per thread: tfx.h) leaves exactly its ranges untouched and every other element as without it"""
    n = 100_003
    g_ = torch.Generator(device=DEV).manual_seed(2)
    p0, g = torch.randn(n + 1, device=DEV, generator=g_)[:n], torch.randn(n + 1, device=DEV, generator=g_)[:n] * 0.1
    m0, v0 = torch.randn(n + 1, device=DEV, generator=g_)[:n] * 0.01, torch.rand(n + 1, device=DEV, generator=g_)[:n] * 1e-3
    sumsq = (g.double() ** 2).sum().float().reshape(1)

    def run(skip, nskip):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        a = capi.make_args('tfx_adam_args', p=p, g=g, m=m, v=v, n=n, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0., max_norm=0.5,
                           grad_scale=1., step=3, sumsq=sumsq, skip=skip, nskip=nskip)
        capi.call('tfx_adam_step', a, stream())
        torch.cuda.synchronize()
        return p, m, v
    base = run(None, 0)
    empty = run(torch.zeros(2, dtype=torch.int64, device=DEV), 0)
    for a, b in zip(base, empty):
        assert torch.equal(a, b)
    # torch Adam at step 3 from the same moments
    rp = p0.clone().requires_grad_(True)
    rp.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([rp], 0.5)
    opt = torch.optim.Adam([rp], lr=3e-4)
    opt.state[rp] = dict(step=torch.tensor(2.), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    opt.step()
    assert torch.allclose(rp.detach(), base[0], rtol=1e-5, atol=1e-6)
    ranges = [(0, 8), (8, 12), (1000, 1004), (4096, 8192), (50_000, 50_008), (99_996, 100_000)]
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for a, b in ranges:
        mask[a:b] = True
    got = run(torch.tensor(ranges, dtype=torch.int64, device=DEV).reshape(-1), len(ranges))
    for t, t0, tb in zip(got, (p0, m0, v0), base):
        assert torch.equal(t[mask], t0[mask]), 'a skipped element changed'
        diff = (t != tb) & ~mask
        print(f'  elements outside the table that differ from the run without a table: {int(diff.sum())}')
        assert not bool(diff.any()), f'elements outside the table differ from the run without a table, first at {diff.nonzero()[:8].flatten().tolist()}'


# ---------------------------------------------------------------------------------------------------------------- 5. plumbing
def test_weights_reach_the_next_forward_and_load_state_dict_restores():
    from transfusion_pytorch_amd.optim import FusedMuon
    cfg, sd, batch, times, noise = build_case('small2')
    model = build_native(cfg, sd)
    model.train()
    model._noise_override = {t: v.cuda() for t, v in noise.items()}
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    loss0 = model(batch, times=times)
    loss0.backward()
    opt = FusedMuon(model, lr=3e-3, muon_lr=2e-2, max_grad_norm=0.5)
    opt.step(); opt.zero_grad()
    with torch.no_grad():
        loss1 = float(model(batch, times=times))
    print(f'  loss {float(loss0):.6f} -> {loss1:.6f}')
    assert abs(loss1 - float(loss0)) > 1e-4 * abs(float(loss0)), 'the step did not reach the forward'
    model.load_state_dict(saved)
    with torch.no_grad():
        loss2 = float(model(batch, times=times))
    assert abs(loss2 - float(loss0)) <= 1e-6 * max(1., abs(float(loss0))), (loss2, float(loss0))


def test_image_example_with_muon_trains():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import image_flow_unet as ex
    losses, images = ex.main(steps=60, log=lambda *a: None, muon=True)
    assert all(l == l for l in losses)
    assert falling(losses)
    assert images.shape == (4, 1, 28, 28)


def test_no_sync_accumulation_feeds_the_step():
    """two micro-batch backwards under no_sync(), then the accumulated buffer and the optimizer state copied into a second instance: both steps give
    the same bits (the optimizer consumes whatever the buffer holds; the backward's own summation order is not under test)"""
    from transfusion_pytorch_amd.optim import FusedMuon
    m1, batch = fresh_model('small2')
    o1 = FusedMuon(m1, lr=3e-4, max_grad_norm=0.5)
    m1(batch).backward()
    o1.step(); o1.zero_grad(set_to_none=False)
    with o1.no_sync():
        m1(batch).backward()
    m1(batch).backward()
    torch.cuda.synchronize()
    m2, _ = fresh_model('small2')
    m2.load_state_dict(m1.state_dict())
    m2 = m2.cuda()
    o2 = FusedMuon(m2, lr=3e-4, max_grad_norm=0.5)
    assert torch.equal(m1.store.flat, m2.store.flat)
    m2.store.grad.copy_(m1.store.grad)
    o2.m, o2.v, o2.step_count = o1.m.clone(), o1.v.clone(), o1.step_count
    o2.sumsq = torch.zeros(1, device=DEV)
    single = m1.store.grad.clone()
    o1.step(); o2.step()
    torch.cuda.synchronize()
    assert torch.equal(m1.store.flat, m2.store.flat) and torch.equal(o1.m, o2.m) and torch.equal(o1.v, o2.v)
    assert float(single.abs().sum()) > 0
