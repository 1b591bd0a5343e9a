"""tfx_sample_tokens_filtered (top-k / top-p / min-p on the device) against the fp64 `filter_reference` of tests/_sampler_filter_cases.py (pinned on the
CPU by tests/test_sampler_filters_cpu.py), cell by cell; "filters off" against tfx_sample_tokens_range bit for bit; the edges; and the keyword
arguments of the four sampling routes end to end on a random-weight model.

The id buffer of every launch sits between guard bands of sentinels and starts at -7; pad columns of the logits hold 1e9 and must never win."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from _decode_loss_cases import F64, SAMPLE_MODES, SAMPLE_SEEDS, SAMPLE_SHAPES, min_p_margin, sample_logits, u_for  # noqa: E402
from _sampler_filter_cases import (FILTER_MODES, FILTER_SEEDS, FILTER_SHAPES, MIN_P_MARGIN, NUCLEUS_MARGIN, TIE_ROWS, TOP_K_MARGIN, aim_targets,  # noqa: E402
                                   case, filter_reference, nucleus_margin, top_k_margin)
from transfusion_pytorch_amd import Transfusion, capi  # noqa: E402

DEV = 'cuda'
U_TOP = 1. - 2. ** -24                                       # the largest fp32 below 1
SENTINEL = -7
N_SWEEP = 257


def sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(entry, lg, ld, B, V, Vd, T, mp, k, p, u, active=None, want_rc=0):
    """one launch of `entry` ('filtered' or 'range'); returns the ids (CPU, long) of a guarded buffer that starts at SENTINEL"""
    g = 64
    full = torch.full((B + 2 * g,), SENTINEL, dtype=torch.int32, device=DEV)
    out = full[g:g + B]
    L = capi.lib()
    if entry == 'filtered':
        rc = L.tfx_sample_tokens_filtered(lg.data_ptr(), ld, B, V, Vd, T, mp, k, p, ptr(u), ptr(active), out.data_ptr(), sp())
    else:
        rc = L.tfx_sample_tokens_range(lg.data_ptr(), ld, B, V, Vd, T, mp, ptr(u), ptr(active), out.data_ptr(), sp())
    assert rc == want_rc, (entry, rc)
    host = full.cpu().long()
    assert bool((host[:g] == SENTINEL).all()) and bool((host[g + B:] == SENTINEL).all()), 'the id buffer\'s guard bands'
    return host[g:g + B]


def modes_of(shape):
    return [(m, FILTER_SEEDS[shape][i]) for i, m in enumerate(FILTER_MODES) if FILTER_SEEDS[shape][i] is not None]


def assert_margins(lg, V, Vd, T, mp, k, p):
    assert nucleus_margin(lg, V, Vd, T, k, p) >= NUCLEUS_MARGIN, 'no column may sit on the nucleus boundary'
    assert min_p_margin(lg, V, T, mp) >= MIN_P_MARGIN, 'no column may sit on the min-p threshold'
    assert top_k_margin(lg, Vd, k) >= TOP_K_MARGIN


# ---------------------------------------------------------------------------------------------- 1. aimed draws
@pytest.mark.parametrize('shape', FILTER_SHAPES, ids=str)
def test_every_aimed_cell_is_hit_exactly(shape):
    """u in the middle of a survivor's cell of the inverse CDF over the surviving set must return that survivor: the first, the last, the one behind the
    longest run of filtered columns, the ones nearest the 64-column trip boundary, and the heaviest - cells of >= 1e-3 of the surviving mass"""
    B, V, Vd, ld = shape
    for (T, mp, k, p), seed in modes_of(shape):
        lg, keep, q = case(shape, (T, mp, k, p), seed)
        assert_margins(lg, V, Vd, T, mp, k, p)
        assert bool(keep.any(-1).all())
        tg = aim_targets(keep, q)
        for r in range(B):
            assert len(tg[r]) >= 1, (r, tg[r])
        dlg = lg.to(DEV)
        for rnd in range(max(len(t) for t in tg)):
            want = torch.tensor([t[rnd % len(t)] for t in tg])
            got = launch('filtered', dlg, ld, B, V, Vd, T, mp, k, p, u_for(q, want).to(DEV))
            assert torch.equal(got, want), ((T, mp, k, p), got.tolist(), want.tolist())


# ---------------------------------------------------------------------------------------------- 2. sweep
def sweep_rows(keep, q):
    """per row of a table entry: (row, fp64 inverse-CDF picks of the N_SWEEP uniforms, mask of the uniforms at least 1e-4 of the mass away from every
    cell edge).  The sweep takes the first two rows whose mask excuses at most 10 % - a property of the inputs alone, known before any launch (of the
    table only the all-columns mode of the 4100-column shape, whose 4100 cells crowd the edges, has fewer than two such rows: it has one)."""
    u = ((torch.arange(N_SWEEP, dtype=F64) + 0.5) / N_SWEEP).to(torch.float32)
    out = []
    for r in range(keep.shape[0]):
        cdf = q[r].cumsum(-1)
        target = u.to(F64) * cdf[-1]
        idx = keep[r].nonzero().flatten()
        edges = cdf[idx]
        pick = idx[torch.searchsorted(edges, target, right=True).clamp(max=idx.numel() - 1)]
        dist = (target[:, None] - torch.cat([torch.zeros(1, dtype=F64), edges])[None]).abs().min(-1).values / cdf[-1]
        firm = dist >= 1e-4
        if int((~firm).sum()) <= N_SWEEP // 10:
            out.append((r, pick, firm))
    return u, out[:2]


@pytest.mark.parametrize('shape', FILTER_SHAPES, ids=str)
def test_sweep_of_uniforms_follows_the_fp64_inverse_cdf(shape):
    """a row replicated into 257 launch rows with u = (i + 0.5) / 257: every pick is a survivor, and equals the fp64 inverse CDF wherever u is at least
    1e-4 of the mass away from a cell edge (at most 10 % of the 257 are excused, asserted); u = 0 gives the first survivor, the largest fp32 below 1 a
    survivor."""
    B, V, Vd, ld = shape
    for (T, mp, k, p), seed in modes_of(shape):
        lg, keep, q = case(shape, (T, mp, k, p), seed)
        assert_margins(lg, V, Vd, T, mp, k, p)
        u, rows = sweep_rows(keep, q)
        assert len(rows) >= min(2, B) or (V == 4100 and k >= V and len(rows) >= 1), (T, mp, k, p)
        for r, pick, firm in rows:
            dlg = lg[r:r + 1].expand(N_SWEEP, ld).contiguous().to(DEV)
            got = launch('filtered', dlg, ld, N_SWEEP, V, Vd, T, mp, k, p, u.to(DEV))
            assert bool(((got >= 0) & (got < Vd)).all()) and bool(keep[r][got.clamp(0, Vd - 1)].all()), ((T, mp, k, p), r, 'a pick outside the surviving set')
            excused = int((~firm).sum())
            print(f'sweep {shape} {(T, mp, k, p)} row {r}: {int(keep[r].sum())} survivors, {excused} of {N_SWEEP} excused, '
                  f'{int((got != pick).sum())} differ from the fp64 inverse CDF')
            assert excused <= N_SWEEP // 10
            assert torch.equal(got[firm], pick[firm]), ((T, mp, k, p), r, (got != pick).nonzero().flatten().tolist())
            edge = launch('filtered', dlg[:2].contiguous(), ld, 2, V, Vd, T, mp, k, p, torch.tensor([0., U_TOP], device=DEV))
            assert int(edge[0]) == int(keep[r].nonzero()[0]) and 0 <= int(edge[1]) < Vd and bool(keep[r][int(edge[1])])


# ---------------------------------------------------------------------------------------------- 3. off is the old kernel
@pytest.mark.parametrize('B,V,Vd,ld', SAMPLE_SHAPES)
def test_filters_off_equals_the_range_entry_bit_for_bit(B, V, Vd, ld):
    g = torch.Generator().manual_seed(5)
    for n, seed in zip((B, 64), SAMPLE_SEEDS[(B, V, Vd, ld)]):
        dlg = sample_logits(n, V, Vd, ld, seed).to(DEV)
        for T, mp in SAMPLE_MODES:
            for u in (torch.rand(n, generator=g), torch.zeros(n), torch.full((n,), U_TOP)):
                old = launch('range', dlg, ld, n, V, Vd, T, mp, 0, 1., u.to(DEV))
                for k, p in ((0, 1.), (0, 2.)):
                    new = launch('filtered', dlg, ld, n, V, Vd, T, mp, k, p, u.to(DEV))
                    assert torch.equal(new, old), (T, mp, k, p)


# ---------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize('shape', [(5, 390, 256, 392), (9, 392, 390, 392), (3, 4100, 4100, 4104), (2, 1025, 1000, 1032)], ids=str)
def test_active_mask_greedy_and_top_1(shape):
    B, V, Vd, ld = shape
    lg = sample_logits(B, V, Vd, ld, 0)
    dlg = lg.to(DEV)
    T, mp, k, p = 0.7, 0., 40, 0.5
    assert_margins(lg, V, Vd, T, mp, k, p)
    keep, q = filter_reference(lg, V, Vd, T, k, p, mp)
    first = keep.int().argmax(-1)
    act = torch.tensor([r % 2 == 0 for r in range(B)])
    got = launch('filtered', dlg, ld, B, V, Vd, T, mp, k, p, torch.zeros(B, device=DEV), act.to(DEV, torch.int32))
    assert torch.equal(got, torch.where(act, first, torch.full_like(first, SENTINEL))), 'rows with active == 0 keep their value'
    amax = torch.tensor([int((row == row.max()).nonzero()[0]) for row in lg[:, :V]])
    for k, p in ((0, 1.), (3, 0.5), (1, 1e-6)):
        got = launch('filtered', dlg, ld, B, V, Vd, 0., 0.1, k, p, None)
        assert torch.equal(got, amax), 'temperature 0: the argmax over all V columns, whatever the filters'
    best = lg[:, :Vd].argmax(-1)
    assert all(int((lg[r, :Vd] == lg[r, best[r]]).sum()) == 1 for r in range(B))
    for uval in (0., 0.5, U_TOP):
        got = launch('filtered', dlg, ld, B, V, Vd, 1., 0., 1, 1., torch.full((B,), uval, device=DEV))
        assert torch.equal(got, best), 'top_k = 1: the best candidate for any u'


@pytest.mark.parametrize('shape', [s for s in FILTER_SHAPES if s[2] < s[1]], ids=str)
def test_without_a_survivor_the_result_is_v_draw(shape):
    """the global maximum lies outside the draw range and min-p removes every candidate, with top-k and top-p on"""
    B, V, Vd, ld = shape
    for T, mp, k, p in ((1.0, 0.1, 20, 0.9), (0.7, 0.3, 3, 0.95), (1.0, 0.1, 0, 0.5)):
        lg = sample_logits(B, V, Vd, ld, 0)
        lg[:, V - 1] = lg[:, :Vd].amax(-1) + 2. * (-T * math.log(mp))
        keep, _ = filter_reference(lg, V, Vd, T, k, p, mp)
        assert not bool(keep.any())
        u = torch.tensor([(0., 0.5, U_TOP)[r % 3] for r in range(B)])
        got = launch('filtered', lg.to(DEV), ld, B, V, Vd, T, mp, k, p, u.to(DEV))
        assert bool((got == Vd).all()), ((T, mp, k, p), got.tolist())


def test_bad_arguments_return_minus_3_and_write_nothing():
    B, V, Vd, ld = 5, 390, 256, 392
    dlg = sample_logits(B, V, Vd, ld, 0).to(DEV)
    u = torch.full((B,), 0.5, device=DEV)
    ok = dict(V=V, Vd=Vd, T=1., k=5, p=0.9)
    for bad in (dict(T=-1.), dict(k=-1), dict(p=0.), dict(p=-1.), dict(p=math.nan), dict(Vd=0), dict(Vd=V + 1)):
        a = {**ok, **bad}
        got = launch('filtered', dlg, ld, B, a['V'], a['Vd'], a['T'], 0.1, a['k'], a['p'], u, want_rc=-3)
        assert bool((got == SENTINEL).all()), bad


def test_tie_rows():
    for logits, T, k, p, kept in TIE_ROWS:
        V = len(logits)
        lg = torch.full((1, V + 3), 1e9)
        lg[0, :V] = torch.tensor(logits)
        keep, q = filter_reference(lg, V, V, T, k, p, 0.)
        assert keep[0].nonzero().flatten().tolist() == kept
        n = 64
        u = ((torch.arange(n, dtype=F64) + 0.5) / n).to(torch.float32)
        dlg = lg.expand(n, V + 3).contiguous().to(DEV)
        got = launch('filtered', dlg, V + 3, n, V, V, T, 0., k, p, u.to(DEV))
        assert sorted(set(got.tolist())) == kept, 'ties at the k-th place and at the nucleus boundary all survive, nothing else does'
        cdf = q[0].cumsum(-1)
        assert torch.equal(got, torch.searchsorted(cdf, u.to(F64) * cdf[-1], right=True))      # (no u of the 64 lies on a cell edge of these rows)


# ---------------------------------------------------------------------------------------------- 5. end to end
VOCAB_TEXT = 256


@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    m = Transfusion(num_text_tokens=VOCAB_TEXT, dim_latent=16, modality_default_shape=(4,), transformer=dict(dim=128, depth=2, dim_head=64, heads=2))
    return m.cuda().eval()


def gen(m, seed=3, **kw):
    torch.manual_seed(1)
    prompt = torch.randint(0, VOCAB_TEXT, (2, 7), device=DEV)
    torch.manual_seed(seed)
    return m.generate_text_only(prompt, 7 + 24, **kw).cpu()


def many(m, seed=3, **kw):
    torch.manual_seed(1)
    prompts = [torch.randint(0, VOCAB_TEXT, (n,), device=DEV) for n in (5, 9)]
    noise = torch.randn(16, 16, device=DEV)
    torch.manual_seed(seed)
    out = m.sample_many(prompts, max_length=24, init_modality_noise=noise, modality_steps=2, fixed_modality_shape=(4,), cfg_scale=1.,
                        return_unprocessed_modalities=True, **kw)
    return [[(p[0], p[1].cpu()) if isinstance(p, tuple) else p.cpu() for p in s] for s in out]


def same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all((isinstance(p, tuple) and isinstance(o, tuple) and p[0] == o[0] and torch.equal(p[1], o[1]))
                                                             or (not isinstance(p, tuple) and not isinstance(o, tuple) and torch.equal(p, o))
                                                             for p, o in zip(x, y)) for x, y in zip(a, b))


def test_off_values_change_nothing_end_to_end(model):
    base = gen(model)
    assert base.shape == (2, 24)
    for kw in (dict(top_k=None, top_p=None), dict(top_k=0, top_p=1.0), dict(top_k=model.md.vocab)):
        assert torch.equal(gen(model, **kw), base), kw
    assert not torch.equal(gen(model, seed=4), base), 'the draw follows the seed'
    base = many(model)
    for kw in (dict(text_top_k=None, text_top_p=None), dict(text_top_k=0, text_top_p=1.0), dict(text_top_k=model.md.vocab)):
        assert same(many(model, **kw), base), kw


def test_top_k_1_and_a_tiny_top_p_keep_the_best_candidate_alone(model):
    a, b = gen(model, top_k=1), gen(model, top_p=1e-6)
    assert torch.equal(a, b) and not torch.equal(a, gen(model))
    assert torch.equal(a, gen(model, seed=11, top_k=1)), 'one candidate: the uniforms do not matter'
    assert bool((a < VOCAB_TEXT).all())
    assert same(many(model, text_top_k=1), many(model, text_top_p=1e-6))


def test_top_k_1_at_a_temperature_is_greedy_in_sample_many(model):
    assert same(many(model, text_top_k=1, text_temperature=1.), many(model, text_temperature=0.))


def test_uncached_loop_honours_the_filters(model):
    """`sample_one(cache_kv=False, text_top_k=1)` (the loop over forward()) against the KV-cached decoder with the same arguments, by the rule of
    tests/test_decode_contract_gpu.py: the text in front of the first decoded modality is identical up to the first divergence, which must sit on a
    near-tie (top-2 margin < 0.05) of the un-cached full forward over the agreed history"""
    torch.manual_seed(1)
    prompt = torch.randint(0, VOCAB_TEXT, (6,), device=DEV)
    noise = torch.randn(16, 16, device=DEV)
    kw = dict(max_length=20, text_temperature=1., text_top_k=1, init_modality_noise=noise, modality_steps=2, fixed_modality_shape=(4,), cfg_scale=1.,
              return_unprocessed_modalities=True)
    a = model.sample_one(prompt, cache_kv=False, **kw)
    c = model.sample_many([prompt], **kw)[0]
    assert not isinstance(a[0], tuple) and not isinstance(c[0], tuple)
    la, lc = a[0].tolist(), c[0].tolist()
    assert len(la) > 6 and len(lc) > 6
    k = next((i for i, (x, y) in enumerate(zip(la, lc)) if x != y), None)
    if k is None:
        assert len(la) == len(lc)
    else:
        with torch.no_grad():
            lg = model([[a[0][:k]]], return_loss=False)[0, -1]
        gap = float((lg[la[k]] - lg[lc[k]]).abs())
        print(f'divergence at {k}: tokens {la[k]} / {lc[k]}, margin {gap:.4f}')
        assert gap < 0.05, (k, la, lc, gap)
