"""The filtered text draw without a GPU: `filter_reference` (tests/_sampler_filter_cases.py, written from include/tfx.h) against an independent
restatement built the usual way, the case table against its margins, the argument validation, the keyword arguments of the five methods, and the C ABI
(export, version tag, host-side argument check)."""
import ctypes
import inspect
import math

import pytest
import torch

from _decode_loss_cases import F64, min_p_margin, sample_logits
from _sampler_filter_cases import (FILTER_MODES, FILTER_SEEDS, FILTER_SHAPES, MIN_P_MARGIN, NARROW_MAX, NUCLEUS_MARGIN, TIE_ROWS, TOP_K_MARGIN, case, cases,
                                   filter_reference, nucleus_margin, top_k_margin)
from transfusion_pytorch_amd import Transfusion, capi
from transfusion_pytorch_amd.transfusion import _check_text_filters

CASES = cases()
IDS = [f'{s}-{m}' for s, m, _ in CASES]


def usual_warpers(logits, V, V_draw, T, top_k, top_p, min_p):
    """the chain as samplers usually spell it, on fp64: temperature; torch.topk and "remove what is below the k-th value" over the text columns; a
    descending sort + cumsum and "remove where the mass strictly ahead >= top_p" over the renormalised top-k survivors; then min_p_filter as the
    reference spells it (T:591-595) over all V columns, those outside the draw range included.  Returns the boolean keep mask over [0, V_draw)."""
    l = logits[:, :V].to(F64) / T
    c = l[:, :V_draw]                                                                    # the candidates: the text-only mask comes first
    if 0 < top_k < V_draw:
        kth = torch.topk(c, top_k, dim=-1).values[:, -1:]
        c = torch.where(c < kth, float('-inf'), c)
    if top_p < 1.:
        sp, si = c.softmax(-1).sort(-1, descending=True)
        ahead = sp.cumsum(-1) - sp
        remove = torch.zeros_like(c, dtype=torch.bool).scatter(1, si, ahead >= top_p)
        c = torch.where(remove, float('-inf'), c)
    l = torch.cat([c, l[:, V_draw:]], -1)                                                # min_p_filter (T:591-595) over all V columns
    probs = l.softmax(-1)
    max_probs = probs.amax(-1, keepdim=True)
    limit = min_p * max_probs
    l = torch.where(probs < limit, float('-inf'), l)
    return torch.isfinite(l[:, :V_draw])


@pytest.mark.parametrize('shape,mode,seed', CASES, ids=IDS)
def test_filter_reference_equals_the_usual_warpers_on_tie_free_rows(shape, mode, seed):
    B, V, Vd, ld = shape
    T, mp, k, p = mode
    lg, keep, q = case(shape, mode, seed)
    want = usual_warpers(lg, V, Vd, T, k, p, mp)
    tie_free = [r for r in range(B) if lg[r, :Vd].unique().numel() == Vd]                # (a tied pair across the nucleus boundary is the one place the two differ)
    assert len(tie_free) >= (B + 1) // 2
    for r in tie_free:
        assert torch.equal(keep[r], want[r]), (r, (keep[r] != want[r]).nonzero().flatten().tolist())
    assert bool(((q > 0) == keep).all())
    if p < 1. or 0 < k < Vd:
        assert bool(keep.any(-1).all()) or mp > 0., 'top-k and top-p never empty a row'


def test_filter_reference_on_the_tie_rows():
    for logits, T, k, p, kept in TIE_ROWS:
        lg = torch.tensor([logits], dtype=torch.float32)
        V = lg.shape[1]
        keep, q = filter_reference(lg, V, V, T, k, p, 0.)
        assert keep[0].nonzero().flatten().tolist() == kept
    lg = torch.tensor([TIE_ROWS[1][0]], dtype=torch.float32)
    r = ((lg.to(F64) - lg.to(F64).amax()) / 1.).exp()[0]
    assert torch.allclose(r, torch.tensor([1., .5, .5, .25, .25], dtype=F64), atol=1e-6)


@pytest.mark.parametrize('shape,mode,seed', CASES, ids=IDS)
def test_every_table_entry_meets_its_margins(shape, mode, seed):
    B, V, Vd, ld = shape
    T, mp, k, p = mode
    lg = case(shape, mode, seed)[0]
    assert nucleus_margin(lg, V, Vd, T, k, p) >= NUCLEUS_MARGIN
    assert min_p_margin(lg, V, T, mp) >= MIN_P_MARGIN
    assert top_k_margin(lg, Vd, k) >= TOP_K_MARGIN
    for s in range(seed):                                                                # the FIRST such seed
        l2 = sample_logits(B, V, Vd, ld, s)
        assert not (nucleus_margin(l2, V, Vd, T, k, p) >= NUCLEUS_MARGIN and min_p_margin(l2, V, T, mp) >= MIN_P_MARGIN and top_k_margin(l2, Vd, k) >= TOP_K_MARGIN)


def test_the_table_covers_every_shape_and_both_width_classes():
    assert set(FILTER_SEEDS) == set(FILTER_SHAPES) and all(len(v) == len(FILTER_MODES) for v in FILTER_SEEDS.values())
    assert NARROW_MAX == capi.ENUMS['TFX_SAMPLE_NARROW_MAX']
    assert any(s[1] == NARROW_MAX for s in FILTER_SHAPES) and any(s[1] == NARROW_MAX + 1 for s in FILTER_SHAPES)
    for s in FILTER_SHAPES:
        modes = [m for i, m in enumerate(FILTER_MODES) if FILTER_SEEDS[s][i] is not None]
        assert any(m[2] > 0 and m[3] >= 1. for m in modes) and any(m[2] == 0 and m[3] < 1. for m in modes) and any(m[2] > 0 and m[3] < 1. for m in modes)


def test_validation_helper():
    assert _check_text_filters(None, None) == (None, None)
    assert _check_text_filters(0, 1) == (0, 1.) and _check_text_filters(40, 0.9) == (40, 0.9)
    assert _check_text_filters(10 ** 12, 1e-6) == (2 ** 31 - 1, 1e-6)
    for bad in (True, False, 1.5, '3'):
        with pytest.raises(TypeError):
            _check_text_filters(bad, None)
    with pytest.raises(ValueError):
        _check_text_filters(-1, None)
    for bad in (0, 0., -0.5, 1.0001, 2, math.nan, math.inf, '0.5', True):
        with pytest.raises(ValueError):
            _check_text_filters(None, bad)


def test_keyword_arguments_exist_with_none_defaults():
    for name, kws in (('sample_many', ('text_top_k', 'text_top_p')), ('sample_one', ('text_top_k', 'text_top_p')),
                      ('_sample_one_through_forward', ('text_top_k', 'text_top_p')), ('generate_text_only', ('top_k', 'top_p')), ('sample', ('text_top_k', 'text_top_p'))):
        params = inspect.signature(getattr(Transfusion, name)).parameters
        for kw in kws:
            assert kw in params and params[kw].default is None, (name, kw)
    names = list(inspect.signature(Transfusion.sample_many).parameters)                  # positional calls stay valid: the new ones come last
    assert names.index('text_top_k') > names.index('_pos_emb_in_decode')
    assert list(inspect.signature(Transfusion.generate_text_only).parameters)[:6] == ['self', 'prompt', 'seq_len', 'temperature', 'min_p', 'cache_kv']
    from transfusion_pytorch_amd import sampling
    for fn in (sampling._sample_text_token, sampling._pick_text_only):
        p = inspect.signature(fn).parameters
        assert p['top_k'].default is None and p['top_p'].default is None
    assert {'top_k', 'top_p'} <= set(sampling._Call.__dataclass_fields__)


def test_header_and_library_export_the_entry_and_the_version_tag():
    assert 'tfx_sample_tokens_filtered' in capi.FUNCTIONS
    ret, argt = capi.FUNCTIONS['tfx_sample_tokens_filtered']
    assert ret is ctypes.c_int and len(argt) == 13 and argt[7] is ctypes.c_int32 and argt[8] is ctypes.c_float
    L = capi.lib()
    assert hasattr(L, 'tfx_sample_tokens_filtered')
    v = L.tfx_version()
    assert v.startswith(b'tfx-hip gfx950') and b'-topkp' in v


def test_argument_check_answers_minus_3_before_any_launch():
    buf = (ctypes.c_float * 16)()
    ids = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    f, i = ctypes.addressof(buf), ctypes.addressof(ids)
    call = lambda V=8, Vd=8, T=1., k=0, p=1.: capi.lib().tfx_sample_tokens_filtered(f, 8, 1, V, Vd, T, 0.1, k, p, f, None, i, None)
    for kw in (dict(T=-1.), dict(k=-1), dict(p=0.), dict(p=-0.5), dict(p=math.nan), dict(Vd=0), dict(Vd=9), dict(V=4, Vd=8)):
        assert call(**kw) == -3, kw
    assert list(ids) == [-7] * 4
