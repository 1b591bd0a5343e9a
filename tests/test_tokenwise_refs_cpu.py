"""The token-wise checker of tests/_tokenwise_cases.py on the CPU: an fp32 emulation of a CORRECT kernel, in two summation orders (left to right, and the
lane layout with its 64-lane tree), has no element over its bound for every operation - so the bounds are not too tight - and every fault of the list is caught
by the per-element check or the guard bands.  Next to each fault the whole-tensor Frobenius ratio of the first-round tests (tests/test_kernels_gpu.py) is
computed at its old tolerance: it misses a neighbour's row statistic and a double rounding, which is why the per-element tests exist."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tokenwise_cases as C  # noqa: E402

ORDERS = ('linear', 'tree')
# the tolerances of the first-round tests for the outputs the faults land in
OLD_TOL = {'u': 6e-3, 'out': 6e-3, 'dx': 1.5e-2, 'dtable[gamma|beta]': 5e-3, 'dgamma_text': 5e-3, 'dy': 6e-3, 'dtable[z]': 5e-3, 'save': 1e-4, 'dqkv': 1.2e-2,
           'dgamma_q': 1e-2, 'dgamma_k': 1e-2, 'dlayerscale': 5e-3, 'dbias': 1e-5, 'mean': 0., 'rstd': 0.}


def _pre_case(T, d, kind='scatter', **kw):
    return C.build_adaln(C.layout(kind, T), d, **kw)


@pytest.mark.parametrize('order', ORDERS)
def test_emulated_adaln_is_under_its_bounds(order):
    rep = {}
    shapes = [(1001, 520, 'scatter', {}), (1001, 512, 'runs', {}), (4101, 64, 'scatter', {}), (130, 2048, 'runs', {}), (37, 8, 'scatter', {}),
              (130, 1032, 'runs', dict(eps_rows=True)), (0, 64, 'model', dict(wrappers=2)), (0, 520, 'all_text', {}), (0, 64, 'all_mod', {}), (0, 8, 'one_seg', {})]
    for T, d, kind, kw in shapes:
        c = _pre_case(T, d, kind, **kw)
        label = f'adaln {kind} T={c.T} d={d} {order}'
        o = C.outs_pre_fwd(c); C.emulate_pre_fwd(c, o, order)
        C.check_outs(label + ' pre fwd', [o.u, o.mean, o.rstd], rep.setdefault('pre fwd', {}))
        for stored in ((False, True) if kind != 'scatter' else (False,)):
            for use_add in (False, True):
                o = C.outs_pre_bwd(c, stored, use_add); C.emulate_pre_bwd(c, o, order, stored, use_add)
                C.check_outs(f'{label} pre bwd stored={stored} add={use_add}', [o.dx, o.dtable, o.dgamma_text], rep.setdefault('pre bwd', {}))
            o = C.outs_post_bwd(c, stored); C.emulate_post_bwd(c, o, order, stored)
            C.check_outs(f'{label} post bwd stored={stored}', [o.dy, o.dtable, o.dlayerscale, o.dbias], rep.setdefault('post bwd', {}))
        o = C.outs_post_fwd(c); C.emulate_post_fwd(c, o, order)
        C.check_outs(label + ' post fwd', [o.out], rep.setdefault('post fwd', {}))
    print(f'adaln emulation ({order}): worst error / bound ' + '; '.join(f'{k}: ' + ', '.join(f'{n} {v:.3f}' for n, v in r.items()) for k, r in rep.items()))
    assert all(0 < v <= 1 for r in rep.values() for v in r.values())


@pytest.mark.parametrize('order', ORDERS)
def test_emulated_rmsnorm_attnres_qk_embed_are_under_their_bounds(order):
    rep = {}
    for T, d, zr in ((1001, 520, False), (130, 2048, True), (37, 8, True), (4101, 64, False), (130, 1032, False)):
        c = C.build_rmsnorm(T, d, zero_row=zr)
        o = C.outs_rmsnorm(c); C.emulate_rmsnorm(c, o, order)
        C.check_outs(f'rmsnorm T={T} d={d} {order}', [o.y, o.dx, o.dgamma], rep.setdefault('rmsnorm', {}))
    for T, d, L, zr in ((130, 520, 5, False), (37, 1032, 33, True), (19, 64, 64, False), (130, 8, 1, False), (1001, 64, 2, True)):
        c = C.build_attnres(T, d, L, zero_row=zr)
        o = C.outs_attnres_fwd(c); C.emulate_attnres_fwd(c, o, order)
        C.check_attnres_fwd(f'attnres fwd T={T} d={d} L={L} {order}', c, o, rep.setdefault('attnres fwd', {}))
        for first in (0, 1):
            o = C.outs_attnres_bwd(c, first); C.emulate_attnres_bwd(c, o, order, first)
            C.check_outs(f'attnres bwd T={T} d={d} L={L} first={first} {order}', [o.dhiddens, o.dgamma, o.dpq], rep.setdefault('attnres bwd', {}))
    for T, H in ((130, 2), (5500, 3), (700, 12)):
        c = C.build_qk(T, H)
        o = C.outs_qk(c); C.emulate_qk(c, o, order)
        C.check_outs(f'qk T={T} H={H} {order}', [o.qk, o.dqkv, o.dgamma_q, o.dgamma_k], rep.setdefault('qk_norm_rope', {}))
    for kind, T, d in (('scatter', 1001, 520), ('runs', 130, 8), ('all_mod', 0, 64)):
        c = C.build_embed(C.layout(kind, T), d, 40)
        o = C.outs_embed(c); C.emulate_embed(c, o, order)
        C.check_outs(f'embed {kind} d={d} {order}', [o.x, o.dtable], rep.setdefault('embed', {}))
    print(f'emulation ({order}): worst error / bound ' + '; '.join(f'{k}: ' + ', '.join(f'{n} {v:.3f}' for n, v in r.items()) for k, r in rep.items()))
    assert all(v <= 1 for r in rep.values() for v in r.values())
    assert all(0 < r[n] for k, r in rep.items() for n in r if not (k == 'embed' and n == 'x'))


def test_segment_layouts_hold_what_the_model_makes():
    """every length 1 - 9 as a modality instance and as a text run, one instance of 1030 tokens, starts that are not monotone with balance=True"""
    for balance in (False, True):
        lay = C.layout('model', balance=balance)
        tok = lay.tok.reshape(-1)
        mod = {int(n) for s, n in zip(lay.seg_start, lay.seg_len) if tok[s] >= 0}
        text = {int(n) for s, n in zip(lay.seg_start, lay.seg_len) if tok[s] < 0}
        assert mod == set(range(1, 10)) | {1030} and text == set(range(1, 10))
        assert bool((lay.seg_start[1:] < lay.seg_start[:-1]).any()) == balance
    assert C.layout('one_seg').n_seg == 1


def _run_fault(fault):
    """(outputs of the faulty emulation, the outputs the old tests would have looked at)"""
    if fault in C.PRE_FAULTS:
        T, d, kind, kw = {'row_stats_from_neighbour': (1001, 520, 'scatter', {}), 'double_round': (1001, 512, 'scatter', {}),
                          'last_chunk_out_of_stats': (1001, 520, 'scatter', {}), 'eps_dropped': (130, 64, 'scatter', dict(eps_rows=True)),
                          'last_token_unwritten': (1001, 64, 'scatter', {}), 'beta_on_text_row': (1001, 64, 'scatter', {})}[fault]
        c = _pre_case(T, d, kind, **kw)
        o = C.outs_pre_fwd(c); C.emulate_pre_fwd(c, o, 'tree', fault)
        return [o.u, o.mean, o.rstd]
    if fault in ('segment_tail_token_twice', 'segment_added_not_stored', 'table_pad_written'):
        c = C.build_adaln(C.layout('model', balance=True), 64)
        o = C.outs_pre_bwd(c, True); C.emulate_pre_bwd(c, o, 'tree', True, fault=fault)
        return [o.dx, o.dtable, o.dgamma_text]
    if fault == 'second_trip_skipped':
        c = _pre_case(4101, 64)
        o = C.outs_post_bwd(c, False); C.emulate_post_bwd(c, o, 'tree', False, fault=fault)
        return [o.dy, o.dtable, o.dlayerscale, o.dbias]
    if fault == 'rope_carry_off_by_one':
        assert C.rope_carries(5500, 3)
        c = C.build_qk(5500, 3)
        o = C.outs_qk(c); C.emulate_qk(c, o, 'tree', fault)
        return [o.dqkv, o.dgamma_q, o.dgamma_k]
    if fault == 'save_lane_ge_32_dropped':
        c = C.build_attnres(37, 64, 33)
        o = C.outs_attnres_fwd(c); C.emulate_attnres_fwd(c, o, 'tree', fault)
        return [o.out, o.save]
    raise KeyError(fault)


# what the old whole-tensor ratio does with each fault at these shapes (measured here; the two the issue names are the point of the new suite)
OLD_MEASURE_MISSES = {'row_stats_from_neighbour': True, 'double_round': True, 'eps_dropped': False, 'last_token_unwritten': False,
                      'last_chunk_out_of_stats': False, 'beta_on_text_row': False, 'segment_tail_token_twice': False, 'segment_added_not_stored': False,
                      'second_trip_skipped': False, 'table_pad_written': True, 'rope_carry_off_by_one': False, 'save_lane_ge_32_dropped': False}


@pytest.mark.parametrize('fault', C.FAULTS)
def test_fault_is_caught_per_element(fault):
    outs = _run_fault(fault)
    old = {o.name: C.old_ratio(o) for o in outs}
    missed = all(r <= OLD_TOL[n] or OLD_TOL[n] == 0. for n, r in old.items())
    print(f'{fault}: old whole-tensor ratios ' + ', '.join(f'{n} {r:.3e} (tolerance {OLD_TOL[n]:g})' for n, r in old.items() if OLD_TOL[n]) +
          f' -> the old measure {"MISSES" if missed else "sees"} it')
    assert missed == OLD_MEASURE_MISSES[fault]
    with pytest.raises(AssertionError) as ei:
        for o in outs:
            C.check_out(fault, o)
    print(ei.value)
    assert ('outside the product' in str(ei.value)) == (fault == 'table_pad_written')


def test_fault_list_is_the_issue_s():
    assert set(C.FAULTS) == set(OLD_MEASURE_MISSES) and len(C.FAULTS) == 12
