"""The launch lists of real Plans, built on the CPU (tests/_plan_digest.py): every list of a fixed matrix of plans is, item for item and argument byte
for argument byte with addresses canonicalised, what tests/plan_digests.json records; and a launch list owns the argument structs it refers to, so a
backward list that `select_frozen` drops takes them along."""
import gc
import json
import weakref

import pytest
import torch

import _plan_digest as P

with open(P.JSON_PATH) as f:
    RECORDED = json.load(f)


def test_matrix_is_what_was_recorded():
    assert sorted(RECORDED) == sorted(P.CASES)


@pytest.mark.parametrize('name', list(P.CASES))
def test_lists_are_what_was_recorded(name):
    got, want = P.run_case(name), RECORDED[name]
    assert sorted(got) == sorted(want)                             # the stages of the case (the file keeps its keys sorted)
    for stage in want:
        g, w = got[stage], want[stage]
        for lst in P.LISTS:
            if g['lists'][lst] != w['lists'][lst]:
                # the entry-point names show WHERE two lists part; equal names leave an argument
                assert (g['lists'][lst] or [None] * 3)[1] == (w['lists'][lst] or [None] * 3)[1], (name, stage, lst)
                assert g['lists'][lst] == w['lists'][lst], (name, stage, lst, 'same launches, another argument')
        assert g['src_tab'] == w['src_tab'], (name, stage)
        assert g['state'] == w['state'], (name, stage)


def _seg_structs(lists):
    return sum(len(L.patch.get('seg', ())) for L in lists)


def test_dropped_backward_lists_take_their_structs_along():
    """eight distinct frozen sets through `select_frozen`: what `set_segments` visits is what the live lists registered - the forward's and at most
    _BWD_SETS + 2 backward states' (select_frozen pops the current key, trims to _BWD_SETS + 1 entries and re-inserts) - not what nine builds
    registered; and an args struct of a dropped list is gone once the list is"""
    m, ps, plan = P.cpu_plan()
    names = list(ps.params)
    sets = [frozenset(n for n in names if f'.layers.{k % 5}.' in n and ('.2.fn.' if k < 5 else '.1.fn.') in n) for k in range(8)]
    assert len(set(sets)) == 8
    plan.select_frozen(sets[0])
    first = plan.bwd
    per_state = _seg_structs([first])
    assert per_state == 5 * 5 + 1                                  # per layer: the pull launch and its wrapper side, the fused pre / post pair, the AdaLN-pre backward; hidden 0's pull launch
    struct = weakref.ref(next(a for fn, a in first if fn == 'tfx_attn_bwd'))
    kept = weakref.ref(first.keep[0])
    del first
    for fz in sets[1:]:
        plan.select_frozen(fz)
    live = plan._lists()
    states = len(plan._bwd_sets)
    assert states <= plan._BWD_SETS + 2
    assert sum(L is plan.bwd for L in live) == 1 and len({id(L) for L in live}) == len(live)
    assert _seg_structs(live) == _seg_structs([plan.fwd, plan.vel, plan.rec]) + states * per_state
    assert _seg_structs(live) < 9 * per_state
    gc.collect()
    assert struct() is None and kept() is None
    # the setters still reach every kept list
    plan.set_segments(torch.tensor([0, 64], dtype=torch.int32), torch.tensor([64, 64], dtype=torch.int32))
    assert all(a.n_seg == 2 for L in live for a in L.patch.get('seg', ()))
    plan.select_frozen(frozenset())
    assert all(a.n_seg == 2 for a in plan.bwd.patch['seg'])
