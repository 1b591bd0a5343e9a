"""Activation checkpointing (Transfusion.set_activation_checkpointing_, engine.Plan `ckpt`): what can be checked without a GPU - the switch itself, the
plan key, and the launch lists and buffers of real training Plans built on the CPU (nothing is launched)."""
import copy
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILY = ('ua', 'uf', 'og', 'lse', 'ya', 'xb', 'yf', 'ag', 'hm', 'qkvg', 'qkr')          # (+ stats, whose layer axis is the second, xa and - with LASER - vl)


def _model(depth=5):
    from transfusion_pytorch_amd import Transfusion
    torch.manual_seed(0)
    return Transfusion(num_text_tokens=16, dim_latent=(32, 8), transformer=dict(dim=64, depth=depth, heads=1))


def _cpu_plan(ckpt, depth=5, groups=0):
    """a real training Plan built on the CPU (tests/_plan_digest.py): the lists are the product's own"""
    from _plan_digest import cpu_plan
    m, _, plan = cpu_plan(depth=depth, dp_groups=groups, ckpt=ckpt)
    return m, plan


def _name(item):
    return item[0] if isinstance(item[0], str) else item[0].__name__


def test_switch_default_chaining_and_type_check():
    m = _model(2)
    assert m.activation_checkpointing is False
    assert m.set_activation_checkpointing_() is m and m.activation_checkpointing is True
    assert m.set_activation_checkpointing_(False) is m and m.activation_checkpointing is False
    assert m.set_activation_checkpointing_(True).activation_checkpointing is True
    for bad in (1, 0, 'yes', None, 1.0):
        with pytest.raises(TypeError):
            m.set_activation_checkpointing_(bad)
    assert m.activation_checkpointing is True                       # a refused call changes nothing
    with pytest.raises(AttributeError):
        m.activation_checkpointing = False                          # read-only


def test_copies_carry_the_switch():
    m = _model(2).set_activation_checkpointing_(True)
    assert copy.deepcopy(m).activation_checkpointing is True
    assert m._clone_architecture().activation_checkpointing is True          # what create_ema() / EMA(...) build their copy with
    assert copy.deepcopy(_model(2)).activation_checkpointing is False


def test_plan_key_carries_the_switch_for_training_plans_only(monkeypatch):
    """`_plan` with the Plan class stubbed out: a training plan of each setting gets a key of its own (both stay cached), an inference plan's key does
    not depend on the switch"""
    from transfusion_pytorch_amd import transfusion as T
    made = []

    class Stub:
        nbytes = 1

        def __init__(self, store, b, n, I, R, training=True, dp_groups=0, ckpt=False):
            self.training, self.ckpt = training, ckpt
            made.append(self)

        def select_frozen(self, *a):
            pass
    monkeypatch.setattr(T, 'Plan', Stub)
    monkeypatch.setenv('TFX_PLAN_BUDGET_GB', '1')
    m = _model(2)
    p_plain = m._plan(2, 64, 0, {}, True)
    i_plain = m._plan(2, 64, 0, {}, False)
    m.set_activation_checkpointing_(True)
    p_ckpt = m._plan(2, 64, 0, {}, True)
    assert m._plan(2, 64, 0, {}, False) is i_plain                  # inference: the same plan, the switch is not looked at
    assert p_ckpt is not p_plain and p_ckpt.ckpt is True and p_plain.ckpt is False and i_plain.ckpt is False
    assert len(m._plans) == 3 and len(set(m._plans)) == 3
    m.set_activation_checkpointing_(False)
    assert m._plan(2, 64, 0, {}, True) is p_plain and len(made) == 3          # back on the plan that never saw the switch


@pytest.mark.parametrize('side', ['1', '0'])
def test_checkpointed_plan_slots_bytes_and_segments(side, monkeypatch):
    """depth 5 (the two top layers project a U-Net skip): the family has `n_slots` leading entries, the bytes saved are at least the
    allocation arithmetic's, and every layer below the top n_slots has ONE recompute segment, in front of its backward launches, that is the forward's
    own launches of the layer with the attention side's AdaLN-pre as a launch of its own and without the layer's end launch"""
    monkeypatch.setenv('TFX_SIDE_STREAM', side)
    monkeypatch.delenv('TFX_TN_DEFER', raising=False)
    m, P = _cpu_plan(False)
    _, C = _cpu_plan(True)
    D, ns = m.md.depth, 2 if side == '1' else 1
    assert C.n_slots == ns and C.ckpt and not P.ckpt and P.n_slots is None
    fam = [getattr(C, k) for k in FAMILY]
    assert all(t.shape[0] == ns for t in fam) and C.stats.shape[1] == ns
    assert all(getattr(P, k).shape[0] == D for k in FAMILY) and P.stats.shape[1] == D
    xa = {t.data_ptr(): t for t in C.xa.values()}
    assert len(xa) == min(ns, len(C.xa)) and len({t.data_ptr() for t in P.xa.values()}) == len(P.xa)
    # the allocation arithmetic: the plain plan holds D entries of the family and one xa per skip layer, the checkpointed one n_slots entries and at most
    # n_slots xa buffers; nothing else differs
    nb = lambda t: t.numel() * t.element_size()
    slot_bytes = sum(nb(t) for t in fam + [C.stats]) // ns
    xa_saved = sum(nb(t) for t in P.xa.values()) - sum(nb(t) for t in xa.values())
    assert xa_saved >= 0
    assert C.nbytes <= P.nbytes - (D - ns) * slot_bytes - xa_saved
    # what outlives a layer stays per layer
    assert C.hid.shape == P.hid.shape and len(C.xres) == D + 1 and len(C.arsave) == D and C.arerr.shape[0] == D and C.sc_plan.shape[0] == D
    # the forward lists launch the same things; the plain plan is what it always was
    assert [_name(x) for x in C.fwd] == [_name(x) for x in P.fwd]
    assert all(P.recompute_range(i) is None for i in range(D))
    assert [C.recompute_range(i) is None for i in range(D)] == [i >= D - ns for i in range(D)]
    names_f = [_name(x) for x in C.fwd]
    ends = [k for k, nm in enumerate(names_f) if nm == 'tfx_layer_end_fwd']
    assert len(ends) == D
    prev_hi = len(C.bwd)
    for i in range(D - ns):
        lo, hi = C.recompute_range(i)
        assert hi <= prev_hi or i == 0
        seg = C.bwd[lo:hi]
        first = ends[i - 1] + 1 if i else names_f.index('tfx_adaln_pre_fwd')
        fwd = C.fwd[first:ends[i]]
        seg_names, fwd_names = [_name(x) for x in seg], [_name(x) for x in fwd]
        assert 'tfx_layer_end_fwd' not in seg_names and 'tfx_attnres_fwd' not in seg_names
        assert seg_names.count('tfx_adaln_pre_fwd') == 1
        # layers whose AdaLN-pre rode in the previous layer's end launch get it back as a launch of their own; the rest is item for item the forward's
        if 'tfx_adaln_pre_fwd' not in fwd_names:
            k = seg_names.index('tfx_adaln_pre_fwd')
            assert k == 0
            seg, seg_names = seg[1:], seg_names[1:]
        assert seg_names == fwd_names
        for a, b in zip(seg, fwd):
            if isinstance(a[1], ctypes.Structure):
                assert bytes(a[1]) == bytes(b[1]), (i, _name(a))      # same buffers, same sizes: the slot of layer i
        # the segment stands in front of the layer's backward: the next launch is the pull launch of hidden i + 1
        assert _name(C.bwd[hi]) == 'tfx_attnres_pull_bwd'
        if ns == 2:
            assert C.bwd[lo - 1] == ('tfx_join_wait', i + 2)           # the slot's last readers on the side stream have finished
    order = [C.recompute_range(i)[0] for i in range(D - ns)]
    assert order == sorted(order, reverse=True)


def test_checkpointed_plan_ignores_deferred_weight_gradient_tables(monkeypatch):
    monkeypatch.setenv('TFX_TN_DEFER', '2')
    _, P = _cpu_plan(False)
    _, C = _cpu_plan(True)
    assert P.tn_run == 2 and P.tn_tables
    assert C.tn_run == 0 and not C.tn_tables


def test_truncated_backward_holds_no_recompute_segment(monkeypatch):
    """trunk frozen, heads trainable: the backward ends at `bwd_end` in front of the layers - no segment below it; a frozen lower half: the layers the
    truncated list never reaches are never recomputed"""
    monkeypatch.delenv('TFX_SIDE_STREAM', raising=False)
    m, C = _cpu_plan(True, depth=6)
    names = list(m.store.params)
    heads = frozenset(n for n in names if n.startswith('transformer.') or n.startswith('text_embed') or n.startswith('latent_to_model'))
    C.select_frozen(heads)
    assert C.bwd_end is not None and 0 < C.bwd_end < len(C.bwd)
    segs = [C.recompute_range(i) for i in range(4)]
    assert all(s is not None and s[0] >= C.bwd_end for s in segs)
    low = frozenset(n for n in heads if not any(n.startswith(f'transformer.layers.{j}.') and '.to_film.' not in n and '.to_ada_ln_zero.' not in n for j in (3, 4, 5))
                    ) | frozenset(n for n in names if '.to_film.' in n or '.to_ada_ln_zero.' in n or n.startswith('transformer.to_time_cond'))
    C.select_frozen(low)
    assert C.bwd_end is not None
    assert C.recompute_range(3)[1] <= C.bwd_end                      # layer 3 is reached (layers 4, 5 are live from the forward)
    assert all(C.recompute_range(i)[0] >= C.bwd_end for i in range(3))
    C.select_frozen(frozenset())
    assert C.bwd_end is None and all(C.recompute_range(i) is not None for i in range(4))
