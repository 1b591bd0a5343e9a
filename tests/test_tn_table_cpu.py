"""Weight-gradient table launches (tfx.h `table`, engine.Plan `tn_defer`): what can be checked without a GPU - the plan's own launch list and problem
tables built on the CPU, and the library's host-side planning of a table head."""
import collections
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transfusion_pytorch_amd import capi
from _plan_digest import cpu_plan  # noqa: E402

REC = capi.STRUCTS['tfx_gemm_tn_args']


def _cpu_plan(tn_defer, depth=5, groups=3):
    """a real training Plan built on the CPU (nothing is launched): the lists and tables are the product's own"""
    return cpu_plan(depth=depth, dp_groups=groups, tn_defer=tn_defer)


def _records(tab, n):
    raw = bytes(tab.cpu().numpy().tobytes())
    assert len(raw) == n * (ctypes.sizeof(REC) + 4)
    recs = (REC * n).from_buffer_copy(raw)
    ends = (ctypes.c_int32 * n).from_buffer_copy(raw, n * ctypes.sizeof(REC))
    return recs, list(ends)


def _item_key(item):
    fn, a = item
    name = fn if isinstance(fn, str) else fn.__name__
    if isinstance(a, ctypes.Structure):
        return (type(item).__name__, name, bytes(a))
    if isinstance(a, (tuple, list)):
        return (type(item).__name__, name, tuple(v for v in a if isinstance(v, int) and v < 4096))      # (sizes; pointers differ between two plans)
    return (type(item).__name__, name, a)


@pytest.mark.parametrize('run', [1, 2, 'all'])
def test_tables_respect_cuts_and_cover_every_gradient_once(run):
    """deferral forced on the CPU plan (depth 5, 3 exchange groups, T = 128): a table launch sits in front of its group's cut, so no record may write (C or
    colsum) into a range that left at or before the launch's position - the property test_dp_gloo checks on the visible list items; and the tables together hold
    every layer's weight / bias gradient exactly once."""
    from transfusion_pytorch_amd.optim import GradReducer
    m, ps, plan = _cpu_plan(run)
    md, d = m.md, m.md.dim
    red = GradReducer(m, None, groups=3)
    base = ps.grad.data_ptr(); lo, hi = base, base + 4 * ps.numel
    assert [c[1:] for c in plan.bwd_cuts] == [(4, 4), (2, 3), (0, 1)]
    assert plan.tn_tables
    cuts = sorted((idx, first, last) for idx, first, last in plan.bwd_cuts)
    seen = collections.Counter()
    for idx, low, high, tab, n in plan.tn_tables:
        fn, head = plan.bwd[idx]
        assert fn == 'tfx_gemm_tn' and head.table_count == n and head.table_host and head.M == plan.T
        recs, ends = _records(tab, n)
        assert bytes(recs[0])[:REC.group_next.offset] == bytes(head)[:REC.group_next.offset]          # the head is the first product
        tiles = 0
        for r, e in zip(recs, ends):
            tiles += -(-r.N // 256) * -(-r.K // 256)
            assert e == tiles and r.M == plan.T and not r.group_next and not r.table
        sent = [rg for cidx, first, last in cuts if cidx <= idx for rg in red.ranges(first, last)]
        # a run stays inside one exchange group: its launch comes before the cut that hands the group over
        assert any(first <= low and high <= last and cidx > idx for cidx, first, last in cuts), (idx, low, high, cuts)
        for r in recs:
            for ptr in (r.C, r.colsum):
                if not ptr:
                    continue
                assert lo <= ptr < hi
                off = (ptr - base) // 4
                assert not any(a <= off < b for a, b in sent), (idx, off, sent)
                seen[ptr] += 1
    gp = ps.grad_ptr
    want = []
    for i in range(md.depth):
        p = f'transformer.layers.{i}'
        want += [gp(f'{p}.2.fn.net.3.weight'), gp(f'{p}.2.fn.net.0.weight'), gp(f'{p}.2.fn.net.0.bias'), gp(f'{p}.1.fn.to_out.1.weight'), gp(f'{p}.1.fn.to_qk.0.weight')]
        if md.has_skip(i):
            want += [gp(f'{p}.0.weight'), gp(f'{p}.0.weight', d)]
    assert sorted(seen) == sorted(want) and set(seen.values()) == {1}
    # nothing is left in the list as a per-layer group
    heads = [a for fn, a in plan.bwd if fn == 'tfx_gemm_tn' and a.table]
    assert len(heads) == len(plan.tn_tables)
    expect_runs = {1: 5, 2: 3, 'all': 3}[run]                          # groups (4), (2, 3), (0, 1)
    assert len(plan.tn_tables) == expect_runs
    assert all(a._algo_flops > 0 for a in heads)                       # (the run's summed algorithmic work: bench.py reads it from the head)


def test_default_rule_leaves_tiny_plan_unchanged(monkeypatch):
    """the default defers only where a layer's own chains run as one-wave groups: the tiny plan (T = 128) keeps its backward list item for item"""
    monkeypatch.delenv('TFX_TN_DEFER', raising=False)
    _, _, p_def = _cpu_plan(None)
    _, _, p_off = _cpu_plan(0)
    assert p_def.tn_run == 0 and not p_def.tn_tables
    assert len(p_def.bwd) == len(p_off.bwd)
    assert [_item_key(a)[:2] for a in p_def.bwd] == [_item_key(b)[:2] for b in p_off.bwd]
    assert p_def.bwd_cuts == p_off.bwd_cuts and p_def.nbytes == p_off.nbytes
    monkeypatch.setenv('TFX_TN_DEFER', '2')                            # the environment switch is read per Plan
    _, _, p_env = _cpu_plan(None)
    assert p_env.tn_run == 2 and len(p_env.tn_tables) == 3


def _table(shapes, M, splits=0, **head_kw):
    """host-only table (the device pointer is a dummy: tfx_gemm_tn_plan reads the host copy)"""
    n, rs = len(shapes), ctypes.sizeof(REC)
    host = ctypes.create_string_buffer(n * (rs + 4))
    ends = (ctypes.c_int32 * n).from_buffer(host, n * rs)
    tiles = 0
    for k, sh in enumerate(shapes):
        N, K = sh[:2]
        kw = dict(sh[2]) if len(sh) > 2 else {}
        a = capi.make_args('tfx_gemm_tn_args', **{**dict(M=M, N=N, K=K, lda=(N + 7) // 8 * 8, a_cols=(N + 7) // 8 * 8, ldb=(K + 7) // 8 * 8, b_cols=(K + 7) // 8 * 8, ldc=K,
                                                         k_valid=K, splits=0, accumulate=1, alpha=1.0), **kw})
        ctypes.memmove(ctypes.addressof(host) + k * rs, ctypes.addressof(a), rs)
        tiles += -(-N // 256) * -(-K // 256)
        ends[k] = tiles
    head = REC.from_buffer_copy(host, 0)
    head.table, head.table_host, head.table_count, head.splits = 4096, ctypes.addressof(host), n, splits
    for k, v in head_kw.items():
        setattr(head, k, v)
    head._host = host
    return head, tiles


def _plan(head):
    out = [ctypes.c_int32(-9) for _ in range(4)]
    assert capi.lib().tfx_gemm_tn_plan(ctypes.byref(head), *[ctypes.byref(o) for o in out]) == 0
    return tuple(o.value for o in out)


def _makespan(M, tiles, s):
    chunk = -(-(-(-M // s)) // 64) * 64
    return -(-tiles * s // 256) * chunk, chunk


def test_table_head_plan():
    """host logic of a table head: kind 3, the summed tiles, and the chunk count that minimises ceil(tiles x chunks / 256) x chunk length over chunks of >= 256
    rows; tables with a member the one-wave kernel does not take report the head's own plan"""
    T = 65536
    layer = [(512, 1408), (2816, 512), (512, 512), (1544, 512)]          # config 2: FeedForward pair, to_out, to_qk/v/gates
    skip = [(512, 512), (512, 512)]
    shapes = []
    for i in range(7, -1, -1):
        shapes += layer + (skip if i >= 4 else [])
    head, tiles = _table(shapes, T)
    assert tiles == 448
    kind, t, s, grid = _plan(head)
    assert (kind, t) == (3, 448)
    best = min(_makespan(T, tiles, c)[0] for c in range(1, 257) if _makespan(T, tiles, c)[1] >= 256)
    assert _makespan(T, tiles, s)[0] == best and _makespan(T, tiles, s)[1] >= 256
    assert (s, grid) == (4, 1792)                                        # 7 full rounds of 16384-row chunks = the ideal 448 x 65536 / 256
    # smaller tables: one launch whatever the tile count, chunks of >= 256 rows, no more blocks than the makespan rule's own choice (the atomics term only
    # ever argues for fewer chunks)
    for sub in (shapes[:4], shapes[:10], shapes[:22]):
        head, tiles = _table(sub, T)
        kind, t, s, grid = _plan(head)
        costs = {c: _makespan(T, tiles, c)[0] for c in range(1, 257) if _makespan(T, tiles, c)[1] >= 256}
        assert (kind, t) == (3, tiles) and s in costs and s <= min(c for c in costs if costs[c] == min(costs.values()))
        assert grid == (tiles * s + 7) // 8 * 8
    # forced chunk counts are taken as given down to 192 rows
    head, tiles = _table(shapes[:6], 1536, splits=8)
    assert _plan(head) == (3, tiles, 8, (tiles * 8 + 7) // 8 * 8)
    own = _plan(capi.make_args('tfx_gemm_tn_args', M=T, N=512, K=1408, lda=512, a_cols=512, ldb=1408, b_cols=1408, ldc=1408, k_valid=1408, splits=0, accumulate=1, alpha=1.0))
    for bad in ([(512, 1408), (2816, 512, dict(a_rowmap=64))],           # gathered rows
                [(512, 1408), (2816, 512, dict(M=T // 2))]):             # another M
        assert _plan(_table(bad, T)[0]) == own
    assert _plan(_table(shapes[:6], 1000)[0])[0] != 3                    # M % 64 != 0
    assert _plan(_table(shapes[:6], 1536, splits=16)[0])[0] != 3         # 96-row chunks
