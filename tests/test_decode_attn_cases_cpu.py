"""The decode attention catalogue and its sentinels on the CPU (tests/_decode_attn_cases.py): the catalogue covers the visible lengths the two
decode kernels' key walks, masks and clamps depend on, and its sentinel inputs make one key more or less on any edge's rows fail the per-row
tolerances of tests/test_decode_attn_edges_gpu.py by a margin (fp64 reference with kv_end moved by +-1 against the unmoved one)."""
import pytest
import torch

from _decode_attn_cases import (CATALOGUE, COMPACT, MUTATION_MARGIN, ROWS_CASES, TILED_CASES, build_decode_inputs, decode_reference, norm_rows,
                                round_bf16, row_err, row_tol)


def test_rows_kernel_cases_cover_the_key_walk():
    """decode_attn_rows_k: 32 keys per trip of the block, 8 keys per wave, the clamp at the longer row's length"""
    assert all(c.lq in (1, 2) and c.units is None for c in ROWS_CASES)
    assert {c.lq for c in ROWS_CASES} == {1, 2}
    ends = {e for c in ROWS_CASES for ke in c.kv_end for e in ke}
    assert {0, 1, 31} <= {e % 32 for e in ends} and {0, 1, 7} <= {e % 8 for e in ends}
    assert {1, 2} <= ends and {0, 1} <= {c.n_kv - e for c in ROWS_CASES for ke in c.kv_end for e in ke}
    pairs = {ke for c in ROWS_CASES if c.lq == 2 for ke in c.kv_end}
    assert any(a < b_ and (b_, a) in pairs for a, b_ in pairs)                       # both orders of an unequal pair
    assert any(c.b * c.h > 256 for c in ROWS_CASES)                                  # more than one block per CU
    assert any(c.h % 2 for c in ROWS_CASES) and any(c.n_kv > 4096 for c in ROWS_CASES)


def _waves(case):
    """(sample, tile, lengths of the tile's rows, lengths of one wave's 32 rows) for every wave of every query tile"""
    for s, ke in enumerate(case.kv_end):
        for t0 in range(0, len(ke), 128):
            tile = ke[t0:t0 + 128]
            for w0 in range(0, len(tile), 32):
                yield s, t0 // 128, tile, tile[w0:w0 + 32]


def test_tiled_cases_cover_the_cache_addressing():
    """attn_fwd_pipe_kernel<true> with n_kv > 0: tile_kv_limit's true maximum, the per-wave kve_min, tile_dma's clamp at n_kv - 1"""
    assert all(c.units is None for c in TILED_CASES)
    W = [w for c in TILED_CASES for w in _waves(c)]
    assert any(max(w) > w[-1] for _, _, _, w in W)                                   # a wave's largest kv_end not on its last row
    assert any(len(w) > 1 and (min(w) - 1) // 32 != (max(w) - 1) // 32 for _, _, _, w in W)   # a wave's rows straddle a 32-key unit boundary
    assert any(len(t) > 1 and t[-1] == min(t) and t[-1] < max(t) for _, _, t, _ in W)         # a tile whose last row has the smallest kv_end
    lqs = {c.lq for c in TILED_CASES}
    assert {1, 2} <= lqs and max(lqs) > 256 and any(128 < lq <= 256 for lq in lqs)
    assert any(c.n_kv < 64 for c in TILED_CASES) and any(c.n_kv % 64 for c in TILED_CASES) and any(c.n_kv > 4096 for c in TILED_CASES)
    assert any(e == c.n_kv for c in TILED_CASES for ke in c.kv_end for e in ke)
    assert any(c.dh == 32 for c in TILED_CASES)


def test_compacted_case_covers_the_row_ranges():
    row0, cnt, R = COMPACT.units
    assert 0 in cnt and 1 in cnt and 2 in cnt and max(cnt) > 128 and COMPACT.lq == max(cnt)
    assert any(r % 8 for r, c in zip(row0, cnt) if c)
    owned = torch.zeros(R, dtype=torch.bool)
    for s, r0, c in COMPACT.spans():
        assert not owned[r0:r0 + c].any() and r0 + c <= R
        owned[r0:r0 + c] = True
    live = [(r0, c) for r0, c in zip(row0, cnt) if c]
    assert not owned[0] and not owned[R - 1]                                          # unowned rows before and behind the units ...
    assert any(not owned[a + c:b_].all() for (a, c), (b_, _) in zip(live, live[1:]))  # ... and between them
    assert COMPACT.kv_end[cnt.index(1)] == (1,)                                       # the one-row unit sees one key
    two = COMPACT.kv_end[cnt.index(2)]
    assert max(two) == COMPACT.n_kv and min(two) < max(two)
    for ke in COMPACT.kv_end:                                                         # the larger units: a block with a longer inner row
        if len(ke) > 2:
            assert max(ke) > ke[0] == ke[-1]


def test_laser_subset():
    sub = [c for c in CATALOGUE if c.sub]
    assert len(CATALOGUE) // 3 <= len(sub) and all(c.n_kv < 2048 for c in sub)
    assert any(c in ROWS_CASES and c.lq == 1 for c in sub) and any(c in ROWS_CASES and c.lq == 2 for c in sub) and COMPACT in sub
    assert any(c in TILED_CASES and c.lq > 128 for c in sub) and any(c.dh == 32 for c in sub)


def test_masked_cache_rows_are_loud_and_finite():
    """cache rows at or past a sample's largest kv_end are random rows of the visible rows' scale, none zero, none non-finite"""
    for case in CATALOGUE:
        inp = build_decode_inputs(case, 0)
        assert all(torch.isfinite(inp[x]).all() for x in ('q', 'k', 'v', 'gate'))
        k, v = inp['k'].view(case.b, case.n_kv, -1), inp['v'].view(case.b, case.n_kv, -1)
        for s, ke in enumerate(case.kv_end):
            m = max(ke, default=0)
            if m < case.n_kv:
                for x in (k, v):
                    assert float(x[s, m:].norm(dim=-1).min()) >= 0.5 * float(x.norm(dim=-1).median()), (case.name, s)


@pytest.mark.parametrize('laser', [False, True])
@pytest.mark.parametrize('mode', [None, 0, 1])
def test_decode_checks_fail_on_one_key_more_or_less(mode, laser):
    """for every edge of every case and every path of the GPU tests (gains of plan mode 0 / 1 / none, plain and LASER): the fp64 reference on the
    bf16-rounded inputs with kv_end moved by +1 / -1 on the edge's rows (skipping moves below 1 or above n_kv) differs from the unmoved one on
    EVERY one of those rows, in every sentinel head, by >= MUTATION_MARGIN x the tolerance the GPU tests assert - out by row_err, lse in nats.
    Every edge moves in at least one direction, every case with more than one visible key in both."""
    tol = row_tol(laser)
    for case in CATALOGUE:
        if laser and not case.sub:
            continue
        inp = round_bf16(build_decode_inputs(case, mode))
        qt, kt = norm_rows(inp, case)
        base = decode_reference(case, qt, kt, inp['v'], inp['gate'], inp['kv_end'], laser=laser)
        first = {s: r0 for s, r0, _ in case.spans()}
        dirs = set()
        assert len(inp['edges']) == sum(len(set(ke)) for ke in case.kv_end)
        for kind, s, rows, keys in inp['edges']:
            e = case.kv_end[s][rows[0]]
            moved = 0
            for d in (1, -1):
                if e + d < 1 or e + d > case.n_kv:
                    continue
                kv = inp['kv_end'].clone()
                kv[[first[s] + r for r in rows]] += d
                out, lse = decode_reference(case, qt, kt, inp['v'], inp['gate'], kv, laser=laser, only=s)[s]
                d_out = float(row_err(out, base[s][0])[0, 0::2][:, rows].min())
                d_lse = float((lse - base[s][1]).abs()[0, 0::2][:, rows].min())
                assert d_out >= MUTATION_MARGIN * tol['out'], (case.name, mode, laser, kind, s, e, d, 'out', d_out)
                assert d_lse >= MUTATION_MARGIN * tol['lse'], (case.name, mode, laser, kind, s, e, d, 'lse', d_lse)
                moved += 1
                dirs.add(d)
            assert moved >= 1, (case.name, s, e)
        if any(e > 1 for ke in case.kv_end for e in ke):
            assert dirs == {1, -1}, case.name
