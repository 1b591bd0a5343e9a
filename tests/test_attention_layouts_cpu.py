"""The attention sweep's mask catalogue and sentinels on the CPU (tests/_attn_cases.py): the catalogue follows the packer's mask rule, covers the
layouts the kernels' skip paths depend on, and its sentinel inputs make one key more or less on any edge's rows fail the GPU sweep's per-row
tolerances by a margin (fp64 reference with kv_end moved by +-1 against the unmoved one)."""
import numpy as np
import pytest
import torch

from _attn_cases import CASES, CATALOGUE, MUTATION_MARGIN, build_inputs, edges, layout_maps, metrics, reference, row_tol

KINDS = {'block_end', 'block_start', 'causal', 'tile', 'clipped'}


def test_layout_maps_match_token_maps_on_a_packed_batch():
    """the helper's rule against packing.token_maps for a real packed batch (196- and 49-token image blocks, a 1-D block, text-only sample),
    also at a view length that clips a block"""
    from oracle.transfusion_oracle import OracleConfig
    from transfusion_pytorch_amd.packing import scan_batch, token_maps
    cfg = OracleConfig(num_text_tokens=200, dim=64, depth=1, dim_latents=(8, 16), heads=1, dim_head=64)
    g = torch.Generator().manual_seed(3)
    ti = lambda L: torch.randint(0, 200, (L,), generator=g)
    batch = [[ti(5), (0, torch.randn(14, 14, 8, generator=g)), ti(3), (1, torch.randn(7, 7, 16, generator=g))],
             [(1, torch.randn(7, 7, 16, generator=g)), (0, torch.randn(4, 8, generator=g)), (1, torch.randn(7, 7, 16, generator=g))],
             [ti(9)]]
    P = scan_batch(batch, num_modalities=2, dim_latents=cfg.dim_latents, sos_id=cfg.sos_id, eos_id=cfg.eos_id, meta_id=cfg.meta_id,
                   som_ids=cfg.som_ids, eom_ids=cfg.eom_ids, add_sos_eos=True)
    assert sorted(set(int(x) for x in P.inst_len)) == [4, 49, 196]
    for n in (P.n_full - 1, P.n_full - 40):
        tm = token_maps(P, n, 2)
        samples = [[] for _ in range(P.b)]
        for bi, off, ln in zip(P.inst_b, P.inst_off, P.inst_len):
            samples[int(bi)].append((int(off), int(ln)))
        kv_end, q_start = layout_maps(n, samples)
        assert np.array_equal(kv_end.numpy(), tm.kv_end) and np.array_equal(q_start.numpy(), tm.q_start), n


def test_catalogue_covers_the_layouts():
    ns = {c.n for c in CATALOGUE}
    assert {1, 5, 33, 63, 65, 127, 129, 200, 1000, 1024, 2048, 4096} <= ns
    assert any(c.h >= 16 for c in CATALOGUE) and any(c.dh == 32 for c in CATALOGUE)
    assert all(c.b == 1 and c.h == 2 for c in CATALOGUE if c.n >= 2048)
    kinds, lens, starts0, ends_n, ends_64, past_64 = set(), set(), False, False, False, False
    for c in CATALOGUE:
        kinds |= {k for k, _, _ in edges(c)}
        for s, blocks in enumerate(c.samples):
            for off, ln in blocks:
                hi = min(off + ln, c.n)
                lens.add(ln)
                starts0 |= off == 0
                ends_n |= off + ln == c.n and s < c.b - 1                   # ends exactly at n in a sample that is not the last
                ends_64 |= hi % 64 == 0 and off + ln <= c.n
                past_64 |= hi % 64 == 1 and hi > 1
    assert kinds == KINDS and starts0 and ends_n and ends_64 and past_64
    assert {1, 49, 196} <= lens and max(lens) >= 256
    assert any(len(set(c.samples)) == c.b and c.b > 1 for c in CATALOGUE)     # different layouts per sample
    assert any(blocks == ((0, c.n),) for c in CATALOGUE for blocks in c.samples)   # a whole sample one block
    assert any(blocks == () for c in CATALOGUE for blocks in c.samples)             # pure causal


@pytest.mark.parametrize('mode,laser,nr', [(None, False, False), (0, False, False), (1, False, False), (0, True, False), (0, False, True)])
def test_sweep_fails_on_one_key_more_or_less(mode, laser, nr):
    """for every edge kind and every path of the GPU sweep (plan modes, LASER, the fused QK-norm backward's raw d q | d k): the fp64 reference
    with kv_end moved by +1 / -1 on the edge's rows (skipping moves that leave a row with no key or point past n) differs from the unmoved
    one, on the affected rows (out, dq: the edge's rows; dk, dv: the keys the rows see either way), by >= MUTATION_MARGIN x that path's per-row
    tolerance - in the sentinel head"""
    tol = row_tol(laser, nr)
    seen = set()
    for name in ('n5', 'n33', 'n65', 'n129', 'n200', 'dh32'):
        case = CASES[name]
        inp = build_inputs(case, mode)
        base = reference(inp, case, laser=laser, nr=nr)
        for kind, s, rows, keys in inp['edges']:
            e = int(inp['kv_end'][s, rows[0]])
            for d in (1, -1):
                if e + d < 1 or e + d > case.n:
                    continue
                kv = inp['kv_end'].clone()
                kv[s, rows] += d
                m = metrics(reference(inp, case, laser=laser, nr=nr, kv_end=kv), base)
                worst = {q: float(m[q][s, 0, rows].max()) for q in ('out', 'dq')}
                worst.update({q: float(m[q][s, 0, :max(e, e + d)].max()) for q in ('dk', 'dv')})
                for q, w in worst.items():
                    assert w >= MUTATION_MARGIN * tol[q], (name, kind, s, e, d, q, w)
                seen.add(kind)
    assert seen == KINDS, seen
