"""The parameter-side checker of tests/_param_cases.py on the CPU: an fp32 emulation of a CORRECT kernel, in two orders (sums: left to right and by halving;
elementwise kernels: the kernel's expression and an algebraically equal one), has no element over its bound - so the bounds are not too tight - and every
fault of the list is caught by the per-element check or a guard band.  Next to each fault the whole-tensor Frobenius ratio of the older tests
(tests/test_kernels_gpu.py; the tightest model-level tolerance where a kernel had no direct test) is computed and the faults it misses are printed.
Fault 1 is what the kernels of tfx_colsum_bf16 did with a row-map entry of -1 before they skipped it: the row in front of the source was added in."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _param_cases as C  # noqa: E402

ORDERS = ('linear', 'tree')


def _upd(rep, name, v):
    rep[name] = max(rep.get(name, 0.), v)


@pytest.fixture(scope='module')
def muon():
    return C.build_muon()


@pytest.mark.parametrize('order', ORDERS)
def test_emulated_colsum_sumsq_are_under_their_bounds(order):
    rep = {}
    shapes = [(8, 8), (520, 528), (1024, 1024), (1, 1), (65, 72), (130, 131)]
    for k, (Cc, ld) in enumerate(shapes):
        for j, R in enumerate((1, 9, 65, 1001)):
            maps = C.COLSUM_MAPS[(k + j) % 5]
            c = C.build_colsum(R, Cc, ld, maps)
            C.emulate_colsum(c, order)
            _upd(rep, 'colsum out', C.check_out(f'colsum R={R} C={Cc} ld={ld} {maps} {order}', c.out))
    for n in C.SUMSQ_N[:6] + ((2 ** 20 + 7,) if order == 'tree' else ()):
        c = C.build_sumsq(n)
        C.emulate_sumsq(c, order)
        _upd(rep, 'sumsq', C.check_out(f'sumsq n={n} {order}', c.out))
        _upd(rep, 'sumsq_det', C.check_out(f'sumsq_det n={n} {order}', c.det))
    print(f'emulation ({order}): worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))
    assert all(0 < v <= 1 for v in rep.values())


@pytest.mark.parametrize('order', ORDERS)
def test_emulated_elementwise_kernels_are_under_their_bounds(order):
    rep = {}
    for n in C.VEC_N:
        for d in C.EMA_DECAYS:
            c = C.build_ema(n, d)
            online = c.online.clone()
            C.emulate_ema(c, order)
            _upd(rep, 'ema', C.check_out(f'ema n={n} decay={d} {order}', c.out))
            if d == 0 and order == 'linear':
                assert torch.equal(c.out.view[0], online)
        for s in C.SCALES:
            c = C.build_scale(n, s)
            C.emulate_scale(c, order)
            _upd(rep, 'scale', C.check_out(f'scale n={n} s={s} {order}', c.out))
    for R, dl, ld in C.NOISE_SHAPES:
        for with_eps in (True, False):
            c = C.build_noise(R, dl, ld, with_eps=with_eps)
            C.emulate_noise(c, order)
            _upd(rep, 'noise xt', C.check_out(f'noise R={R} dl={dl} eps={with_eps} {order}', c.xt))
            assert C.check_out(f'noise flow R={R}', c.flow) == 0
    for I, half, ld in C.FOURIER_SHAPES:
        c = C.build_fourier(I, half, ld)
        C.emulate_fourier(c, order)
        _upd(rep, 'fourier', C.check_out(f'fourier I={I} half={half} {order}', c.out))
    print(f'emulation ({order}): worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))
    assert all(0 < v <= 1 for v in rep.values())


def test_emulated_copies_are_exact():
    for Rs, Cs in C.CAST_SHAPES:
        for use_map in (False, True):
            for cd in ('lt', 'gt'):
                for tr in (False, True):
                    c = C.build_cast(Rs, Cs, use_map, cd, tr)
                    assert c.Rd % 32 and c.ld % 32
                    C.emulate_cast(c, None)
                    assert C.check_out(f'cast {Rs}x{Cs} map={use_map} {cd} t={tr}', c.out) == 0
    for cols in C.SCATTER_COLS:
        c = C.build_scatter(cols)
        C.emulate_scatter(c)
        assert C.check_out(f'scatter cols={cols}', c.out) == 0


@pytest.mark.parametrize('order', ORDERS)
def test_emulated_muon_is_under_its_bounds(order, muon):
    rep = {}
    c = muon
    k = 0
    for mu in C.MUON_MOMENTA:
        for nes in (False, True):
            clip = C.MUON_CLIPS[k % 4]; k += 1
            o = C.muon_prep_outs(c, mu, nes, clip, ws_poison=bool(k % 2))
            C.emulate_muon_prep(c, o, order)
            for out in (o.buf, o.ws, o.partials):
                _upd(rep, out.name, C.check_out(f'muon prep mu={mu} nesterov={nes} {clip} {order}', out))
            assert torch.equal(C._bits(o.ws.view[0, c.ps]), C._bits(o.ws.view[0, c.pt]))
            nrm = C.muon_norm_out(c, o.partials.view[0].clone())
            C.emulate_muon_norm(c, nrm, o.partials.view[0].clone(), order)
            _upd(rep, 'inv', C.check_out(f'muon norm mu={mu} {order}', nrm))
    for lr, decay in ((0.02, 1.), (0.02, 1 - 0.02 * 0.1)):
        a = C.muon_apply_out(c, lr, decay)
        C.emulate_muon_apply(c, a, order)
        _upd(rep, 'apply', C.check_out(f'muon apply decay={decay} {order}', a))
    print(f'muon emulation ({order}): worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.items()))
    assert all(0 < v <= 1 for v in rep.values())


def test_muon_host_tables_give_disjoint_regions(muon):
    """the layout of optim._muon_host_tables: both copies of every matrix inside the workspace, disjoint, leading dimensions multiples of 128 that hold a row;
    the blocks of the prep / apply grid numbered without gaps; the lr ratio per shape"""
    c = muon
    pos = torch.cat([c.ps, c.pt])
    assert int(pos.min()) >= 0 and int(pos.max()) < c.x_elems and pos.unique().numel() == pos.numel()
    nb = 0
    assert len({m['lr_ratio'] for m in c.H['mats']}) == c.nmat
    for i, (m, (off, r, cc)) in enumerate(zip(c.H['mats'], c.segs)):
        assert (m['off'], m['rows'], m['cols']) == (off, r, cc) and off % 4 == 0
        assert m['ld_s'] % 128 == 0 and m['ld_t'] % 128 == 0 and m['ld_s'] >= cc and m['ld_t'] >= r
        assert m['blk0'] == nb and bool(m['flip']) == (r > cc)
        assert c.ratio0[i] == max(1., r / cc) ** 0.5
        nb += -(-r // 64) * -(-cc // 64)
    assert nb == c.nblk == len(c.H['blk_mat']) and c.H['mats'][-1]['prep_blocks'] == 272
    assert [c.H['blk_mat'][m['blk0']] for m in c.H['mats']] == list(range(c.nmat))


def _run_fault(fault, muon):
    """outputs of the faulty emulation"""
    c = muon
    if fault == 'neg_row_reads_previous_row':
        k = C.build_colsum(130, 64, 64, 'rows_neg'); C.emulate_colsum(k, 'tree', fault); return [k.out]
    if fault == 'colsum8_tail_dropped':
        k = C.build_colsum(1001, 520, 528, 'none'); C.emulate_colsum(k, 'tree', fault); return [k.out]
    if fault == 'dup_colmap_overwrites':
        k = C.build_colsum(65, 130, 131, 'cols'); C.emulate_colsum(k, 'tree', fault); return [k.out]
    if fault in ('transposed_edge_block_swapped', 'partial_last_row_group_dropped', 'clip_after_momentum', 'nesterov_reads_old_buf'):
        o = C.muon_prep_outs(c, 0.95, True, C.MUON_CLIPS[1])
        C.emulate_muon_prep(c, o, 'tree', fault)
        return [o.buf, o.ws, o.partials]
    if fault == 'norm_first_256_partials':
        o = C.muon_prep_outs(c, 0.95, True, C.MUON_CLIPS[0])
        C.emulate_muon_prep(c, o, 'tree')
        p = o.partials.view[0].clone()
        nrm = C.muon_norm_out(c, p); C.emulate_muon_norm(c, nrm, p, 'tree', fault)
        return [nrm]
    if fault == 'apply_reads_transposed_copy_of_flipped':
        a = C.muon_apply_out(c, 0.02, 1.); C.emulate_muon_apply(c, a, 'linear', fault); return [a]
    if fault == 'sumsq_tail_dropped':
        k = C.build_sumsq(1023); C.emulate_sumsq(k, 'tree', fault); return [k.out, k.det]
    if fault == 'cast_t_reads_rows_past_Rs':
        k = C.build_cast(200, 70, True, 'gt', True); C.emulate_cast(k, None, fault); return [k.out]
    if fault == 'ema_online_swapped':
        k = C.build_ema(2053, 0.9999); C.emulate_ema(k, 'linear', fault); return [k.out]
    if fault == 'noise_time_of_row_0':
        k = C.build_noise(300, 48, 64); C.emulate_noise(k, 'linear', fault); return [k.xt, k.flow]
    if fault == 'scale_through_bf16_twice':
        k = C.build_scale(2053, 1. / 3.); C.emulate_scale(k, 'linear', fault); return [k.out]
    raise KeyError(fault)


# what the old whole-tensor ratio does with each fault at these shapes (measured here, at the old tolerance of the output or, where the older suite had no direct
# test, the tightest model-level one).  It sees the gross faults - where it had a test that reached the path at all: no older test passed a map to colsum, ran a
# tail of sumsq against a reference, or called the Muon kernels one by one.
OLD_MEASURE_MISSES = {'neg_row_reads_previous_row': False, 'colsum8_tail_dropped': False, 'dup_colmap_overwrites': False, 'transposed_edge_block_swapped': True,
                      'partial_last_row_group_dropped': False, 'clip_after_momentum': False, 'nesterov_reads_old_buf': False,
                      'apply_reads_transposed_copy_of_flipped': False, 'norm_first_256_partials': True, 'sumsq_tail_dropped': True,
                      'cast_t_reads_rows_past_Rs': False, 'ema_online_swapped': False, 'noise_time_of_row_0': False, 'scale_through_bf16_twice': True}


@pytest.mark.parametrize('fault', C.FAULTS)
def test_fault_is_caught_per_element(fault, muon):
    outs = _run_fault(fault, muon)
    old = {o.name: C.old_ratio(o) for o in outs}
    tols = {n: C.OLD_TOL.get(n, C.NO_DIRECT_TOL) for n in old}
    missed = all(r <= tols[n] for n, r in old.items())
    print(f'{fault}: old whole-tensor ratios ' + ', '.join(f'{n} {r:.3e} (tolerance {tols[n]:g})' for n, r in old.items()) +
          f' -> the old measure {"MISSES" if missed else "sees"} it')
    assert missed == OLD_MEASURE_MISSES[fault]
    with pytest.raises(AssertionError) as ei:
        for o in outs:
            C.check_out(fault, o)
    print(ei.value)


def test_fault_list_is_the_issue_s():
    assert set(C.FAULTS) == set(OLD_MEASURE_MISSES) and len(C.FAULTS) == 14
