"""Training attention (tfx_attn_fwd + tfx_attn_bwd) over the mask layout catalogue of tests/_attn_cases.py against fp64 autograd: long modality
blocks at odd offsets, blocks on and across the 64-key / 128-query tile edges, clipped blocks in front of another sample, one-row samples, 16
heads, dim_head 32; plan modes 0 / 1 (the training path: the generated dQ asm loop, the dK/dV kernel's mode-0/1 branches) and no plan (mode 2);
LASER and the fused QK-norm / RoPE backward on a subset.  Per-row metrics (tests/_attn_cases.py ROW_TOL) besides the global ones, in every
head, sentinel heads in which one key more or less moves a row by O(1), poisoned outputs and guard columns.  Then the forward against a KV cache in the
compacted layout with long units, and the bit-identity of TFX_ATTN_BWD_PIPE=0 to the default."""
import os
import subprocess
import sys

import pytest
import torch

from _attn_cases import (CASES, CATALOGUE, LASER_C, POISON, attention_ref, exact_input_reference, gain_err, metrics, reference, row_err,
                         row_tol, run_kernels)

pytestmark = pytest.mark.gpu
DEV, BF = 'cuda', torch.bfloat16
# global relative Frobenius tolerances: tests/test_kernels_gpu.py (plain), tests/test_laser_gpu.py (LASER), the fused-backward test (d q | d k raw)
GLOBAL_TOL = {'out': 8e-3, 'dq': 2e-2, 'dk': 2e-2, 'dv': 2e-2, 'dgate': 2e-2}
GLOBAL_TOL_LASER = {'out': 1e-2, 'dq': 4e-2, 'dk': 4e-2, 'dv': 4e-2, 'dgate': 4e-2}
# gain gradients relative to the sum of their terms' magnitudes (they cancel ~1000-fold here).  d gamma_q is checked against the exact-input
# reference only: against the whole chain its q~ are fp64, not the kernel's bf16 ones, which moves the sentinel rows' dS (measured up to 0.2)
GLOBAL_TOL_NR = {'dq': 2.5e-2, 'dk': 2.5e-2, 'dgk': 2e-2}


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _sweep(case, mode, laser=False, nr=False):
    """global errors against fp64 autograd of the whole chain (reference()), per-row errors against fp64 from each kernel's own inputs
    (exact_input_reference()), every head"""
    inp, qk, got = run_kernels(case, mode, laser=laser, nr=nr)
    full = reference(inp, case, laser=laser, nr=nr, qk=None if nr else qk, dev=DEV)
    if nr:                                         # the forward, dv and dgate of the fused path are the plain path's: from the kernel's q~ | k~
        plain = reference(inp, case, qk=qk, dev=DEV)
        for key in ('out', 'lse', 'dv', 'dgate'):
            full[key] = plain[key]
    ex = exact_input_reference(inp, case, qk, got, laser=laser, nr=nr, dev=DEV)
    gt = dict(GLOBAL_TOL_LASER if laser else GLOBAL_TOL)
    if nr:
        gt.update(GLOBAL_TOL_NR)
    if case.n == 1:                                # one key per row: dq = dk = 0 exactly, no relative global error (the per-row check stays)
        gt.pop('dq'); gt.pop('dk')
    rt = row_tol(laser, nr)
    glob = {key: gain_err(got[key], full[key], ex[key + '_scale']) if key in ('dgq', 'dgk') else relerr(got[key], full[key]) for key in gt}
    m = metrics(got, ex)
    worst = {key: float(v.max()) for key, v in m.items()}
    where = {key: tuple(int(i) for i in torch.nonzero(v == v.max())[0].tolist()) for key, v in m.items()}
    if nr:                                         # the gain gradients: sums over every row and head
        for key in ('dgq', 'dgk'):
            worst[key], where[key] = gain_err(got[key], ex[key], ex[key + '_scale']), ()
    print(f'ROWERR {case.name} mode={mode} laser={int(laser)} nr={int(nr)} ' + ' '.join(f'{k}={worst[k]:.2e}@{where[k]}' for k in worst)
          + ' | global ' + ' '.join(f'{k}={v:.2e}' for k, v in glob.items()))
    fails = [f'{k}: global {glob[k]:.3e} > {gt[k]}' for k in glob if not glob[k] <= gt[k]]
    fails += [f'{k}: row {where[k]} {worst[k]:.3e} > {rt[k]}' for k in worst if not worst[k] <= rt[k]]
    assert not fails, f'{case.name} mode {mode} laser {laser} nr {nr}: ' + '; '.join(fails)


@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('name', [c.name for c in CATALOGUE])
def test_attention_layout_sweep(name, mode):
    _sweep(CASES[name], mode)


@pytest.mark.parametrize('mode', [None, 0, 1])
@pytest.mark.parametrize('laser,nr', [(True, False), (False, True)])
@pytest.mark.parametrize('name', [c.name for c in CATALOGUE if c.sub])
def test_attention_layout_sweep_laser_and_fused_norm_bwd(name, laser, nr, mode):
    _sweep(CASES[name], mode, laser=laser, nr=nr)


# ---------------------------------------------------------------------------------------------- forward against a KV cache, compacted rows
@pytest.mark.parametrize('laser', [0, 1])
def test_attention_compacted_rows_with_long_units(laser):
    """tfx.h q_row0 / q_cnt (sample_many's decode plans): units of 300 rows (three query tiles), 140 and 57 rows, a q_cnt = 0 sample, flat rows
    owned by no sample between and behind the units (must keep their bits); within a unit the largest kv_end sits on an inner row (a text
    row next to a block), not on a tile's last row.  Per-row metric against fp64."""
    torch.manual_seed(7)
    b, h, nkv = 4, 2, 700
    HD = h * 64
    cnt, row0, R = [300, 0, 140, 57], [0, 305, 306, 450], 520                  # rows 300..305, 446..449 and 507..519 belong to no sample
    nmax = max(cnt)
    cache = (torch.randn(b, nkv, 2 * HD, device=DEV) * 2).to(BF)
    cache[:, :, :HD] = (cache[:, :, :HD].float() * 0.6).to(BF)
    q = (torch.randn(R, HD, device=DEV) * 0.35).to(BF)
    gate = torch.randn(R, 8, device=DEV).to(BF)
    kv_end = torch.zeros(R, dtype=torch.int32)
    for s_, (r0, c) in enumerate(zip(row0, cnt)):
        base = 100 + 150 * s_
        kv_end[r0:r0 + c] = base                                               # the block being decoded sees prefix + block ...
        if c:
            kv_end[r0 + min(5, c - 1)] = base + 97                                # ... a text row next to it sees more
    kv_end = kv_end.to(DEV)
    if laser:
        side = torch.zeros(b * nkv, HD, device=DEV, dtype=BF)
        la = tfx_args('tfx_laser_v_args', T=b * nkv, H=h, v=cache.view(b * nkv, 2 * HD)[:, HD:], ld_v=2 * HD, vl=side, ld_vl=HD, c=LASER_C)
        call('tfx_laser_v_fwd', la)
        v_in, ld_v = side, HD
    else:
        v_in, ld_v = cache.view(b * nkv, 2 * HD)[:, HD:], 2 * HD
    out = torch.full((R, HD + 8), POISON, device=DEV, dtype=torch.int16).view(BF)
    lse = torch.full((b, h, nmax), float('nan'), device=DEV)
    a = tfx_args('tfx_attn_args', q=q, k=cache, v=v_in, ld_q=HD, ld_k=2 * HD, ld_v=ld_v, gate=gate, ld_gate=8, kv_end=kv_end, q_start=kv_end,
                 out=out, ld_out=HD + 8, lse=lse, b=b, h=h, n=nmax, softcap=50.0, n_kv=nkv, laser=laser,
                 q_row0=torch.tensor(row0, dtype=torch.int32, device=DEV), q_cnt=torch.tensor(cnt, dtype=torch.int32, device=DEV))
    call('tfx_attn_fwd', a)
    torch.cuda.synchronize()
    owned = torch.zeros(R, dtype=torch.bool)
    worst, worst_lse = 0., 0.
    for s_, (r0, c) in enumerate(zip(row0, cnt)):
        assert bool(torch.isnan(lse[s_, :, c:]).all()), 'lse rows past the unit are not written'
        if c == 0:
            continue
        owned[r0:r0 + c] = True
        qf = q[r0:r0 + c].double().reshape(1, c, h, 64).transpose(1, 2)
        kf = cache[s_, :, :HD].double().reshape(1, nkv, h, 64).transpose(1, 2)
        vf = cache[s_, :, HD:].double().reshape(1, nkv, h, 64).transpose(1, 2)
        ref, ref_lse = attention_ref(qf, kf, vf, gate[r0:r0 + c, :h].double().t()[None], kv_end[None, r0:r0 + c], laser=bool(laser))
        got = out[r0:r0 + c, :HD].float().reshape(1, c, h, 64).transpose(1, 2)
        assert torch.isfinite(got).all()
        worst = max(worst, float(row_err(got, ref).max()))
        worst_lse = max(worst_lse, float((lse[s_, :, :c] - ref_lse[0]).abs().max()))
    print(f'  compacted laser={laser}: worst row {worst:.3e} lse {worst_lse:.3e}')
    tol = row_tol(bool(laser))
    assert worst <= tol['out'] and worst_lse <= tol['lse']
    assert bool((out[~owned.to(DEV)].view(torch.int16) == POISON).all()), 'flat rows owned by no sample must keep their bits'
    assert bool((out[:, HD:].view(torch.int16) == POISON).all()), 'the ld padding of out must keep its bits'


def tfx_args(name, **kw):
    from transfusion_pytorch_amd import capi
    return capi.make_args(name, **kw)


def call(fn, a):
    from transfusion_pytorch_amd import capi
    capi.call(fn, a, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- bit-identity of the switches
def test_attention_switches_are_bit_identical():
    """tfx.h / attention.hip: TFX_ATTN_BWD_PIPE=0 (the plain-loop dQ kernel) gives the bits of the default (the generated dQ loop).
    The library reads the switch once per process: one child per setting (tests/_attn_hash_child.py) hashes
    out, lse, d q~ | d k~ and d v | d gate over long-block layouts in plan modes none / 0 / 1."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_attn_hash_child.py')
    outs = []
    for extra in ({}, {'TFX_ATTN_BWD_PIPE': '0'}):
        env = dict(os.environ)
        env.pop('TFX_ATTN_BWD_PIPE', None)
        env.update(extra)
        r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append((extra, [ln for ln in r.stdout.splitlines() if ln.startswith('CASE')]))
    base = outs[0][1]
    assert len(base) == 12
    for extra, lines in outs[1:]:
        assert len(lines) == len(base)
        for a, b in zip(base, lines):
            assert a == b, f'{extra}:\n default: {a}\n switch:  {b}'
