"""The GEMM checker of tests/_gemm_cases.py on the CPU: an emulated CORRECT kernel (fp32 matmul on the bf16 operands, the epilogue in fp32, one bf16 round)
passes the per-element bound with zero elements over it for every spec of the covering lists - so the bound is not too tight - and each fault that the
whole-matrix Frobenius ratio of the older GEMM tests lets through (tolerances 6e-3 NT / 5e-3 TN) is caught: the recorded reason the per-element tests exist.
The old ratio misses a fault only when the wrong elements are a small enough share of the matrix (one row of 65,536 is 3.9e-3), so the row faults run at
M = 131,073 - on the CPU, once; the GPU tests keep small shapes."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as G  # noqa: E402

OLD_TOL_NT, OLD_TOL_TN = 6e-3, 5e-3


def test_covering_lists_cover_every_pair():
    """every (form, epilogue) and (form, feature) pair at least once with a ragged M and a ragged N tile (GEGLU: N % 64 == 0 by contract); the 256 x 256 family
    meets one to five K tiles, N % 8 != 0 and the long-K fp32 case"""
    for form in (5, 4, 2, 1, 0):
        cases = [c for c in G.NT_CASES if c.form == form]
        tm, tn = G.NT_TILE[form]
        ragged = [c for c in cases if c.M % tm and (c.N % tn or c.epi.startswith('GEGLU'))]
        epis = G.EPIS[:4] if form == 0 else G.EPIS
        assert {c.epi for c in ragged} >= set(epis), form
        assert {c.feat for c in ragged} >= set(G.FEATS[:5]), form
        for epi in ('BF16', 'F32'):
            assert {c.bias for c in cases if c.epi == epi and c.feat is None} == {False, True}, (form, epi)
    fam = G.NT_FAMILY_CASES
    assert {c.form for c in fam} == {3, 6, 7}
    assert {c.K for c in fam if c.form in (6, 7)} >= {64, 128, 192, 256, 320}
    assert {c.epi for c in fam if c.form == 3} >= set(G.EPIS) and {c.feat for c in fam if c.form == 3} >= set(G.FEATS[:5]) - {'rowmap'}
    assert any(c.N % 8 for c in fam if c.form == 6) and any(c.epi == 'F32' and c.K == 1024 for c in fam if c.form == 6)
    assert {c.M for c in fam} == {1025, 1279} and {c.N for c in fam} >= {264, 520, 260}
    print(f'covering lists: {len(G.NT_CASES)} NT in process, {len(fam)} NT 256 x 256 family, {len(G.TN_CASES)} TN + chain of {len(G.TN_CHAIN)} + table of {len(G.TN_TABLE)}')


def test_in_process_cases_run_on_the_kernel_they_name():
    """tfx_gemm_nt_plan / tfx_gemm_tn_plan are host logic: the in-process lists name the right kernels before any GPU is involved"""
    from transfusion_pytorch_amd import capi
    lib = capi.lib()
    for sp in G.NT_CASES:
        case = G.build_nt(sp)
        a = capi.make_args('tfx_gemm_nt_args', epi=capi.ENUMS['TFX_EPI_' + sp.epi], **case.kw)
        kind, grid = ctypes.c_int32(-9), ctypes.c_int32(-9)
        assert lib.tfx_gemm_nt_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(grid)) == 0, sp.name
        assert kind.value == sp.form, f'{sp.name}: the planner names kind {kind.value}'
    for sp in G.TN_CASES:
        case = G.build_tn(sp)
        out = [ctypes.c_int32(-9) for _ in range(4)]
        assert lib.tfx_gemm_tn_plan(ctypes.byref(capi.make_args('tfx_gemm_tn_args', **case.kw)), *[ctypes.byref(o) for o in out]) == 0, sp.name
        assert out[0].value == sp.form, f'{sp.name}: the planner names kind {out[0].value}'


@pytest.mark.parametrize('form', [5, 4, 2, 1, 0, 7, 6, 3])
def test_correct_emulation_has_no_element_over_the_bound_nt(form):
    worst = 0.
    for sp in G.NT_CASES + G.NT_FAMILY_CASES:
        if sp.form == form:
            worst = max(worst, G.check_case(G.emulate_nt(G.build_nt(sp))))
    print(f'NT form {form}: worst error / bound of the emulation {worst:.3f}')
    assert 0 < worst <= 1


def test_correct_emulation_has_no_element_over_the_bound_tn():
    for sp in G.TN_CASES + G.TN_CHAIN + G.TN_TABLE:
        worst = G.check_tn(G.emulate_tn(G.build_tn(sp)))
        assert 0 < worst <= 1, sp.name


def test_activation_allowances():
    """the figures the module's docstring quotes, and the fp32 CPU evaluation of the same formulas inside them (measured on the reference side)"""
    import torch.nn.functional as F
    x = torch.linspace(-7.9, 7.9, 200001, dtype=torch.float64)
    assert abs(G.L_GELU1 - 1.1290) < 1e-4 and abs(G.L_GELU2 - 0.7979) < 1e-4 and abs(G.L_SILU - 1.0998) < 1e-4
    assert abs(G.R3 - (2.0 ** -24) * G.L_GELU3 / 6) < 1e-20 and 5e-6 < G.R2 < 7e-6 and abs(G.D_CDF - 1.03e-6) < 1e-8
    d_gelu = (F.gelu(x.float()).double() - G.gelu64(x)).abs()
    d_silu = (F.silu(x.float()).double() - G.silu64(x)).abs()
    print(f'A_GELU(0) {float(G.a_gelu(torch.zeros(1, dtype=torch.float64))):.3e}  A_GELU(2) {float(G.a_gelu(torch.full((1,), 2., dtype=torch.float64))):.3e}  '
          f'A_DGELU {float(G.a_dgelu(torch.zeros(1, dtype=torch.float64))):.3e}  A_SILU(2) {float(G.a_silu(torch.full((1,), 2., dtype=torch.float64))):.3e}; '
          f'torch fp32 gelu / silu deviation from fp64: {float(d_gelu.max()):.2e} / {float(d_silu.max()):.2e}')
    assert bool((d_gelu <= G.a_gelu(x) + G.U32 * G.gelu64(x).abs()).all()) and bool((d_silu <= G.a_silu(x) + G.U32 * x.abs()).all())


# (fault, the spec it is injected into): shapes at which the old ratio is blind to it
BIG = 131073
NT_FAULT_SPECS = [
    ('last_row_unwritten', G.NT(3, BIG, 68, 64, 'BF16')),
    ('last_row_from_above', G.NT(3, BIG, 68, 64, 'BF16', True)),
    ('k_tile_dropped', G.NT(3, 4099, 520, 320, 'BF16', True)),
    ('bias_shifted', G.NT(1, 70, 4100, 64, 'BF16', True, None, 0, 0.05)),
    ('resid_unmapped', G.NT(3, BIG, 68, 64, 'RESID', False, 'resid_mapped_few')),
    ('a2_boundary', G.NT(3, BIG, 68, 128, 'BF16', False, 'a2_first')),
    ('guard_column', G.NT(2, 1025, 264, 320, 'BF16', True, 'rowmap')),
    ('guard_column', G.NT(5, 130, 200, 320, 'SILU', True)),
    ('dropped_row_written', G.NT(2, 1025, 264, 320, 'BF16', True, 'rowmap')),
    ('dropped_row_written', G.NT(4, 130, 200, 192, 'RESID', False, 'resid_mapped')),
]


@pytest.mark.parametrize('fault,spec', NT_FAULT_SPECS, ids=[f'{f}-{s.M}x{s.N}x{s.K}-{s.epi}' for f, s in NT_FAULT_SPECS])
def test_nt_fault_is_caught_and_the_old_ratio_misses_it(fault, spec):
    assert fault in G.NT_FAULTS
    good = G.emulate_nt(G.build_nt(spec))
    G.check_case(good)
    base = max(G.old_ratio(good))
    bad = G.emulate_nt(G.build_nt(spec), fault)
    old = max(G.old_ratio(bad))
    print(f'{fault}: old ratio {old:.3e} (without the fault {base:.3e}; tolerance {OLD_TOL_NT})')
    assert old <= OLD_TOL_NT, 'the old whole-matrix check was expected to miss this fault'
    with pytest.raises(AssertionError) as ei:
        G.check_case(bad)
    print(ei.value)
    assert ('outside the product' in str(ei.value)) == (fault in ('guard_column', 'dropped_row_written'))


TN_FAULT_SPECS = [('k_group_off_by_one', G.TN(2, 128, 1000, 1024, 1, k_group=40)), ('colsum_twice', G.TN(0, 128, 80008, 64, 1, colsum=True, rowmap=True))]


@pytest.mark.parametrize('fault,spec', TN_FAULT_SPECS, ids=[f for f, _ in TN_FAULT_SPECS])
def test_tn_fault_is_caught_and_the_old_ratio_misses_it(fault, spec):
    assert fault in G.TN_FAULTS
    G.check_tn(G.emulate_tn(G.build_tn(spec)))
    bad = G.emulate_tn(G.build_tn(spec), fault)
    old = max(G.old_ratio_tn(bad))
    print(f'{fault}: old ratio {old:.3e} (tolerance {OLD_TOL_TN})')
    assert old <= OLD_TOL_TN, 'the old whole-matrix check was expected to miss this fault'
    with pytest.raises(AssertionError) as ei:
        G.check_tn(bad)
    print(ei.value)


def test_tn_guard_faults_are_caught():
    """a write at or beyond k_valid, into a k_group gap's neighbour row guard, or into the row a dropped map entry would have named"""
    case = G.emulate_tn(G.build_tn(G.TN(0, 128, 200, 136, 1, 0.5, True, 3)))
    G.check_tn(case)
    o = case.outs[0]
    free = (set(range(200)) - set(case.dest[case.kept].tolist())).pop()
    for r, c in ((G.GUARD + 5, 133), (G.GUARD + 5, 136), (G.GUARD + 200, 0), (G.GUARD + free, 0)):
        saved = o.buf[r, c].clone()
        o.buf[r, c] = 1.0
        with pytest.raises(AssertionError, match='outside the product'):
            G.check_tn(case)
        o.buf[r, c] = saved
    G.check_tn(case)
