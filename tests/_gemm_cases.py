"""GEMM case builders, fp64 references, per-element bounds and guard bands (not collected: no test_ prefix; imports no GPU code at module level).

Shared by tests/test_gemm_refs_cpu.py (a correct fp32 emulation passes, every injected fault is caught - and the old whole-matrix ratio misses it),
tests/test_gemm_elementwise_gpu.py (every NT / TN kernel form in the test process) and tests/_gemm_elementwise_child.py (the 256 x 256 NT family).

The reference of a case is computed in float64 from the exact bf16 operand values (the saved `aux` bits of GEGLU_BWD included): the pre-activation
x, the expected output(s) y and the magnitude sum S (NT: sum_k |a||b| + |bias| + |R|; TN: |alpha| sum_m |a||b| + |C_initial|).

Bound of one element, derived, not tuned (u16 = 2^-8: bf16 round-to-nearest-even; u32 = 2^-24):
  E32 = 2 (n + 2) u32 S     fp32 accumulation of the n products and two more terms in ANY order (bf16 x bf16 is exact in fp32; (n + 2) u32 S is the
                            classical bound, the factor 2 covers the MFMA block adder's internal alignment); n = K for NT, n = M for TN (atomics included)
  fp32 outputs              tol = E32
  bf16 outputs              tol = u16 |y| + 2 E32    (u16 |y| is SHARP: round-to-nearest of a value just above a power of two is off by u16 |y|, so over 1e5 elements
                            the worst error / bound of a correct kernel sits at 0.9-0.99 - the CPU emulation gives the same figures; what the accumulation
                            uses of its share shows on the fp32 outputs: about 0.01)
  activations               tol = u16 |y| + 2 L E32 + A: L = the largest derivative magnitude (fp64, evaluated below: L_SILU, L_GELU1, L_GELU2), A = the
                            approximation allowance of the device function.  Products (GEGLU v = a gelu'(g), h = a gelu(g)) take L E32 per factor:
                            |gelu'(g)| E32(a) + |a| L_GELU2 E32(g), resp. |gelu(g)| E32(a) + |a| L_GELU1 E32(g).
  GEGLU_BWD                 y = dh x saved: the saved bf16 value is an operand (exact), tol = (u16 + u32) |y| + 2 |saved| E32.

Allowances A, from the schemes csrc/gemm.hip and csrc/tfx_common.h document:
  sigmoid (SILU)   sigmoidf_(x) = v_rcp_f32(1 + __expf(-x)).  __expf = v_exp_f32(x log2 e): rounding the product moves the exponent by |x| log2(e) u32, i.e.
                   the result by |x| u32 relative; v_exp_f32 and v_rcp_f32 are 1 ulp (2 u32) each, the sum 1 + e one rounding; e / (1 + e) <= 1:
                   sigma within (|x| + 5) u32, silu = x sigma one rounding more.   A_SILU = (|x| + 8) u32 |y|     (4.8e-7 |y| at x = 0)
  GELU, polynomial (every kernel but the ping-pong one): Phi from Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7, halved in Phi = 7.5e-8) + the fp32
                   Horner form / __expf / v_rcp_f32, for which 16 u32 is ALLOWED, not derived (five FMAs, one v_exp, one v_rcp on values <= 1.5 would
                   come to about 8 u32):      D_CDF = 7.5e-8 + 16 u32 = 1.03e-6;   gelu = g Phi: |g| D_CDF
                   gelu' = Phi + g phi(g): D_CDF + 8 u32 (|g| phi(g) (g^2 / 2 + 3) < 2)
  GELU, grid (ping-pong kernel): second-order Taylor polynomial on a 2^-7 grid, |d| <= 2^-8:  remainder R3 = (2^-8)^3 max|gelu'''| / 6 = 7.7e-9 for gelu
                   and one order less, R2 = (2^-8)^2 max|gelu'''| / 2 = 5.9e-6, for the derivative slot (max|gelu'''| = 0.7788, evaluated below); three fp32 table
                   entries and two FMAs: 4 u32 (|gelu| + 2^-8), resp. 4 u32 L_GELU1.  Beyond +-8 the end nodes extrapolate: the polynomial's own
                   quadratic term 31 phi(8) (|g| - 8 + 2^-7)^2 plus the tail (1 + |g|) (1 - Phi(8)) - both below 1e-12 for |g| < 100.
                   A case does not know which scheme its kernel uses: A takes the SUM of both, A_GELU = |g| D_CDF + R3 + 4 u32 (|gelu| + 2^-8) + u32 |gelu| + ext,
                   A_DGELU = D_CDF + 8 u32 + R2 + 4 u32 L_GELU1 + ext  (7.7e-6, next to u16 |gelu'| ~ 2e-3: the activations' error is the bf16 store).

Guard bands: every output buffer has GUARD rows in front and behind and ld = width + GUARD columns (but for the few cases about ldc itself); guards, dropped rows, rows that no map entry names,
TN columns from k_valid on and the gaps of k_group are filled with a fixed non-NaN bit pattern (or, where the output aliases the residual, hold its
values) and must come back bit-identical.  Padding columns of lda > K / ldb > K hold 1e4: an over-read along K is a wrong element.
"""
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

U16, U32 = 2.0 ** -8, 2.0 ** -24
GUARD = 8
FILL_BF16, FILL_F32 = 0x4B4B, 0x4B4B4B4B       # bf16 1.33e7 / fp32 1.33e7: finite, never produced by a case
PAD = 1e4
BF = torch.bfloat16
EPIS = ('BF16', 'F32', 'SILU', 'RESID', 'GEGLU', 'GEGLU_BWD')
FEATS = ('a2_first', 'a2_last', 'a_rowmap', 'rowmap', 'resid_mapped', 'resid_mapped_few')     # the last: identity map but for two scattered rows (fault specs of the CPU test)
NT_TILE = {0: (128, 128), 1: (128, 128), 2: (128, 128), 3: (256, 256), 4: (64, 128), 5: (64, 64), 6: (256, 256), 7: (256, 256)}
TN_TILE = {-1: (128, 128), 0: (128, 128), 2: (256, 256), 3: (256, 256)}


# ---------------------------------------------------------------------------------------------- activations in float64
def _phi(g):
    return torch.exp(-0.5 * g * g) * (2 * math.pi) ** -0.5


def _Phi(g):
    return 0.5 * torch.erfc(-g * 2 ** -0.5)


def gelu64(g):
    return g * _Phi(g)


def dgelu64(g):
    return _Phi(g) + g * _phi(g)


def silu64(x):
    return x * torch.sigmoid(x)


_G = torch.linspace(-12, 12, 2400001, dtype=torch.float64)
L_GELU1 = float(dgelu64(_G).abs().max())                          # 1.1290
L_GELU2 = float((_phi(_G) * (2 - _G * _G)).abs().max())           # 0.7979 = 2 phi(0)
L_GELU3 = float((_phi(_G) * _G * (_G * _G - 4)).abs().max())      # 0.7788
_S = torch.sigmoid(_G)
L_SILU = float((_S * (1 + _G * (1 - _S))).abs().max())            # 1.0998
del _G, _S
D_CDF = 7.5e-8 + 16 * U32
R3 = (2.0 ** -8) ** 3 * L_GELU3 / 6
R2 = (2.0 ** -8) ** 2 * L_GELU3 / 2
_PHI8 = math.exp(-32.) * (2 * math.pi) ** -0.5
_Q8 = 0.5 * math.erfc(8 * 2 ** -0.5)


def _ext(g):
    far = (g.abs() - 8 + 2.0 ** -7).clamp_min(0)
    return torch.where(g.abs() > 8 - 2.0 ** -7, 31 * _PHI8 * far * far + (1 + g.abs()) * _Q8, torch.zeros_like(g))


def a_silu(x):
    return (x.abs() + 8) * U32 * silu64(x).abs()


def a_gelu(g):
    u = gelu64(g).abs()
    return g.abs() * D_CDF + R3 + 4 * U32 * (u + 2.0 ** -8) + U32 * u + _ext(g)


def a_dgelu(g):
    return D_CDF + 8 * U32 + R2 + 4 * U32 * L_GELU1 + _ext(g)


def geglu_perm(dip):
    """physical column c of the interleaved layout -> (is_gate, feature)."""
    c = torch.arange(2 * dip)
    blk, within = c // 64, c % 64
    is_gate = within >= 32
    feat = blk * 32 + within % 32
    return is_gate, feat


# ---------------------------------------------------------------------------------------------- bounds and checks
def e32(n_terms, S):
    return 2 * (n_terms + 2) * U32 * S


def tol_f32(E):
    return E


def tol_bf16(y, E):
    return U16 * y.abs() + 2 * E


def nt_ref(A, B, bias=None, R=None):
    """(x, E32) in float64 of A . B^T + bias + R from bf16 operands on any device: the one-line per-element check next to an older test's whole-matrix one:
    assert_elementwise(name, C, x, tol_bf16(x, E))"""
    x = A.double() @ B.double().T
    S = A.double().abs() @ B.double().abs().T
    if bias is not None:
        x += bias.double(); S += bias.double().abs()
    if R is not None:
        x += R.double(); S += R.double().abs()
    return x, e32(A.shape[1], S)


def assert_elementwise(name, got, ref, tol, tile=(128, 128), rows=None):
    """every element finite and within its bound; reports the worst element (row, column, tile coordinates, error, bound).  Returns the worst error / bound."""
    got = got.double()
    assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
    if got.numel() == 0:
        return 0.
    err = (got - ref).abs()
    finite = torch.isfinite(got)
    ratio = torch.where(finite, err / tol.clamp_min(1e-300), torch.full_like(err, float('inf')))
    ratio = torch.where(finite & (err == 0), torch.zeros_like(ratio), ratio)
    flat = int(ratio.argmax())
    r, c = divmod(flat, got.shape[1])
    worst = float(ratio.flatten()[flat])
    over = int((ratio > 1).sum())
    if over:
        row = int(rows[r]) if rows is not None else r
        raise AssertionError(f'{name}: {over} of {got.numel()} elements over their bound (or non-finite); worst at row {row} col {c} '
                             f'(tile {row // tile[0]}, {c // tile[1]}; {row % tile[0]}, {c % tile[1]} inside): got {float(got[r, c])!r} want {float(ref[r, c])!r} '
                             f'err {float(err[r, c]):.3e} tol {float(tol[r, c]):.3e}')
    return worst


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def assert_untouched(name, buf, before, written):
    """everything outside the `written` mask (guards, dropped / unnamed rows, cut columns) is bit-identical to the snapshot"""
    moved = (_bits(buf) != _bits(before)) & ~written
    if bool(moved.any()):
        idx = moved.nonzero()[0].tolist()
        raise AssertionError(f'{name}: {int(moved.sum())} elements outside the product were written; first at buffer row {idx[0] - GUARD} col {idx[-1] if len(idx) > 1 else 0} '
                             f'(rows / columns relative to the output: negative or >= its size = a guard)')


def relerr(a, b):
    """the old whole-matrix measure (tests/test_kernels_gpu.py check): Frobenius norm of the difference over the reference's"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-20))


def guarded(rows, cols, dtype, device, pad=GUARD):
    """(buffer [GUARD + rows + GUARD, cols + pad] filled with the guard pattern, view of its rows x cols inside)"""
    buf = torch.empty(rows + 2 * GUARD, cols + pad, dtype=dtype, device=device)
    _bits(buf).fill_(FILL_BF16 if dtype == BF else FILL_F32)
    return buf, buf[GUARD:GUARD + rows, :cols]


def padded(t, pad_cols=GUARD):
    """copy of the 2-D operand with `pad_cols` columns of PAD behind every row (ld = cols + pad_cols); returns (buffer, view)"""
    buf = torch.full((t.shape[0], t.shape[1] + pad_cols), PAD, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


# ---------------------------------------------------------------------------------------------- NT cases
class NT(NamedTuple):
    form: int                    # the kernel tfx_gemm_nt_plan must name (0 fallback, 1 LDS-DMA 128 x 128, 2 mid, 3 ping-pong, 4 skinny, 5 decode, 6 / 7 one-wave)
    M: int
    N: int                       # as tfx_gemm_nt_args.N: GEGLU = the 2 dip physical columns, GEGLU_BWD = dip
    K: int
    epi: str
    bias: bool = False
    feat: Optional[str] = None   # one of FEATS
    seed: int = 0
    bias_scale: float = 1.0
    ldc_pad: int = GUARD         # ldc = width + ldc_pad (ldc2 likewise): 8 guard columns unless the case is about the alignment of ldc itself

    @property
    def name(self):
        return f'nt{self.form} {self.M}x{self.N}x{self.K} {self.epi} bias={int(self.bias)} {self.feat or "-"}' + ('' if self.ldc_pad == GUARD else f' ldc+{self.ldc_pad}')


def _nt(form, shapes_epis):
    return [NT(form, *s) for s in shapes_epis]


# In the test process (default environment).  K % 64 == 0 is the contract (tfx.h; pinned by test_nt_gemm_kernel_selection): the decode kernel's K values
# are 256, 320, 512.  Every (form, epilogue) and (form, feature) pair with a ragged M and a ragged N tile; GEGLU / GEGLU_BWD need N % 64 == 0 (N = 128, 320), so
# the register-staged fallback (N % 4 != 0 in the default environment) cannot meet them here (NT_STAGED_GEGLU runs them in a child with TFX_GEMM_GLDS=0).
# The `ldc+<pad>` cases are about the alignment of ldc: ldc = N = 6 / 5 without guard columns (the model-to-latent projection at a dim_latent that is no
# multiple of 4 - fp32 rows 8 / 4 bytes apart from 16-byte alignment), and ldc % 4 == 2 / odd ldc on the LDS-DMA kernels' direct-store epilogue.
NT_CASES = (
    _nt(5, [(1, 4, 256, 'BF16'), (63, 200, 320, 'BF16', True), (65, 200, 512, 'F32'), (130, 4, 256, 'F32', True), (130, 200, 320, 'SILU', True),
            (65, 200, 256, 'RESID', True), (1, 200, 512, 'RESID'), (63, 128, 256, 'GEGLU', True), (130, 320, 320, 'GEGLU'), (65, 128, 512, 'GEGLU_BWD'),
            (130, 320, 256, 'GEGLU_BWD'), (130, 200, 512, 'BF16', False, 'a2_first'), (65, 200, 320, 'RESID', True, 'a2_last'),
            (63, 200, 256, 'BF16', False, 'a_rowmap'), (130, 200, 320, 'BF16', True, 'rowmap'), (130, 200, 256, 'RESID', False, 'resid_mapped'),
            (65, 4, 512, 'SILU', False, 'rowmap')]) +
    _nt(4, [(1, 4, 64, 'BF16'), (63, 200, 128, 'BF16', True), (65, 200, 192, 'F32'), (130, 4, 64, 'F32', True), (130, 200, 128, 'SILU', True),
            (65, 200, 192, 'RESID', True), (1, 200, 64, 'RESID'), (63, 128, 64, 'GEGLU', True), (130, 320, 192, 'GEGLU'), (65, 128, 128, 'GEGLU_BWD'),
            (130, 320, 64, 'GEGLU_BWD'), (130, 200, 192, 'BF16', False, 'a2_first'), (65, 200, 192, 'RESID', True, 'a2_last'),
            (63, 200, 64, 'BF16', False, 'a_rowmap'), (130, 200, 128, 'BF16', True, 'rowmap'), (130, 200, 192, 'RESID', False, 'resid_mapped'),
            (65, 4, 128, 'SILU', False, 'rowmap')]) +
    _nt(2, [(1025, 132, 256, 'BF16'), (1151, 264, 320, 'BF16', True), (1151, 132, 320, 'F32'), (1025, 264, 256, 'F32', True), (1151, 132, 256, 'SILU', True),
            (1025, 264, 320, 'RESID', True), (1025, 128, 256, 'GEGLU', True), (1151, 320, 320, 'GEGLU'), (1151, 128, 320, 'GEGLU_BWD'),
            (1025, 320, 256, 'GEGLU_BWD'), (1151, 264, 320, 'BF16', False, 'a2_first'), (1025, 132, 320, 'RESID', True, 'a2_last'),
            (1151, 132, 256, 'BF16', False, 'a_rowmap'), (1025, 264, 320, 'BF16', True, 'rowmap'), (1151, 264, 256, 'RESID', False, 'resid_mapped')]) +
    _nt(1, [(1025, 132, 64, 'BF16'), (1151, 264, 192, 'BF16', True), (1151, 132, 192, 'F32'), (1025, 264, 64, 'F32', True), (1151, 132, 64, 'SILU', True),
            (1025, 264, 192, 'RESID', True), (1025, 128, 64, 'GEGLU', True), (1151, 320, 192, 'GEGLU'), (1151, 128, 192, 'GEGLU_BWD'),
            (1025, 320, 64, 'GEGLU_BWD'), (1151, 264, 192, 'BF16', False, 'a2_first'), (1025, 132, 192, 'RESID', True, 'a2_last'),
            (1151, 132, 64, 'BF16', False, 'a_rowmap'), (1025, 264, 192, 'BF16', True, 'rowmap'), (1151, 264, 64, 'RESID', False, 'resid_mapped')]) +
    _nt(0, [(70, 202, 64, 'BF16'), (1025, 390, 192, 'BF16', True), (1025, 202, 320, 'F32'), (70, 390, 64, 'F32', True), (70, 202, 192, 'SILU', True),
            (1025, 390, 64, 'RESID', True), (1025, 202, 192, 'BF16', False, 'a2_first'), (70, 390, 320, 'RESID', True, 'a2_last'),
            (1025, 202, 64, 'BF16', False, 'a_rowmap'), (70, 390, 192, 'BF16', True, 'rowmap'), (1025, 202, 128, 'RESID', False, 'resid_mapped'),
            (70, 6, 64, 'F32', True, None, 0, 1.0, 0), (1025, 5, 128, 'F32', True, None, 0, 1.0, 0), (70, 5, 64, 'BF16', False, None, 0, 1.0, 0),
            (1025, 6, 64, 'BF16', True, None, 0, 1.0, 0), (70, 202, 64, 'SILU', True, None, 0, 1.0, 5)]) +
    _nt(1, [(1025, 132, 64, 'BF16', True, None, 0, 1.0, 6), (1151, 264, 192, 'F32', True, None, 0, 1.0, 5), (1151, 132, 192, 'RESID', False, 'rowmap', 0, 1.0, 5)]) +
    _nt(2, [(1151, 264, 256, 'BF16', False, None, 0, 1.0, 5), (1025, 132, 320, 'SILU', True, None, 0, 1.0, 6)]) +
    _nt(5, [(130, 200, 256, 'BF16', True, None, 0, 1.0, 5), (65, 200, 512, 'F32', False, None, 0, 1.0, 6)]) +
    _nt(4, [(130, 200, 128, 'RESID', True, None, 0, 1.0, 5)]) +
    # the K rings of the 4-wave LDS-DMA kernels, filled and wrapped (csrc/nt_ring.h).  Skinny, 6 slots: 5 / 6 / 7 / 8 K-tiles = the deepest wait, a prologue that
    # exactly fills the ring, the first refill, the wrap onto slots 0 and 1 (a2_last: the second source starts in tile 7 = slot 1).  N = 5512: 3 x 87 = 261
    # tiles of 64 x 64, one more than the decode kernel takes.  Two slots with one refill (2 K-tiles); four slots wrapped and drained (7 K-tiles).
    _nt(4, [(130, 5512, 320, 'BF16', True), (130, 5512, 384, 'F32'), (130, 5512, 448, 'BF16', False, 'a_rowmap'), (130, 5512, 512, 'BF16', False, 'a2_last')]) +
    _nt(1, [(1025, 132, 128, 'BF16')]) +
    _nt(2, [(1151, 264, 448, 'BF16', True)]))
NT_STAGED_GEGLU = [c for c in NT_CASES if c.epi.startswith('GEGLU')]      # on kind 0 in a child with TFX_GEMM_GLDS=0

# The 256 x 256 family (child process, TFX_NT_PP_MIN=1): one to five K tiles = every entry path of the generated loops; N = 260: the one-wave kernel's direct store.
NT_FAMILY_CASES = (
    _nt(7, [(1025, 264, 192, 'BF16'), (1279, 520, 256, 'BF16', True), (1025, 520, 320, 'BF16', False, 'rowmap'), (1279, 264, 256, 'BF16', True, 'rowmap'),
            (1279, 520, 192, 'BF16')]) +
    _nt(6, [(1025, 264, 64, 'BF16'), (1279, 520, 128, 'BF16', True), (1279, 260, 192, 'BF16', True), (1025, 260, 320, 'BF16', False, 'rowmap'),
            (1279, 260, 256, 'BF16'), (1025, 264, 1024, 'F32', True), (1279, 260, 128, 'BF16', True, 'rowmap')]) +
    _nt(3, [(1025, 264, 64, 'F32'), (1279, 520, 320, 'F32', True), (1025, 260, 128, 'F32'), (1025, 264, 128, 'SILU', True), (1279, 260, 256, 'SILU'),
            (1279, 520, 192, 'RESID', True), (1025, 260, 64, 'RESID'), (1025, 320, 256, 'GEGLU', True), (1279, 128, 64, 'GEGLU'),
            (1279, 128, 320, 'GEGLU_BWD'), (1025, 320, 128, 'GEGLU_BWD'), (1279, 264, 192, 'BF16', False, 'a2_first'), (1025, 520, 320, 'RESID', True, 'a2_last'),
            (1279, 264, 128, 'BF16', False, 'a_rowmap'), (1025, 520, 256, 'SILU', True, 'rowmap'), (1025, 264, 256, 'RESID', False, 'resid_mapped'),
            (1279, 264, 128, 'RESID', True, None, 0, 1.0, 5), (1025, 520, 64, 'F32', True, None, 0, 1.0, 6)]) +       # ldc odd / % 4 == 2: the direct stores
    _nt(6, [(1025, 264, 192, 'BF16', False, None, 0, 1.0, 6), (1279, 520, 256, 'BF16', True, None, 0, 1.0, 5)]))      # ldc % 8 != 0 keeps K >= 192 off kind 7


def build_nt(spec, device='cpu'):
    """operands, tfx_gemm_nt_args keywords (without `epi`: the caller holds the enum) and the fp64 reference of one NT case"""
    M, N, K, epi, feat = spec.M, spec.N, spec.K, spec.epi, spec.feat
    g = torch.Generator(device='cpu').manual_seed(1000 * spec.seed + M + 7 * N + 13 * K + 101 * EPIS.index(epi) + (17 * (FEATS.index(feat) + 1) if feat else 0))
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(device)
    keep = []
    # ---- A (rows possibly gathered, K possibly split over two sources), B
    Msrc = M // 2 + 1 if feat == 'a_rowmap' else M
    A = rn(Msrc, K)
    B = rn(N, K, scale=K ** -0.5)
    Bbuf, Bv = padded(B)
    kw = dict(B=Bv, ldb=K + GUARD, M=M, N=N, K=K)
    if feat in ('a2_first', 'a2_last'):
        assert K >= 128
        K1 = 64 if feat == 'a2_first' else K - 64
        A1buf, A1v = padded(A[:, :K1].contiguous()); A2buf, A2v = padded(A[:, K1:].contiguous())
        kw.update(A=A1v, lda=K1 + GUARD, A2=A2v, lda2=K - K1 + GUARD, K1=K1)
        keep += [A1buf, A2buf]
    else:
        Abuf, Av = padded(A)
        kw.update(A=Av, lda=K + GUARD)
        keep.append(Abuf)
    Aeff = A
    if feat == 'a_rowmap':
        amap = torch.randint(0, Msrc, (M,), generator=g).to(torch.int32)       # M draws from M / 2 + 1 rows: repeats, out of order
        amap[0], amap[M - 1] = Msrc - 1, 0
        amap = amap.to(device)
        kw.update(a_rowmap=amap); keep.append(amap)
        Aeff = A[amap.long()]
    # ---- output rows
    T = M
    dest = torch.arange(M)
    if feat == 'resid_mapped_few':
        T = M + 37
        dest[M // 3], dest[M - 1] = M + 5, M + 30
        dest[7] = -1
    elif feat in ('rowmap', 'resid_mapped'):
        T = M + 37
        dest = torch.randperm(T, generator=g)[:M]
        dest[::17] = -1                                                          # drops (row 0 among them)
    if T != M:
        rmap = dest.to(torch.int32).to(device)
        kw.update(rowmap=rmap); keep.append(rmap)
    dest = dest.to(device)
    kept = dest >= 0
    # ---- side operands
    x = Aeff.double() @ B.double().T
    S = Aeff.double().abs() @ B.double().abs().T
    if spec.bias:
        bias = torch.full(((N + 3) // 4 * 4,), PAD, device=device)              # readable up to ceil(N / 4) 4 floats (tfx.h)
        bias[:N] = (torch.randn(N, generator=g) * spec.bias_scale).to(device)
        kw.update(bias=bias); keep.append(bias)
        x = x + bias[:N].double(); S = S + bias[:N].double().abs()
    wC = {'GEGLU_BWD': 2 * N}.get(epi, N)
    dtC = torch.float32 if epi == 'F32' else BF
    lp = spec.ldc_pad
    Cbuf, Cv = guarded(T, wC, dtC, device, lp)
    kw.update(C=Cv, ldc=wC + lp)
    if epi == 'RESID':
        if feat in ('resid_mapped', 'resid_mapped_few'):                         # the engine's in-place use: R aliases C, read at the scattered row
            Cv.copy_(rn(T, N))
            kw.update(R=Cv, ldr=N + lp, resid_mapped=1)
            R = torch.zeros(M, N, dtype=torch.float64, device=device)
            R[kept] = Cv[dest[kept]].double()
        else:
            Rbuf, Rv = padded(rn(M, N))
            kw.update(R=Rv, ldr=N + GUARD); keep.append(Rbuf)
            R = Rv.double()
        x = x + R; S = S + R.abs()
    E = e32(K, S)
    outs = []

    def out(name, buf, view, ref, tol):
        outs.append(SimpleNamespace(name=name, buf=buf, view=view, before=None, ref=ref, tol=tol, ncols=ref.shape[1]))

    if epi == 'BF16' or epi == 'RESID':
        out('C', Cbuf, Cv, x, tol_bf16(x, E))
    elif epi == 'F32':
        out('C', Cbuf, Cv, x, tol_f32(E))
    elif epi == 'SILU':
        C2buf, C2v = guarded(T, N, BF, device, lp)
        kw.update(C2=C2v, ldc2=N + lp)
        y = silu64(x)
        out('C silu', Cbuf, Cv, y, U16 * y.abs() + 2 * L_SILU * E + a_silu(x))
        out('C2 pre', C2buf, C2v, x, tol_bf16(x, E))
    elif epi == 'GEGLU':
        assert N % 64 == 0 and T == M
        dip = N // 2
        is_gate = geglu_perm(dip)[0].to(device)
        a, gg, Ea, Eg = x[:, ~is_gate], x[:, is_gate], E[:, ~is_gate], E[:, is_gate]
        u, d1 = gelu64(gg), dgelu64(gg)
        v, h = a * d1, a * u
        ref = torch.empty_like(x); tol = torch.empty_like(x)
        ref[:, ~is_gate] = u; tol[:, ~is_gate] = U16 * u.abs() + 2 * L_GELU1 * Eg + a_gelu(gg)
        ref[:, is_gate] = v; tol[:, is_gate] = (U16 + U32) * v.abs() + 2 * (d1.abs() * Ea + a.abs() * L_GELU2 * Eg) + a.abs() * a_dgelu(gg)
        C2buf, C2v = guarded(T, dip, BF, device, lp)
        kw.update(C2=C2v, ldc2=dip + lp)
        out('C saved [u|v]', Cbuf, Cv, ref, tol)
        out('C2 hidden', C2buf, C2v, h, (U16 + U32) * h.abs() + 2 * (u.abs() * Ea + a.abs() * L_GELU1 * Eg) + a.abs() * a_gelu(gg))
    elif epi == 'GEGLU_BWD':
        assert N % 64 == 0 and not spec.bias
        is_gate = geglu_perm(N)[0].to(device)
        auxbuf, auxv = padded(rn(M, 2 * N))
        kw.update(aux=auxv, ldaux=2 * N + GUARD); keep.append(auxbuf)
        sv = auxv.double()
        ref = torch.empty(M, 2 * N, dtype=torch.float64, device=device); tol = torch.empty_like(ref)
        for sel in (~is_gate, is_gate):
            ref[:, sel] = x * sv[:, sel]
            tol[:, sel] = (U16 + U32) * ref[:, sel].abs() + 2 * sv[:, sel].abs() * E
        out('C d[a|g]', Cbuf, Cv, ref, tol)
    else:
        raise KeyError(epi)
    for o in outs:
        o.before = o.buf.clone()
    return SimpleNamespace(spec=spec, kw=kw, outs=outs, dest=dest, kept=kept, x=x, S=S, keep=keep + [Bbuf], tile=NT_TILE[spec.form], Aeff=Aeff, B=B, T=T)


def check_case(case):
    """per-element bound on every output of an NT or TN case, then the guard bands; returns the worst error / bound"""
    worst = 0.
    kept, dest = case.kept, case.dest
    src_rows = kept.nonzero().flatten()
    for o in case.outs:
        cols = o.cols if getattr(o, 'cols', None) is not None else torch.arange(o.ncols, device=o.view.device)
        got = o.view[dest[kept]][:, cols]
        worst = max(worst, assert_elementwise(f'{case.spec.name} {o.name}', got, o.ref[kept], o.tol[kept], case.tile, rows=src_rows))
        written = torch.zeros(o.buf.shape, dtype=torch.bool, device=o.buf.device)
        rows = (dest[kept] + GUARD)
        written[rows[:, None], cols[None, :]] = True
        assert_untouched(f'{case.spec.name} {o.name}', o.buf, o.before, written)
    return worst


# ---------------------------------------------------------------------------------------------- CPU emulation of a correct kernel, and of the faults
def emulate_nt(case, fault=None):
    """what a correct kernel writes: fp32 matmul on the bf16 operands, the epilogue in fp32, one bf16 round - into the case's own guarded buffers.
    `fault`: one of NT_FAULTS, injected into that arithmetic."""
    import torch.nn.functional as F
    sp, kw = case.spec, case.kw
    M, N, K = sp.M, sp.N, sp.K
    A, B = case.Aeff.float(), case.B.float()
    acc = A @ B.T
    tm, tn = case.tile
    last_n0 = (N - 1) // tn * tn
    if fault == 'k_tile_dropped':                 # one 64-wide K tile missing for one 4-column group (a row block of 32)
        r0, c0 = min(32, M - 1) // 32 * 32 if M > 32 else 0, (min(N, 72) - 1) // 4 * 4
        k0 = K - 64
        acc[r0:r0 + 32, c0:c0 + 4] -= A[r0:r0 + 32, k0:k0 + 64] @ B[c0:c0 + 4, k0:k0 + 64].T
    if fault == 'a2_boundary':                    # the ragged last row tile switches to the second source one K tile late: that tile comes from the wrong columns
        K1 = kw['K1']
        m0 = (M - 1) // tm * tm
        wrong = torch.cat([case.Aeff[m0:, :K1], case.Aeff[m0:, K1 - 64:K1], case.Aeff[m0:, K1 + 64:]], 1).float()
        acc[m0:] = wrong @ B.T
    x = acc
    if sp.bias:
        b = kw['bias'][:N].clone()
        if fault == 'bias_shifted':               # bias of the last N tile read 4 columns further
            full = kw['bias']
            idx = (torch.arange(last_n0, N) + 4).clamp_max(full.numel() - 1)
            b[last_n0:] = torch.where(idx < N, full[idx], torch.zeros(()))
        x = x + b
    dest = case.dest.clone()
    kept = case.kept
    if sp.epi == 'RESID':
        if sp.feat in ('resid_mapped', 'resid_mapped_few'):
            R = torch.zeros(M, N)
            src = torch.arange(M) if fault == 'resid_unmapped' else dest          # fault: the residual read at m, not at mo
            R[kept] = kw['C'][src[kept].clamp(0, case.T - 1)].float()
        else:
            R = kw['R'].float()
        x = x + R
    res = {}
    if sp.epi in ('BF16', 'RESID', 'F32'):
        res['C'] = x
    elif sp.epi == 'SILU':
        res['C silu'], res['C2 pre'] = F.silu(x), x
    elif sp.epi == 'GEGLU':
        is_gate = geglu_perm(N // 2)[0]
        a, gg = x[:, ~is_gate], x[:, is_gate]
        u = F.gelu(gg)
        d1 = 0.5 * (1 + torch.erf(gg * 2 ** -0.5)) + gg * torch.exp(-0.5 * gg * gg) * (2 * math.pi) ** -0.5
        sv = torch.empty_like(x); sv[:, ~is_gate] = u; sv[:, is_gate] = a * d1
        res['C saved [u|v]'], res['C2 hidden'] = sv, a * u
    elif sp.epi == 'GEGLU_BWD':
        is_gate = geglu_perm(N)[0]
        sv = kw['aux'].float()
        o = torch.empty(M, 2 * N); o[:, ~is_gate] = x * sv[:, ~is_gate]; o[:, is_gate] = x * sv[:, is_gate]
        res['C d[a|g]'] = o
    for o in case.outs:
        val = res[o.name].clone()
        rows = torch.arange(M)
        if fault == 'last_row_unwritten':
            rows = rows[:-1]
        elif fault == 'last_row_from_above' and M > 1:
            val[M - 1] = val[M - 2]
        w = kept[rows]
        o.view[dest[rows][w]] = val[rows][w].to(o.view.dtype)
        if fault == 'guard_column':               # one element at column N of the last row
            o.buf[GUARD + int(dest[kept][-1]), o.ncols] = 1.0
        if fault == 'dropped_row_written':
            named = set(dest[kept].tolist())
            free = next(r for r in range(case.T) if r not in named)
            o.view[free] = val[int((~kept).nonzero()[0])].to(o.view.dtype)
    return case


NT_FAULTS = ('last_row_unwritten', 'last_row_from_above', 'k_tile_dropped', 'bias_shifted', 'resid_unmapped', 'a2_boundary', 'guard_column', 'dropped_row_written')


def old_ratio(case):
    """the whole-matrix Frobenius ratios the old tests look at: each output as those tests see it (the rows x columns of the product; their buffers start
    from zeros, so an element that still holds the guard pattern counts as 0)"""
    out = []
    for o in case.outs:
        got = o.view[case.dest[case.kept]][:, :o.ncols]
        got = torch.where(_bits(got) == (FILL_BF16 if got.dtype == BF else FILL_F32), torch.zeros_like(got), got)
        out.append(relerr(got, o.ref[case.kept]))
    return out


# ---------------------------------------------------------------------------------------------- TN cases
class TN(NamedTuple):
    form: int                    # tfx_gemm_tn_plan's kind: -1 register-staged, 0 = 128 x 128, 2 = 256 x 256 / 8 waves, 3 = one wave per SIMD
    M: int
    N: int
    K: int
    splits: int = 1
    alpha: float = 1.0
    rowmap: bool = False         # permuted output rows with one drop
    kcut: int = 0                # k_valid = K - kcut
    colsum: bool = False
    k_group: int = 0
    lda_pad: int = 0             # lda = a_cols + lda_pad, ldb = b_cols + lda_pad (PAD in the padding)
    gather: bool = False         # row-gathered A and B
    seed: int = 0

    @property
    def name(self):
        return (f'tn{self.form} {self.M}x{self.N}x{self.K} splits={self.splits} alpha={self.alpha} rowmap={int(self.rowmap)} kcut={self.kcut} '
                f'colsum={int(self.colsum)} kg={self.k_group} pad={self.lda_pad} gather={int(self.gather)}')


# every C starts from random non-zero values (the kernels always accumulate).  M = 192 at 2 chunks has chunks under 192 rows: kind 2.
TN_CASES = [
    TN(-1, 100, 200, 136, 1, 0.5, True, 3, gather=True), TN(-1, 100, 64, 64, 3, gather=True, lda_pad=8),
    TN(0, 128, 200, 136, 1, 0.5, True, 3), TN(0, 128, 200, 136, 2, 1.0, True, 0, True), TN(0, 128, 200, 128, 2, k_group=8, lda_pad=8),
    TN(2, 128, 1024, 520, 1, 0.5, True, 3, lda_pad=8), TN(2, 128, 1000, 512, 1, 1.0, True, 0, True, 40), TN(2, 192, 1024, 520, 2),
    TN(3, 192, 1024, 520, 1, 0.5, True, 3), TN(3, 448, 1000, 520, 1, 1.0, True, 0, True), TN(3, 448, 1024, 520, 2, 1.0, False, 3, lda_pad=8),
    TN(3, 448, 1000, 512, 2, 1.0, False, 0, True, 40), TN(3, 192, 1000, 512, 1, k_group=8)]
# members of the two-product `group_next` chain (M = 448, 2 chunks) and of the three-record table (M = 512): different N, K, row maps and colsum
TN_CHAIN = [TN(3, 448, 520, 264, 2, seed=1), TN(3, 448, 300, 520, 2, rowmap=True, colsum=True, seed=2)]
TN_TABLE = [TN(3, 512, 264, 300, 0, seed=3), TN(3, 512, 520, 64, 0, k_group=40, seed=4), TN(3, 512, 300, 520, 0, rowmap=True, colsum=True, lda_pad=8, seed=5)]


def build_tn(spec, device='cpu'):
    """operands, tfx_gemm_tn_args keywords and the fp64 reference of one TN case (C and, with colsum, the folded bias gradient)"""
    M, N, K = spec.M, spec.N, spec.K
    g = torch.Generator(device='cpu').manual_seed(5000 + 1000 * spec.seed + M + 7 * N + 13 * K + spec.splits)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(device)
    ac, bc = (N + 7) // 8 * 8, (K + 7) // 8 * 8
    Msrc = M + 29 if spec.gather else M
    Abuf, Av = padded(rn(Msrc, ac, scale=0.5), spec.lda_pad)
    Bbuf, Bv = padded(rn(Msrc, bc, scale=0.5), spec.lda_pad)
    kv = K - spec.kcut
    kg = spec.k_group
    assert not kg or (K % 64 == 0 and spec.kcut == 0)
    Kout = K // 64 * kg if kg else K
    kw = dict(A=Av, lda=ac + spec.lda_pad, a_cols=ac, B=Bv, ldb=bc + spec.lda_pad, b_cols=bc, M=M, N=N, K=K, k_valid=kv, splits=spec.splits, accumulate=1,
              alpha=spec.alpha, k_group=kg)
    keep = [Abuf, Bbuf]
    Ae, Be = Av, Bv
    if spec.gather:
        am = torch.randint(0, Msrc, (M,), generator=g).to(torch.int32).to(device); bm = torch.randint(0, Msrc, (M,), generator=g).to(torch.int32).to(device)
        kw.update(a_rowmap=am, b_rowmap=bm); keep += [am, bm]
        Ae, Be = Av[am.long()], Bv[bm.long()]
    Ae, Be = Ae[:, :N].double(), Be[:, :K].double()
    dest = torch.arange(N)
    if spec.rowmap:
        dest = torch.randperm(N, generator=g)
        dest[3] = -1
        rmap = dest.to(torch.int32).to(device)
        kw.update(rowmap=rmap); keep.append(rmap)
    dest = dest.to(device)
    kept = dest >= 0
    Cbuf, Cv = guarded(N, Kout, torch.float32, device)
    Cv.copy_(torch.randn(N, Kout, generator=g).to(device))
    kw.update(C=Cv, ldc=Kout + GUARD)
    # product columns that are written, and where
    k = torch.arange(K, device=device)
    wk = (k < kv) & ((k % 64 < kg) if kg else torch.ones_like(k, dtype=torch.bool))
    ccol = ((k // 64) * kg + k % 64 if kg else k)[wk]
    init = torch.zeros(N, int(wk.sum()), dtype=torch.float64, device=device)
    init[kept] = Cv[dest[kept]][:, ccol].double()
    prod = (Ae.T @ Be)[:, wk]
    Sp = (Ae.abs().T @ Be.abs())[:, wk]
    x = spec.alpha * prod + init
    S = abs(spec.alpha) * Sp + init.abs()
    outs = [SimpleNamespace(name='C', buf=Cbuf, view=Cv, before=None, ref=x, tol=tol_f32(e32(M, S)), ncols=x.shape[1], cols=ccol)]
    for o in outs:
        o.before = o.buf.clone()
    case = SimpleNamespace(spec=spec, kw=kw, outs=outs, dest=dest, kept=kept, keep=keep, tile=TN_TILE[spec.form], Ae=Ae, Be=Be, wk=wk, ccol=ccol)
    if spec.colsum:                                                              # the bias gradient is a contiguous [N] vector: guards in front and behind
        assert spec.alpha == 1.0
        sb = torch.empty(N + 2 * GUARD, device=device)
        _bits(sb).fill_(FILL_F32)
        sb[GUARD:GUARD + N] = torch.randn(N, generator=g).to(device)
        kw.update(colsum=sb[GUARD:GUARD + N])
        binit = torch.zeros(N, dtype=torch.float64, device=device)
        binit[kept] = sb[GUARD:GUARD + N][dest[kept]].double()
        bref = Ae.sum(0) + binit
        bS = Ae.abs().sum(0) + binit.abs()
        case.colsum = SimpleNamespace(buf=sb, before=sb.clone(), ref=bref, tol=tol_f32(e32(M, bS)))
    return case


def check_tn(case):
    worst = check_case(case)
    cs = getattr(case, 'colsum', None)
    if cs is not None:
        kept, dest = case.kept, case.dest
        got = cs.buf[GUARD:GUARD + case.spec.N][dest[kept]]
        worst = max(worst, assert_elementwise(f'{case.spec.name} colsum', got[:, None], cs.ref[kept][:, None], cs.tol[kept][:, None], (case.tile[0], 1),
                                              rows=kept.nonzero().flatten()))
        written = torch.zeros_like(cs.buf, dtype=torch.bool)
        written[dest[kept] + GUARD] = True
        moved = (_bits(cs.buf) != _bits(cs.before)) & ~written
        assert not bool(moved.any()), f'{case.spec.name} colsum: entry {int(moved.nonzero()[0]) - GUARD} outside the named rows was written'
    return worst


def emulate_tn(case, fault=None):
    """a correct TN kernel on the CPU: fp32 product, alpha, added to C through the row map / k_valid / k_group; `fault`: one of TN_FAULTS"""
    sp = case.spec
    kept, dest = case.kept, case.dest
    prod = (case.Ae.float().T @ case.Be.float())[:, case.wk] * sp.alpha
    ccol = case.ccol
    o = case.outs[0]
    rows = dest[kept]
    o.view[rows[:, None], ccol[None, :]] += prod[kept]
    if fault == 'k_group_off_by_one':             # one 4-column store of the second group lands one group further
        kg = sp.k_group
        n0 = int(kept.nonzero()[-1])
        o.view[dest[n0], kg:kg + 4] -= prod[n0, kg:kg + 4]
        o.view[dest[n0], 2 * kg:2 * kg + 4] += prod[n0, kg:kg + 4]
    if sp.colsum:
        cs = case.colsum
        add = case.Ae.float().sum(0)
        if fault == 'colsum_twice':
            idx = kept.nonzero().flatten()
            j = idx[add[idx].abs().argsort()[idx.numel() // 2]]                  # the column of median magnitude
            add = add.clone(); add[j] *= 2
        cs.buf[GUARD:GUARD + sp.N][rows] += add[kept]
    return case


TN_FAULTS = ('k_group_off_by_one', 'colsum_twice')


def old_ratio_tn(case):
    o = case.outs[0]
    full_ref = o.before[GUARD:GUARD + case.spec.N, :o.view.shape[1]].double().clone()
    full_ref[case.dest[case.kept][:, None], case.ccol[None, :]] = o.ref[case.kept]
    r = [relerr(o.view, full_ref)]
    cs = getattr(case, 'colsum', None)
    if cs is not None:
        b = cs.before[GUARD:GUARD + case.spec.N].double().clone()
        b[case.dest[case.kept]] = cs.ref[case.kept]
        r.append(relerr(cs.buf[GUARD:GUARD + case.spec.N], b))
    return r
