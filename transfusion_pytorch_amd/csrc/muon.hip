// Muon for gfx950 (CDNA4): momentum + norm, grouped Newton-Schulz products, apply.   torch/optim/_muon.py:24-92, 258-293
//
// The Newton-Schulz iteration X <- a X + (b A + c A A) X, A = X X^T, is a chain of small bf16 GEMMs (m = 128 ... 1024): per matrix they fill a
// handful of CUs, so every product of one kind, over ALL matrices of the model, is ONE launch over a problem table - the launch count of a step
// does not depend on the depth.  One kernel serves the three products.  It is the NT form (both operands K-contiguous, as gemm.hip's):
//
//   gram    A  = X . X^T                       P = Q = X  (m x n)
//   poly    B  = b A + c A . A^T               P = Q = Z = A  (m x m; A is symmetric, so A . A^T is torch's A @ A)
//   update  X'^T = a X^T + X^T . B^T           P = Z = X^T (n x m), Q = B (B symmetric: torch's B @ X, transposed)
//
// so X is kept in both orientations: the update writes its tile to X'^T and, transposed, to X'.  Everything lives in a bf16 workspace whose
// matrices are zero-padded to multiples of the 128 x 128 tile: zero rows and columns stay zero under the iteration, so the padding is exact and
// the kernel needs no bounds predicate.  No atomics and no split sums anywhere: every output element is one fp32 MFMA accumulation chain in K
// order, the norms are two-level sums in a fixed order - the step is bit-deterministic (replicas of a data-parallel run orthogonalise the same
// all-reduced gradient redundantly and must stay identical).
#include "tfx_common.h"
#include "tfx_kernels.h"
#include "nt_ring.h"
#include <cmath>

namespace {

constexpr int BM = 128, BN = RING_BN, BK = RING_BK;
constexpr int PB = 64;                        // prep / apply walk the fp32 matrices in 64 x 64 blocks
constexpr int SUMSQ_DET_BLOCKS = TFX_SUMSQ_DET_PARTIALS;

// sum of a block's 256 per-thread values in a fixed order: DPP wave sums, then the 4 wave totals front to back (every thread gets the total)
TFX_DEV float block_sum256(float s, float* sacc) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sacc[threadIdx.x >> 6] = s;
  __syncthreads();
  const float tot = ((sacc[0] + sacc[1]) + sacc[2]) + sacc[3];
  __syncthreads();
  return tot;
}

// ------------------------------------------------------------------------------------------------
// grouped NT product: C = alpha sz Z + beta sa P . Q^T over a problem table; tile 128 x 128, 4 waves (2 x 2) of 64 x 64 = 2 x 2
// v_mfma_f32_32x32x16_bf16, operands staged by LDS-DMA into a 2-slot ring: nt_ring.h's K loop, as gemm.hip's glds form runs it, on operands that
// need no clamp.  Operands are multiplied swapped, so a lane owns one output row and runs of 4 columns.
// ------------------------------------------------------------------------------------------------
constexpr int GEMM_ST = 2;
__global__ __launch_bounds__(256, 2) void muon_gemm_kernel(const tfx_muon_gemm_problem* tab, const int32_t* tile_prob, int ntiles, float alpha, float beta) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int l = threadIdx.x & 63, hi = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int bid = xcd_remap(blockIdx.x, ntiles);
  const tfx_muon_gemm_problem p = tab[tile_prob[bid]];
  const int lt = bid - p.tile0;
  const int ntn = p.N / BN;
  const int m0 = (lt / ntn) * BM, n0 = (lt % ntn) * BN;

  const bf16 *ga[4], *gb[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int row = ring_src_row(w, j, 32), c = ring_src_chunk(row);
    ga[j] = p.P + (size_t)(m0 + row) * p.ldp + c * 8;
    gb[j] = p.Q + (size_t)(n0 + row) * p.ldq + c * 8;
  }
  f32x16 acc[2][2];
  nt_ring_loop<2, GEMM_ST, false>((bf16*)smem_raw, p.K / BK, acc, [&](int j, int k0) { return ga[j] + k0; }, [&](int j, int k0) { return gb[j] + k0; });

  // epilogue: accumulator register 4 g + e of acc[i][j] is row m_w + 32 i + (l & 31), column n_w + 32 j + 8 g + 4 hi + e
  const float sz = alpha * (p.scale_z ? *p.scale_z : 1.f), sa = beta * (p.scale_acc ? *p.scale_acc : 1.f);
  const int m_w = m0 + wm * 64, n_w = n0 + wn * 64;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int m = m_w + i * 32 + (l & 31);
    bf16x4 z[2][4];
    if (p.Z) {
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int g = 0; g < 4; g++) z[j][g] = *(const bf16x4*)(p.Z + (size_t)m * p.ldz + n_w + j * 32 + 8 * g + 4 * hi);
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int n = n_w + j * 32 + 8 * g + 4 * hi;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          float v = sa * acc[i][j][4 * g + e];
          if (p.Z) v = __builtin_fmaf(sz, bf2f(z[j][g][e]), v);
          o[e] = f2bf(v);
        }
        *(bf16x4*)(p.C + (size_t)m * p.ldc + n) = o;
        if (p.Ct) {
#pragma unroll
          for (int e = 0; e < 4; e++) p.Ct[(size_t)(n + e) * p.ldct + m] = o[e];
        }
      }
  }
}

// ------------------------------------------------------------------------------------------------
// prep: buf = lerp(buf, g, 1 - momentum); u = nesterov ? lerp(g, buf, momentum) : buf; bf16(u) into the workspace in both orientations; the
// block's sum of u^2 into partials[block].  g is the raw gradient times the step's clip coefficient (adam_k's formula).  One launch for all
// matrices: block b works on 64 x 64 block (b - blk0) of matrix blk_mat[b].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void muon_prep_kernel(tfx_muon_prep_args a) {
  __shared__ float tile[PB][PB + 1];
  __shared__ float sacc[4];
  const tfx_muon_mat mt = a.mats[a.blk_mat[blockIdx.x]];
  const int lb = blockIdx.x - mt.blk0;
  const int nbc = (mt.cols + PB - 1) / PB;
  const int r0 = (lb / nbc) * PB, c0 = (lb % nbc) * PB;
  const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6;
  float coef = a.grad_scale;
  if (a.max_norm > 0.f) {
    const float norm = sqrtf(a.sumsq[0]) * a.grad_scale;
    coef *= fminf(1.f, a.max_norm / (norm + 1e-6f));
  }
  const float w1 = 1.f - a.momentum;
  float ss = 0.f;
#pragma unroll 4
  for (int k = 0; k < PB / 4; k++) {
    const int r = r0 + tr + 4 * k, c = c0 + tc;
    float u = 0.f;
    if (r < mt.rows && c < mt.cols) {
      const size_t idx = (size_t)mt.off + (size_t)r * mt.cols + c;
      // rounded to fp32 BEFORE the mix, as clip_grad_norm_ leaves it for torch.lerp: contracted into the `g - b` below, the unrounded product moves a
      // cancelling lerp by thousands of ulp of its result (tests/test_param_kernels_gpu.py)
      float g;
      {
#pragma clang fp contract(off)
        g = a.g[idx] * coef;
      }
      float b = a.buf[idx];
      // torch.lerp(start, end, w): w < 0.5 ? start + w (end - start) : end - (end - start) (1 - w)
      b = w1 < 0.5f ? b + w1 * (g - b) : g - (g - b) * (1.f - w1);
      a.buf[idx] = b;
      u = b;
      if (a.nesterov) u = a.momentum < 0.5f ? g + a.momentum * (b - g) : b - (b - g) * (1.f - a.momentum);
      a.ws[(size_t)mt.s_off + (size_t)r * mt.ld_s + c] = f2bf(u);
    }
    tile[tr + 4 * k][tc] = u;
    ss = __builtin_fmaf(u, u, ss);
  }
  const float tot = block_sum256(ss, sacc);            // (its barriers also publish `tile`)
  if (threadIdx.x == 0) a.partials[blockIdx.x] = tot;
#pragma unroll 4
  for (int k = 0; k < PB / 4; k++) {
    const int c = c0 + tr + 4 * k, r = r0 + tc;
    if (r < mt.rows && c < mt.cols) a.ws[(size_t)mt.t_off + (size_t)c * mt.ld_t + r] = f2bf(tile[tc][tr + 4 * k]);
  }
}

// per matrix: s = max(sqrt(sum of its blocks' partials), eps); inv[2 i] = 1 / s, inv[2 i + 1] = 1 / s^2 (the first gram product and the first
// update carry them: X0 is stored unnormalised - bf16 keeps fp32's exponent range)
__global__ __launch_bounds__(256) void muon_norm_kernel(const tfx_muon_mat* mats, const float* partials, float eps, float* inv) {
  __shared__ float sacc[4];
  const tfx_muon_mat mt = mats[blockIdx.x];
  const int nb = ((mt.rows + PB - 1) / PB) * ((mt.cols + PB - 1) / PB);
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += partials[mt.blk0 + i];
  const float tot = block_sum256(s, sacc);
  if (threadIdx.x == 0) {
    const float r = 1.f / fmaxf(sqrtf(tot), eps);
    inv[2 * blockIdx.x] = r; inv[2 * blockIdx.x + 1] = r * r;
  }
}

// apply: p = p (1 - lr wd) - lr ratio O, O read from the straight-orientation copy of the final iterate
__global__ __launch_bounds__(256) void muon_apply_kernel(tfx_muon_apply_args a) {
  const tfx_muon_mat mt = a.mats[a.blk_mat[blockIdx.x]];
  const int lb = blockIdx.x - mt.blk0;
  const int nbc = (mt.cols + PB - 1) / PB;
  const int r0 = (lb / nbc) * PB, c0 = (lb % nbc) * PB;
  const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const float neg = -(a.lr * mt.lr_ratio);
#pragma unroll 4
  for (int k = 0; k < PB / 4; k++) {
    const int r = r0 + tr + 4 * k, c = c0 + tc;
    if (r < mt.rows && c < mt.cols) {
      const size_t idx = (size_t)mt.off + (size_t)r * mt.cols + c;
      const float o = bf2f(a.ws[(size_t)mt.s_off + (size_t)r * mt.ld_s + c]);
      a.p[idx] = __builtin_fmaf(neg, o, a.p[idx] * a.decay);
    }
  }
}

// sum of squares in a fixed order: block b sums its grid-stride share, one block then sums the partials front to back
__global__ __launch_bounds__(256) void sumsq_det_partial_k(const float* g, long long n, float* partials) {
  __shared__ float sacc[4];
  float s = 0.f;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 256 * 4) {
    if (i + 3 < n) { const f32x4 v = *(const f32x4*)(g + i); s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
    else for (long long j = i; j < n; j++) s += g[j] * g[j];
  }
  const float tot = block_sum256(s, sacc);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void sumsq_det_final_k(const float* partials, float* out) {
  __shared__ float sacc[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < SUMSQ_DET_BLOCKS; i += 256) s += partials[i];
  const float tot = block_sum256(s, sacc);
  if (threadIdx.x == 0) out[0] = tot;
}

int pad_to(int v, int q) { return (v + q - 1) / q * q; }

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define RET() return (int)hipGetLastError()

extern "C" {

int tfx_muon_plan(int32_t rows, int32_t cols, int32_t* flip, int32_t* m, int32_t* n, int32_t* m_pad, int32_t* n_pad, int32_t* gram_tiles,
                  int32_t* update_tiles, int32_t* prep_blocks) {
  if (rows <= 0 || cols <= 0) return -1;
  const int f = rows > cols;
  const int mm = f ? cols : rows, nn = f ? rows : cols;
  const int mp = pad_to(mm, BM), np = pad_to(nn, BM);
  if (flip) *flip = f;
  if (m) *m = mm;
  if (n) *n = nn;
  if (m_pad) *m_pad = mp;
  if (n_pad) *n_pad = np;
  if (gram_tiles) *gram_tiles = (mp / BM) * (mp / BN);
  if (update_tiles) *update_tiles = (np / BM) * (mp / BN);
  if (prep_blocks) *prep_blocks = ((rows + PB - 1) / PB) * ((cols + PB - 1) / PB);
  return 0;
}

int tfx_muon_step_launches(int32_t ns_steps, int32_t nmat) {
  if (ns_steps < 1 || nmat < 1) return -1;
  return 2 /* clip norm */ + 1 /* prep */ + 1 /* norms */ + 3 * ns_steps + 1 /* apply */ + 1 /* adam over the rest */;
}

int tfx_muon_gemm(const tfx_muon_gemm_problem* table, const int32_t* tile_prob, int32_t ntiles, float alpha, float beta, void* s) {
  if (ntiles == 0) return 0;
  if (!table || !tile_prob || ntiles < 0) return -1;
  const int smem = ring_bytes<2, GEMM_ST>;
  static uint32_t attr = 0;
  ensure_smem_attr((const void*)muon_gemm_kernel, smem, attr);
  hipLaunchKernelGGL(muon_gemm_kernel, dim3((unsigned)ntiles), dim3(256), smem, ST(s), table, tile_prob, (int)ntiles, alpha, beta); RET();
}

int tfx_muon_prep(const tfx_muon_prep_args* a, void* s) {
  if (a->nblk == 0) return 0;
  if (!a->mats || !a->blk_mat || !a->g || !a->buf || !a->ws || !a->partials || a->nblk < 0 || (a->max_norm > 0.f && !a->sumsq)) return -1;
  hipLaunchKernelGGL(muon_prep_kernel, dim3((unsigned)a->nblk), dim3(256), 0, ST(s), *a); RET();
}

int tfx_muon_norm(const tfx_muon_mat* mats, int32_t nmat, const float* partials, float eps, float* inv, void* s) {
  if (nmat == 0) return 0;
  if (!mats || !partials || !inv || nmat < 0) return -1;
  hipLaunchKernelGGL(muon_norm_kernel, dim3((unsigned)nmat), dim3(256), 0, ST(s), mats, partials, eps, inv); RET();
}

int tfx_muon_apply(const tfx_muon_apply_args* a, void* s) {
  if (a->nblk == 0) return 0;
  if (!a->mats || !a->blk_mat || !a->p || !a->ws || a->nblk < 0) return -1;
  hipLaunchKernelGGL(muon_apply_kernel, dim3((unsigned)a->nblk), dim3(256), 0, ST(s), *a); RET();
}

int tfx_sumsq_det(const float* g, int64_t n, float* partials, float* sumsq, void* s) {
  if (!g || !partials || !sumsq || n < 0) return -1;
  if (((uintptr_t)g) & 15) return -1;
  hipLaunchKernelGGL(sumsq_det_partial_k, dim3(SUMSQ_DET_BLOCKS), dim3(256), 0, ST(s), g, (long long)n, partials);
  hipLaunchKernelGGL(sumsq_det_final_k, dim3(1), dim3(256), 0, ST(s), partials, sumsq); RET();
}

}  // extern "C"
