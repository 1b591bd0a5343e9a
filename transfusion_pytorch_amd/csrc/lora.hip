// LoRA adapters (include/tfx.h "LoRA adapters"; transfusion_pytorch_amd/lora.py).
//
//   tfx_lora_merge   Weff = W + s B A in fp32, one fma chain per element (fixed order, no atomics): the source the bf16 shadow casts of an adapted
//                    matrix read, and what merge_lora_() copies into the master.  Runs once per optimizer step; exactness matters, speed does not.
//   tfx_lora_down    P[M, r_pad] = Q[M, K] . R[r_pad, K]^T   (U = X A^T and dU = dY B): skinny-N NT product, one wave per 32 rows of Q, all of R's rows per
//                    wave - Q is read once, R (<= 64 rows) comes from L2.
//   tfx_lora_grad    G[r, K] (+)= alpha P[M, r_pad]^T Q[M, K]   (dA and dB^T): skinny-N TN product.  A block owns 128 columns of Q and one run of rows, stages
//                    64-row tiles of P and Q in LDS (the staging and the transposed ds_read_b64_tr_b16 operand reads of gemm.hip's gemm_tn_kernel) and writes
//                    its fp32 partial with plain stores; a second kernel sums the runs in one fixed order.  The 128- and 256-wide tiles of the TN kernels
//                    would spend 2-4 x the MFMA work on an N of at most 64; here N is r_pad = 32 or 64.
// v_mfma_f32_32x32x16_bf16 operand maps (tfx_common.h, tools/probe_layouts.hip): lane l holds A[row l & 31][k = 8 (l >> 5) + e], B[k = 8 (l >> 5) + e][col l & 31],
// e = 0..7; D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
#include "tfx_common.h"
#include "tfx_kernels.h"

namespace tfx {

// ---------------------------------------------------------------------------------------------------- merge
__global__ __launch_bounds__(256) void lora_merge_kernel(tfx_lora_merge_args p) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)p.N * p.K) return;
  const int n = (int)(e / p.K), k = (int)(e - (int64_t)n * p.K);
  const float w = p.W[(size_t)n * p.ldw + k];
  float acc = 0.f;
  for (int j = 0; j < p.r; j++) acc = __builtin_fmaf(p.B[(size_t)n * p.ldb + j], p.A[(size_t)j * p.lda + k], acc);
  p.Weff[(size_t)n * p.ldo + k] = acc == 0.f ? w : __builtin_fmaf(p.s, acc, w);
}

// ---------------------------------------------------------------------------------------------------- down
template <int NT>
__global__ __launch_bounds__(256) void lora_down_kernel(tfx_lora_down_args p) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6, hi = l >> 5;
  const int row = blockIdx.x * 128 + w * 32 + (l & 31);
  const bool row_ok = row < p.M;
  const bf16* q = p.Q + (size_t)(row_ok ? row : 0) * p.ldq + 8 * hi;
  const bf16* r = p.R + (size_t)(l & 31) * p.ldr + 8 * hi;
  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[i][e] = 0.f;
  const u32x4 z = {0, 0, 0, 0};
  for (int k0 = 0; k0 < p.K; k0 += 16) {
    const bool k_ok = k0 + 8 * hi < p.K;                     // K % 8 == 0: a lane's 8 columns are inside or outside together
    const u32x4 a = (row_ok && k_ok) ? *(const u32x4*)(q + k0) : z;
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const u32x4 b = k_ok ? *(const u32x4*)(r + (size_t)i * 32 * p.ldr + k0) : z;
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc[i], 0, 0, 0);   // D[m][j]
    }
  }
  const int m0 = blockIdx.x * 128 + w * 32;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int m = m0 + (e & 3) + 8 * (e >> 2) + 4 * hi;
    if (m >= p.M) continue;
#pragma unroll
    for (int i = 0; i < NT; i++) p.P[(size_t)m * p.ldp + i * 32 + (l & 31)] = f2bf(acc[i][e]);
  }
}

// ---------------------------------------------------------------------------------------------------- grad
constexpr int LG_BM = 64;       // contraction rows per LDS tile
constexpr int LG_LQ = 136;      // LDS row stride of the Q tile (128 columns + 8: gemm.hip TN_LD)
constexpr int LG_LP = 72;       // LDS row stride of the P tile (<= 64 columns + 8)

struct LoraGradPlan { int ktiles, chunks, rows; };
static LoraGradPlan lora_grad_plan(int M, int K) {
  LoraGradPlan g;
  g.ktiles = (K + 127) / 128;
  const int most = (M + LG_BM - 1) / LG_BM;                // no run shorter than one LDS tile
  int want = 512 / g.ktiles;                               // two blocks per CU when the rows allow it
  if (want < 1) want = 1;
  int chunks = most < want ? most : want;
  if (chunks < 1) chunks = 1;
  g.rows = ((M + chunks - 1) / chunks + LG_BM - 1) / LG_BM * LG_BM;
  if (g.rows < LG_BM) g.rows = LG_BM;
  g.chunks = (M + g.rows - 1) / g.rows;
  if (g.chunks < 1) g.chunks = 1;
  return g;
}

template <int NT>
__global__ __launch_bounds__(256) void lora_grad_kernel(tfx_lora_grad_args p, int rows_per_chunk, int Kp) {
  __shared__ __attribute__((aligned(16))) bf16 Ps[2][LG_BM * LG_LP];
  __shared__ __attribute__((aligned(16))) bf16 Qs[2][LG_BM * LG_LQ];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, hi = l >> 5;
  const int k0 = blockIdx.x * 128, chunk = blockIdx.y;
  const int mbeg = chunk * rows_per_chunk;
  const int mend = mbeg + rows_per_chunk < p.M ? mbeg + rows_per_chunk : p.M;
  const int nsteps = (mend - mbeg + LG_BM - 1) / LG_BM;
  constexpr int PCH = NT * 4;                                // 16-byte chunks per row of the P tile
  u32x4 rq[4], rp[2];
  auto gload = [&](int st) {
    const int m0 = mbeg + st * LG_BM;
    const u32x4 z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = t + 256 * i, m = m0 + (c >> 4), col = k0 + (c & 15) * 8;
      rq[i] = (m < mend && col < p.K) ? *(const u32x4*)(p.Q + (size_t)m * p.ldq + col) : z;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int c = t + 256 * i;
      if (c < LG_BM * PCH) {
        const int m = m0 + c / PCH, col = (c % PCH) * 8;
        rp[i] = m < mend ? *(const u32x4*)(p.P + (size_t)m * p.ldp + col) : z;
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = t + 256 * i;
      *(u32x4*)(&Qs[buf][(c >> 4) * LG_LQ + (c & 15) * 8]) = rq[i];
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int c = t + 256 * i;
      if (c < LG_BM * PCH) *(u32x4*)(&Ps[buf][(c / PCH) * LG_LP + (c % PCH) * 8]) = rp[i];
    }
  };
  f32x16 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int e = 0; e < 16; e++) acc[i][e] = 0.f;
  if (nsteps > 0) {
    gload(0);
    sstore(0);
  }
  __syncthreads();
  for (int st = 0; st < nsteps; st++) {
    const int cur = st & 1;
    if (st + 1 < nsteps) gload(st + 1);
    const bf16* ps = Ps[cur];
    const bf16* qs = Qs[cur];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      const int r0 = ks * 16 + 8 * hi;
      const bf16x8 bq = lds_tr8(qs, LG_LQ, r0, r0 + 4, w * 32);
#pragma unroll
      for (int i = 0; i < NT; i++) {
        const bf16x8 ap = lds_tr8(ps, LG_LP, r0, r0 + 4, i * 32);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap, bq, acc[i], 0, 0, 0);          // D[j][k]
      }
    }
    if (st + 1 < nsteps) sstore(cur ^ 1);
    __syncthreads();
  }
  // the partial of (chunk, 128 columns): every (j < r_pad, k < Kp) element of the workspace is written by exactly one lane
  float* out = p.partials + (size_t)chunk * (NT * 32) * Kp + k0 + w * 32 + (l & 31);
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int j = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
      out[(size_t)j * Kp] = acc[i][e];
    }
}

// One thread per element of G.  The runs are added in ONE order, whatever the grid of the product kernel did: eight interleaved chains (run c joins chain
// c % 8, ascending) that close as a fixed tree - eight independent loads in flight per thread instead of one dependent chain of `chunks` loads.
__global__ __launch_bounds__(64) void lora_grad_sum_kernel(tfx_lora_grad_args p, int chunks, int Kp) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= (int64_t)p.r * p.K) return;
  const int j = (int)(e / p.K), k = (int)(e - (int64_t)j * p.K);
  const int c = p.colmap ? p.colmap[k] : k;
  if (c < 0) return;
  const float* src = p.partials + (size_t)j * Kp + k;
  const size_t step = (size_t)p.r_pad * Kp;
  float c8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int ch = 0;
  for (; ch + 8 <= chunks; ch += 8) {
#pragma unroll
    for (int u = 0; u < 8; u++) c8[u] += src[(size_t)(ch + u) * step];
  }
#pragma unroll
  for (int u = 0; u < 8; u++)
    if (ch + u < chunks) c8[u] += src[(size_t)(ch + u) * step];
  const float s = ((c8[0] + c8[1]) + (c8[2] + c8[3])) + ((c8[4] + c8[5]) + (c8[6] + c8[7]));
  float* g = p.G + (int64_t)j * p.g_row_stride + (int64_t)c * p.g_col_stride;
  const float v = p.alpha * s;
  *g = p.accumulate ? *g + v : v;
}

static bool aligned16(const void* x) { return ((uintptr_t)x & 15) == 0; }

}  // namespace tfx

extern "C" {

int tfx_lora_merge(const tfx_lora_merge_args* a, void* stream) {
  if (!a || !a->W || !a->Weff || a->N < 0 || a->K < 0 || a->r < 0 || a->r > 64) return -1;
  if (a->r > 0 && (!a->A || !a->B || a->ldb < a->r || a->lda < a->K)) return -2;
  if (a->ldw < a->K || a->ldo < a->K) return -3;
  const int64_t n = (int64_t)a->N * a->K;
  if (n == 0) return 0;
  hipLaunchKernelGGL(tfx::lora_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

int tfx_lora_down(const tfx_lora_down_args* a, void* stream) {
  if (!a || !a->Q || !a->R || !a->P || a->M < 0 || a->K <= 0) return -1;
  if (a->r_pad != 32 && a->r_pad != 64) return -2;
  if (a->K % 8 || a->ldq % 8 || a->ldr % 8 || a->ldq < a->K || a->ldr < a->K || a->ldp < a->r_pad) return -3;
  if (!tfx::aligned16(a->Q) || !tfx::aligned16(a->R)) return -4;
  if (a->M == 0) return 0;
  const dim3 grid((a->M + 127) / 128), block(256);
  if (a->r_pad == 32) hipLaunchKernelGGL(tfx::lora_down_kernel<1>, grid, block, 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(tfx::lora_down_kernel<2>, grid, block, 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

static int lora_grad_check(const tfx_lora_grad_args* a) {
  if (!a || a->M < 0 || a->K <= 0 || a->r < 1 || a->r > 64) return -1;
  if ((a->r_pad != 32 && a->r_pad != 64) || a->r > a->r_pad) return -2;
  if (a->K % 8 || a->ldq % 8 || a->ldp % 8 || a->ldq < a->K || a->ldp < a->r_pad) return -3;
  return 0;
}

int tfx_lora_grad_plan(const tfx_lora_grad_args* a, int32_t* chunks, int32_t* grid, int64_t* partial_floats) {
  const int rc = lora_grad_check(a);
  if (rc) return rc;
  const tfx::LoraGradPlan g = tfx::lora_grad_plan(a->M, a->K);
  if (chunks) *chunks = g.chunks;
  if (grid) *grid = g.ktiles * g.chunks;
  if (partial_floats) *partial_floats = (int64_t)g.chunks * a->r_pad * g.ktiles * 128;
  return 0;
}

int tfx_lora_grad(const tfx_lora_grad_args* a, void* stream) {
  const int rc = lora_grad_check(a);
  if (rc) return rc;
  if (!a->P || !a->Q || !a->G || !a->partials) return -4;
  if (!tfx::aligned16(a->Q) || !tfx::aligned16(a->P)) return -5;
  const tfx::LoraGradPlan g = tfx::lora_grad_plan(a->M, a->K);
  const int Kp = g.ktiles * 128;
  const dim3 grid(g.ktiles, g.chunks), block(256);
  if (a->r_pad == 32) hipLaunchKernelGGL(tfx::lora_grad_kernel<1>, grid, block, 0, (hipStream_t)stream, *a, g.rows, Kp);
  else hipLaunchKernelGGL(tfx::lora_grad_kernel<2>, grid, block, 0, (hipStream_t)stream, *a, g.rows, Kp);
  int e = (int)hipGetLastError();
  if (e) return e;
  const int64_t n = (int64_t)a->r * a->K;
  hipLaunchKernelGGL(tfx::lora_grad_sum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a, g.chunks, Kp);
  return (int)hipGetLastError();
}

}  // extern "C"
