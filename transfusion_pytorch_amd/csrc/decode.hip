// Decode-side kernels of `sample_many` (reference T:2082-2583): text-token sampling on the device and the ODE state update.
// Latency-bound (a handful of rows per step): one wave per row, no host round trip for the arithmetic.
#include "tfx_kernels.h"

namespace tfx {

// sample_text_token (T:597-605) + min_p_filter (T:591-595) for one row of fp32 logits per wave.
//   temperature == 0 : argmax over the V logits (first index on ties, like torch.argmax)
//   else             : p = softmax(logits / temperature); tokens with p < min_p * max(p) are removed; the survivor with
//                      cumulative mass crossing u * (total surviving mass) is drawn (inverse CDF in index order - the same
//                      distribution torch.multinomial samples from)
// When rounding leaves the target unreached (u close to 1: `mass` and the scan sum the same terms in different orders) the draw is the LAST survivor
// below V_draw, never a column outside the draw range.  When nothing survives below V_draw (V_draw < V, the maximum sits in a masked column and
// min-p removes every text token) the result is V_draw: the reference's masked logits are all -finfo.max there and its argmax takes the first (T:2697-2698).
__global__ __launch_bounds__(256) void sample_tokens_k(const float* logits, int ld, int B, int V, float temperature, float min_p, const float* uniforms,
                                                       const int* active, int* out_ids, int V_draw) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  if (active && !active[row]) return;
  const float* lg = logits + (size_t)row * ld;
  // pass 1: maximum and its first index
  float best = -__builtin_inff(); int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) { const float v = lg[c]; if (v > best) { best = v; bi = c; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (temperature == 0.f) { if (lane == 0) out_ids[row] = bi; return; }
  // pass 2: surviving mass.  p_c / p_max = exp((l_c - l_max) / T): the min-p test needs no normaliser
  const float it = 1.f / temperature;
  float mass = 0.f;
  for (int c = lane; c < V_draw; c += 64) { const float r = __expf((lg[c] - best) * it); mass += r >= min_p ? r : 0.f; }
  mass = wave_sum(mass);
  // pass 3: inverse CDF in index order, 64 columns per step with a wave prefix sum
  const float target = uniforms[row] * mass;
  float run = 0.f; int pick = -1, last = -1;            // last: the last survivor seen so far (the fallback when rounding leaves the target unreached)
  bool done = false;
  for (int c0 = 0; c0 < V_draw && !done; c0 += 64) {
    const int c = c0 + lane;
    float r = 0.f;
    if (c < V_draw) { r = __expf((lg[c] - best) * it); r = r >= min_p ? r : 0.f; }
    float pre = r;                                      // inclusive prefix sum across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(pre, o, 64); if (lane >= o) pre += t; }
    const bool hit = r > 0.f && run + pre > target;
    const unsigned long long m = __ballot(hit), alive = __ballot(r > 0.f);
    if (m) { pick = c0 + __builtin_ctzll(m); done = true; }
    else if (alive) last = c0 + 63 - __builtin_clzll(alive);
    run += __shfl(pre, 63, 64);
  }
  if (!done) pick = last >= 0 ? last : V_draw < V ? V_draw : bi;     // (V_draw == V and no survivor: min_p > 1 - the mode, as before)
  if (lane == 0) out_ids[row] = pick;
}

// ---- the draw behind top-k / top-p / min-p filters (tfx.h: tfx_sample_tokens_filtered) ----
// Every filter is a threshold: a column of the draw range survives when its logit key >= key_thr (top-k), the bit pattern of its r >= tau (top-p)
// and r >= min_p.  The two searches find key_thr and tau by 4 bits per pass over the row; the mass pass and the scan are those of sample_tokens_k
// with this membership test in place of `r >= min_p`.  NW waves share a row: 1 (four rows per 256-thread block) or 16 (one row per block).

// order-preserving integer key of an fp32 logit (-0 counts as +0: the two compare equal as floats)
TFX_DEV uint32_t logit_key(float v) {
  const uint32_t b = __builtin_bit_cast(uint32_t, v + 0.f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
// the one spelling of a column's r = p_c / p_max and of its membership, used by the threshold searches, the mass pass and the scan alike
TFX_DEV float sample_ratio(float l, float best, float it) { return __expf((l - best) * it); }
TFX_DEV bool sample_kept(float l, float r, uint32_t key_thr, uint32_t tau, float min_p) {
  return logit_key(l) >= key_thr && __builtin_bit_cast(uint32_t, r) >= tau && r >= min_p;
}

TFX_DEV int wave_sum_i(int v) {                          // wave_sum's DPP steps on integers
#define TFX_DPP_ADD_I(CTRL, ROWMASK) v += __builtin_amdgcn_update_dpp(0, v, CTRL, ROWMASK, 0xf, false)
  TFX_DPP_ADD_I(0xB1, 0xf); TFX_DPP_ADD_I(0x4E, 0xf); TFX_DPP_ADD_I(0x141, 0xf); TFX_DPP_ADD_I(0x140, 0xf);
  TFX_DPP_ADD_I(0x142, 0xa); TFX_DPP_ADD_I(0x143, 0xc);
#undef TFX_DPP_ADD_I
  return __builtin_amdgcn_readlane(v, 63);
}
TFX_DEV float wave_total(float v) { return wave_sum(v); }
TFX_DEV int wave_total(int v) { return wave_sum_i(v); }

// row total of a thread-strided partial: the wave tree, then (NW > 1) the waves' totals added in wave order.  sm: NW entries.
template <int NW> TFX_DEV float row_total(float v, float* sm) {
  v = wave_sum(v);
  if (NW == 1) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < NW; w++) tot += sm[w];
  __syncthreads();
  return tot;
}
// one search step: a[d], d = 1..15, are this thread's partials of a row quantity that does not grow with d; returns the largest d whose row
// total is >= bound, 0 when there is none.  Totals as in row_total.  sm: NW x 16 entries, digit: one shared word (both unused with NW == 1).
template <int NW, typename T> TFX_DEV int top_digit(const T (&a)[16], T bound, T* sm, int* digit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (NW == 1) {
    int dg = 0;
#pragma unroll
    for (int d = 1; d < 16; d++) if (wave_total(a[d]) >= bound) dg = d;
    return dg;
  }
#pragma unroll
  for (int d = 1; d < 16; d++) { const T s = wave_total(a[d]); if (lane == 0) sm[wave * 16 + d] = s; }
  __syncthreads();
  if (wave == 0) {
    const bool mine = lane >= 1 && lane < 16;
    T tot = 0;
    if (mine) for (int w = 0; w < NW; w++) tot += sm[w * 16 + lane];
    const unsigned long long m = __ballot(mine && tot >= bound);
    if (lane == 0) *digit = m ? 63 - __builtin_clzll(m) : 0;
  }
  __syncthreads();
  return *digit;
}

template <int NW>
__global__ __launch_bounds__(NW == 1 ? 256 : 64 * NW) void sample_tokens_filtered_k(const float* logits, int ld, int B, int V, int V_draw, float temperature,
                                                                                  float min_p, int top_k, float top_p, const float* uniforms,
                                                                                  const int* active, int* out_ids) {
  constexpr int TPR = 64 * NW;                           // threads per row
  __shared__ float sm_f[NW * 16];
  __shared__ int sm_i[NW * 16];
  __shared__ int sm_digit;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = NW == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  const int t0 = NW == 1 ? lane : threadIdx.x;           // this thread's first column
  if (row >= B) return;                                  // (uniform over the threads that share a row, hence over the block when NW > 1)
  if (active && !active[row]) return;
  const float* lg = logits + (size_t)row * ld;
  // pass 1: maximum over all V and its first index
  float best = -__builtin_inff(); int bi = 0x7fffffff;
  for (int c = t0; c < V; c += TPR) { const float v = lg[c]; if (v > best) { best = v; bi = c; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (NW > 1) {
    if (lane == 0) { sm_f[wave] = best; sm_i[wave] = bi; }
    __syncthreads();
    for (int w = 0; w < NW; w++) {
      const float ov = sm_f[w]; const int oi = sm_i[w];
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    __syncthreads();
  }
  if (temperature == 0.f) { if (lane == 0 && (NW == 1 || wave == 0)) out_ids[row] = bi; return; }
  const float it = 1.f / temperature;
  // top-k: key_thr = the k-th largest key of the draw range = the largest t with count(key >= t) >= k, 4 bits per pass from the top
  uint32_t key_thr = 0;
  if (top_k > 0 && top_k < V_draw) {
    for (int shift = 28; shift >= 0; shift -= 4) {
      int cnt[16] = {};
      for (int c = t0; c < V_draw; c += TPR) {
        const uint32_t k = logit_key(lg[c]);
#pragma unroll
        for (int d = 1; d < 16; d++) cnt[d] += k >= (key_thr | (uint32_t)d << shift) ? 1 : 0;
      }
      key_thr |= (uint32_t)top_digit<NW, int>(cnt, top_k, sm_i, &sm_digit) << shift;
    }
  }
  // top-p over the top-k survivors: G(x) = sum of r over survivors with bits(r) > x does not grow with x (fp32 addition in a fixed order is
  // monotone in every term); y = the largest x with G(x) >= top_p M, so the survivors are bits(r) > y, i.e. >= tau = y + 1.  r <= 1 keeps y below
  // the bit pattern of 1.  A row whose M or top_p M underflows to 0 is left unfiltered by top-p (nothing of it is drawn with r == 0 anyway).
  uint32_t tau = 0;
  if (top_p < 1.f) {
    float m = 0.f;
    for (int c = t0; c < V_draw; c += TPR) { const float l = lg[c]; m += logit_key(l) >= key_thr ? sample_ratio(l, best, it) : 0.f; }
    const float P = top_p * row_total<NW>(m, sm_f);
    if (P > 0.f) {
      uint32_t y = 0;
      for (int shift = 28; shift >= 0; shift -= 4) {
        float g[16] = {};
        for (int c = t0; c < V_draw; c += TPR) {
          const float l = lg[c], r = sample_ratio(l, best, it);
          const uint32_t rb = logit_key(l) >= key_thr ? __builtin_bit_cast(uint32_t, r) : 0u;      // (0 is above no threshold)
#pragma unroll
          for (int d = 1; d < 16; d++) g[d] += rb > (y | (uint32_t)d << shift) ? r : 0.f;
        }
        y |= (uint32_t)top_digit<NW, float>(g, P, sm_f, &sm_digit) << shift;
      }
      tau = y + 1;
    }
  }
  if (NW > 1 && wave != 0) return;                       // the draw is one wave's, in sample_tokens_k's order: filters off = its result to the bit
  // surviving mass, then the inverse CDF in index order, 64 columns per step with a wave prefix sum (sample_tokens_k's passes 2 and 3)
  float mass = 0.f;
  for (int c = lane; c < V_draw; c += 64) {
    const float l = lg[c], r = sample_ratio(l, best, it);
    mass += sample_kept(l, r, key_thr, tau, min_p) ? r : 0.f;
  }
  mass = wave_sum(mass);
  const float target = uniforms[row] * mass;
  float run = 0.f; int pick = -1, last = -1;
  bool done = false;
  for (int c0 = 0; c0 < V_draw && !done; c0 += 64) {
    const int c = c0 + lane;
    float r = 0.f;
    if (c < V_draw) { const float l = lg[c]; r = sample_ratio(l, best, it); r = sample_kept(l, r, key_thr, tau, min_p) ? r : 0.f; }
    float pre = r;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(pre, o, 64); if (lane >= o) pre += t; }
    const bool hit = r > 0.f && run + pre > target;
    const unsigned long long m = __ballot(hit), alive = __ballot(r > 0.f);
    if (m) { pick = c0 + __builtin_ctzll(m); done = true; }
    else if (alive) last = c0 + 63 - __builtin_clzll(alive);
    run += __shfl(pre, 63, 64);
  }
  if (!done) pick = last >= 0 ? last : V_draw < V ? V_draw : bi;
  if (lane == 0) out_ids[row] = pick;
}

// out = y + a * f with f = f_cond, or f_uncond + cfg * (f_cond - f_uncond) when f_uncond is given (classifier-free guidance, T:2516-2521)
__global__ void ode_axpy_k(const float* y, const float* fc, const float* fu, float cfg, float a, float* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float f = fc[i];
  if (fu) { const float u = fu[i]; f = u + cfg * (f - u); }
  out[i] = y[i] + a * f;
}

// per-sample solver state machine (tfx.h: tfx_ode_stage / tfx_ode_update): one thread per (sample, row, column < dl)
__global__ void ode_stage_k(const float* y, const float* ym, const float* ctl, int B, int Lc, int dmax, float* x, int H, int Lq, int dl, const int32_t* rows0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * Lc * dl) return;
  const int c = (int)(e % dl), j = (int)((e / dl) % Lc), i = (int)(e / ((long long)dl * Lc));
  const int mode = (int)ctl[i];
  if (mode == 0) return;
  const size_t src = ((size_t)i * Lc + j) * dmax + c;
  const float v = mode == 2 ? ym[src] : y[src];
  for (int h = 0; h < H; h++) {
    const int r0 = rows0 ? rows0[h * B + i] : (h * B + i) * Lq;
    if (r0 >= 0) x[((size_t)r0 + j) * dl + c] = v;
  }
}

__global__ void ode_update_k(float* y, float* ym, const float* ctl, int B, int Lc, int dmax, const float* pred, int H, int Lq, int dl, float cfg,
                             const float* sel, const int32_t* rows0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * Lc * dl) return;
  const int c = (int)(e % dl), j = (int)((e / dl) % Lc), i = (int)(e / ((long long)dl * Lc));
  const int mode = (int)ctl[i];
  if ((mode != 1 && mode != 2) || (sel && sel[i] == 0.f)) return;
  const int rc = rows0 ? rows0[i] : i * Lq;
  if (rc < 0) return;
  float f = pred[((size_t)rc + j) * dl + c];
  if (H == 2) {
    const int ru = rows0 ? rows0[B + i] : (B + i) * Lq;
    if (ru < 0) return;
    const float u = pred[((size_t)ru + j) * dl + c]; f = u + cfg * (f - u);
  }
  const size_t at = ((size_t)i * Lc + j) * dmax + c;
  const float r = y[at] + ctl[B + i] * f;
  if (mode == 1) ym[at] = r; else y[at] = r;
}

// ---- explicit Runge-Kutta tableaus of up to TFX_ODE_MAX_STAGES stages (tfx.h: tfx_ode_rk_stage / tfx_ode_rk_update / tfx_ode_rk_axpy) ----
// The arithmetic the header fixes, shared by the three kernels: fp32 from y, j ascending, one fmaf per term, a zero weight = the term is skipped and
// its k_j is not read; the guided derivative is one fmaf as well.
TFX_DEV float rk_guided(float f, float u, float cfg) { return fmaf(cfg, f - u, u); }
TFX_DEV float rk_accumulate(float acc, const float* k, size_t stride, int nk, const float* w) {
#pragma unroll
  for (int j = 0; j < TFX_ODE_MAX_STAGES - 1; j++)
    if (j < nk && w[j] != 0.f) acc = fmaf(w[j], k[(size_t)j * stride], acc);
  return acc;
}
TFX_DEV int rk_stage_index(float q) { const int v = (int)q; return v < 0 ? 0 : v > TFX_ODE_MAX_STAGES - 1 ? TFX_ODE_MAX_STAGES - 1 : v; }

struct RkWeights { float w[TFX_ODE_MAX_STAGES]; };

__global__ void ode_rk_axpy_k(const float* y, const float* k, long long k_stride, int nk, RkWeights w, const float* fc, const float* fu, float cfg,
                              float* k_out, float* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float g = fc[i];
  if (fu) g = rk_guided(g, fu[i], cfg);
  if (k_out) k_out[i] = g;
  if (out) out[i] = fmaf(w.w[nk], g, rk_accumulate(y[i], k + i, (size_t)k_stride, nk, w.w));
}

// one thread per (sample, row, column < dl), as ode_stage_k / ode_update_k.  ctl: [9][B] = mode, stage index, 3 stage weights, 4 update weights
__global__ void ode_rk_stage_k(const float* y, const float* k, const float* ctl, int B, int Lc, int dmax, float* x, int H, int Lq, int dl, const int32_t* rows0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * Lc * dl) return;
  const int c = (int)(e % dl), j = (int)((e / dl) % Lc), i = (int)(e / ((long long)dl * Lc));
  const int mode = (int)ctl[i];
  if (mode < 1 || mode > 3) return;
  bool any = false;
  for (int h = 0; h < H; h++) any |= (rows0 ? rows0[h * B + i] : 0) >= 0;
  if (!any) return;
  const size_t src = ((size_t)i * Lc + j) * dmax + c;
  float v = y[src];
  if (mode != 3) {
    const float wa[3] = {ctl[2 * B + i], ctl[3 * B + i], ctl[4 * B + i]};
    v = rk_accumulate(v, k + src, (size_t)B * Lc * dmax, rk_stage_index(ctl[B + i]), wa);
  }
  for (int h = 0; h < H; h++) {
    const int r0 = rows0 ? rows0[h * B + i] : (h * B + i) * Lq;
    if (r0 >= 0) x[((size_t)r0 + j) * dl + c] = v;
  }
}

__global__ void ode_rk_update_k(float* y, float* k, const float* ctl, int B, int Lc, int dmax, const float* pred, int H, int Lq, int dl, float cfg,
                                const float* sel, const int32_t* rows0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * Lc * dl) return;
  const int c = (int)(e % dl), j = (int)((e / dl) % Lc), i = (int)(e / ((long long)dl * Lc));
  const int mode = (int)ctl[i];
  if ((mode != 1 && mode != 2) || (sel && sel[i] == 0.f)) return;
  const int q = rk_stage_index(ctl[B + i]);
  if (mode == 1 && q >= TFX_ODE_MAX_STAGES - 1) return;      // a stage that is not the last has one of the k slots: anything else is skipped
  const int rc = rows0 ? rows0[i] : i * Lq;
  if (rc < 0) return;
  float g = pred[((size_t)rc + j) * dl + c];
  if (H == 2) {
    const int ru = rows0 ? rows0[B + i] : (B + i) * Lq;
    if (ru < 0) return;
    g = rk_guided(g, pred[((size_t)ru + j) * dl + c], cfg);
  }
  const size_t at = ((size_t)i * Lc + j) * dmax + c, stride = (size_t)B * Lc * dmax;
  if (mode == 1) { k[(size_t)q * stride + at] = g; return; }
  const float wb[3] = {ctl[5 * B + i], ctl[6 * B + i], ctl[7 * B + i]};
  y[at] = fmaf(ctl[(5 + q) * B + i], g, rk_accumulate(y[at], k + at, stride, q, wb));
}

// ---- Adams-Bashforth multistep rules on top of the tableau kernels (tfx.h: tfx_ode_ab_axpy / tfx_ode_ab_update) ----
// History terms in table order after the k terms, one fmaf each, a zero weight = the term is skipped and its slot is not read; the g term last.
TFX_DEV int ab_slot_index(float s) { const int v = (int)s; return v < 0 ? 0 : v > TFX_ODE_AB_HIST - 1 ? TFX_ODE_AB_HIST - 1 : v; }

struct AbHistory { const float* h[TFX_ODE_AB_HIST]; float w[TFX_ODE_AB_HIST]; };

__global__ void ode_ab_axpy_k(const float* y, AbHistory hs, float wg, const float* fc, const float* fu, float cfg, float* g_out, float* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float g = fc[i];
  if (fu) g = rk_guided(g, fu[i], cfg);
  float acc = y[i];
#pragma unroll
  for (int j = 0; j < TFX_ODE_AB_HIST; j++)
    if (hs.w[j] != 0.f) acc = fmaf(hs.w[j], hs.h[j][i], acc);
  out[i] = fmaf(wg, g, acc);                                 // every read of element i is done: g_out may be one of the h_j
  if (g_out) g_out[i] = g;
}

// ode_rk_update_k with the history ring.  ctl: [16][B] = the 9 rows of ode_rk_update_k, the slot that receives g, 3 slots read, their 3 weights
__global__ void ode_ab_update_k(float* y, float* k, float* hist, const float* ctl, int B, int Lc, int dmax, const float* pred, int H, int Lq, int dl,
                                float cfg, const float* sel, const int32_t* rows0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * Lc * dl) return;
  const int c = (int)(e % dl), j = (int)((e / dl) % Lc), i = (int)(e / ((long long)dl * Lc));
  const int mode = (int)ctl[i];
  if ((mode != 1 && mode != 2) || (sel && sel[i] == 0.f)) return;
  const int q = rk_stage_index(ctl[B + i]);
  if (mode == 1 && q >= TFX_ODE_MAX_STAGES - 1) return;
  const int rc = rows0 ? rows0[i] : i * Lq;
  if (rc < 0) return;
  float g = pred[((size_t)rc + j) * dl + c];
  if (H == 2) {
    const int ru = rows0 ? rows0[B + i] : (B + i) * Lq;
    if (ru < 0) return;
    g = rk_guided(g, pred[((size_t)ru + j) * dl + c], cfg);
  }
  const size_t at = ((size_t)i * Lc + j) * dmax + c, stride = (size_t)B * Lc * dmax;
  const float to = ctl[9 * B + i];
  float* keep = to >= 0.f ? hist + (size_t)ab_slot_index(to) * stride + at : nullptr;
  if (mode == 1) { k[(size_t)q * stride + at] = g; if (keep) *keep = g; return; }
  const float wb[3] = {ctl[5 * B + i], ctl[6 * B + i], ctl[7 * B + i]};
  float acc = rk_accumulate(y[at], k + at, stride, q, wb);
#pragma unroll
  for (int s = 0; s < TFX_ODE_AB_HIST; s++) {
    const float w = ctl[(13 + s) * B + i];
    if (w != 0.f) acc = fmaf(w, hist[(size_t)ab_slot_index(ctl[(10 + s) * B + i]) * stride + at], acc);
  }
  y[at] = fmaf(ctl[(5 + q) * B + i], g, acc);                // every read of the element is done: `keep` may be a slot just read
  if (keep) *keep = g;
}

// R x C block of a fp32 matrix -> bf16 block of another matrix (8 elements per thread)
__global__ void cast_block_k(const float* src, int ld_src, bf16* dst, int ld_dst, int R, int C8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)R * C8) return;
  const int r = (int)(i / C8), c = (int)(i % C8) * 8;
  const f32x4 a = *(const f32x4*)(src + (size_t)r * ld_src + c), b = *(const f32x4*)(src + (size_t)r * ld_src + c + 4);
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; e++) { o[e] = f2bf(a[e]); o[4 + e] = f2bf(b[e]); }
  *(bf16x8*)(dst + (size_t)r * ld_dst + c) = o;
}

__global__ void scale_copy_k(const bf16* src, bf16* dst, long long n, float sc) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i + 7 < n) {
    bf16x8 v = *(const bf16x8*)(src + i);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = f2bf(bf2f(v[e]) * sc);
    *(bf16x8*)(dst + i) = v;
  } else for (long long j = i; j < n; j++) dst[j] = f2bf(bf2f(src[j]) * sc);
}


// Decode attention (reference score pipeline T:998-1027 against the KV cache T:1005-1016): one BLOCK per (sample, head) for up to R = 8 NEW query
// rows of the sample (instantiated for R = 1, 2: text steps), its four waves walk the visible keys 32 at
// a time.  Lane = (key group g = lane / 8, dim slice sl = lane % 8): per trip a wave takes 8 keys, every lane 8 of the 64 dims of its key (16-byte
// loads: a key row is 8 lanes x 16 B, contiguous) - loaded ONCE for all rows - and per row the partial dots meet with three DPP steps, then soft-cap
// (exact tanh - a handful of scores per lane), exp2 against the FIXED reference 0 (|cap * log2e * tanh| <= 72: no running maximum needed, as in
// the training kernel), and the value row joins the row's per-lane accumulator.  The 32 key groups are summed through LDS; out = o / l *
// sigmoid(gate).  A row's arithmetic does not depend on R or on the other rows of its block (keys past its own visible length add exact zeros in
// the same order), so a token comes out the same whichever plan carried it.
template <int R>
__global__ __launch_bounds__(256) void decode_attn_rows_k(tfx_attn_args p) {
  extern __shared__ float red_raw[];                       // [R][wave * 8 + key group][dim slice][8 dims + l]
  float (*red)[32][8][9] = (float (*)[32][8][9])red_raw;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 3, sl = lane & 7;
  const int b = blockIdx.x / p.h, h = blockIdx.x % p.h;
  const int t0 = b * p.n;
  int kve[R], kmax = 1;
  float q8[R][8], o8[R][8], l[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    kve[r] = r < p.n ? min(p.kv_end[t0 + r], p.n_kv) : 0;
    kmax = max(kmax, kve[r]);
    bf16x8 qv;
    if (r < p.n) qv = *(const bf16x8*)(p.q + (size_t)(t0 + r) * p.ld_q + h * 64 + sl * 8);
#pragma unroll
    for (int e = 0; e < 8; e++) { q8[r][e] = r < p.n ? bf2f(qv[e]) : 0.f; o8[r][e] = 0.f; }
    l[r] = 0.f;
  }
  const bf16* kb = p.k + (size_t)b * p.n_kv * p.ld_k + h * 64 + sl * 8;
  const bf16* vb = p.v + (size_t)b * p.n_kv * p.ld_v + h * 64 + sl * 8;
  const float icap = 1.f / p.softcap, cap2 = p.softcap * 1.4426950408889634f;
#pragma unroll 2
  for (int j0 = wv * 8; j0 < kmax; j0 += 32) {
    const int j = j0 + g;
    const int jc = min(j, kmax - 1);
    const bf16x8 kv = *(const bf16x8*)(kb + (size_t)jc * p.ld_k);
    const bf16x8 vv = *(const bf16x8*)(vb + (size_t)jc * p.ld_v);
    float kf[8], vf[8];
#pragma unroll
    for (int e = 0; e < 8; e++) { kf[e] = bf2f(kv[e]); vf[e] = bf2f(vv[e]); }
#pragma unroll
    for (int r = 0; r < R; r++) {
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) dot = __builtin_fmaf(q8[r][e], kf[e], dot);
      dot = group8_sum(dot);
      const float x = dot * icap;
      const float th = 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * (2.f * 1.4426950408889634f)));   // tanh(x)
      const float pj = j < kve[r] ? __builtin_amdgcn_exp2f(cap2 * th) : 0.f;
      l[r] += pj;
#pragma unroll
      for (int e = 0; e < 8; e++) o8[r][e] = __builtin_fmaf(pj, vf[e], o8[r][e]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
#pragma unroll
    for (int e = 0; e < 8; e++) red[r][wv * 8 + g][sl][e] = o8[r][e];
    red[r][wv * 8 + g][sl][8] = l[r];
  }
  __syncthreads();
  if (threadIdx.x < 8 * R && (int)(threadIdx.x >> 3) < p.n) {
    const int r = threadIdx.x >> 3, s2 = threadIdx.x & 7, t = t0 + r;
    // (kernel argument: uniform) gate == NULL = no value gating: sigmoid(+inf) = 1 exactly.  The branch sits AHEAD of the reduction loop: behind it
    // hipcc unrolled the loop into 288 LDS reads in flight (256 VGPRs + 48 AGPRs, one wave per SIMD instead of eight)
    float gate = INFINITY;
    if (p.gate) gate = bf2f(p.gate[(size_t)t * p.ld_gate + h]);
    float o[8], lt = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = 0.f;
    for (int gg = 0; gg < 32; gg++) {
#pragma unroll
      for (int e = 0; e < 8; e++) o[e] += red[r][gg][s2][e];
      lt += red[r][gg][s2][8];
    }
    const float gs = __builtin_amdgcn_rcpf(1.f + __expf(-gate));
    bf16x8 ov;
    if (p.laser) {                                         // LASER (T:1019-1022): `v` is the side cache of v' = exp(softclamp(v)); og = g log(o / l)
      const float rl = 1.f / lt;
#pragma unroll
      for (int e = 0; e < 8; e++) ov[e] = f2bf(gs * __logf(o[e] * rl));
    } else {
      const float sc = gs / lt;
#pragma unroll
      for (int e = 0; e < 8; e++) ov[e] = f2bf(o[e] * sc);
    }
    *(bf16x8*)(p.out + (size_t)t * p.ld_out + h * 64 + s2 * 8) = ov;
    if (p.lse && s2 == 0) p.lse[((size_t)b * p.h + h) * p.n + r] = __logf(lt);
  }
}

template <int R> static int launch_decode_rows(const tfx_attn_args& a, hipStream_t s) {
  static uint32_t attr = 0;
  const int smem = R * 32 * 8 * 9 * 4;
  ensure_smem_attr((const void*)decode_attn_rows_k<R>, smem, attr);
  hipLaunchKernelGGL(decode_attn_rows_k<R>, dim3((unsigned)(a.b * a.h)), dim3(256), smem, s, a);
  return (int)hipGetLastError();
}
}  // namespace tfx
using namespace tfx;

extern "C" {
int tfx_sample_tokens(const float* logits, int32_t ld, int32_t B, int32_t V, float temperature, float min_p, const float* uniforms,
                      const int32_t* active, int32_t* out_ids, void* s) {
  if (B <= 0) return 0;
  if (!logits || !out_ids || V <= 0 || ld < V) return -1;
  if (temperature != 0.f && !uniforms) return -2;
  if (temperature < 0.f) return -3;
  hipLaunchKernelGGL(sample_tokens_k, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)s, logits, ld, B, V, temperature, min_p, uniforms, active, out_ids, V);
  return (int)hipGetLastError();
}
int tfx_sample_tokens_range(const float* logits, int32_t ld, int32_t B, int32_t V, int32_t V_draw, float temperature, float min_p, const float* uniforms,
                            const int32_t* active, int32_t* out_ids, void* s) {
  if (B <= 0) return 0;
  if (!logits || !out_ids || V <= 0 || V_draw <= 0 || V_draw > V || ld < V || (temperature != 0.f && !uniforms)) return -1;
  if (temperature < 0.f) return -3;
  hipLaunchKernelGGL(sample_tokens_k, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)s, logits, ld, B, V, temperature, min_p, uniforms, active, out_ids, V_draw);
  return (int)hipGetLastError();
}
int tfx_sample_tokens_filtered(const float* logits, int32_t ld, int32_t B, int32_t V, int32_t V_draw, float temperature, float min_p, int32_t top_k,
                               float top_p, const float* uniforms, const int32_t* active, int32_t* out_ids, void* s) {
  if (temperature < 0.f || top_k < 0 || !(top_p > 0.f) || V_draw < 1 || V_draw > V) return -3;
  if (B <= 0) return 0;
  if (!logits || !out_ids || ld < V || (temperature != 0.f && !uniforms)) return -1;
  if (V <= TFX_SAMPLE_NARROW_MAX)
    hipLaunchKernelGGL(sample_tokens_filtered_k<1>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)s, logits, ld, B, V, V_draw, temperature, min_p, top_k,
                       top_p, uniforms, active, out_ids);
  else
    hipLaunchKernelGGL(sample_tokens_filtered_k<16>, dim3(B), dim3(1024), 0, (hipStream_t)s, logits, ld, B, V, V_draw, temperature, min_p, top_k, top_p,
                       uniforms, active, out_ids);
  return (int)hipGetLastError();
}
int tfx_ode_axpy(const float* y, const float* f_cond, const float* f_uncond, float cfg_scale, float a, float* out, int64_t n, void* s) {
  if (n <= 0) return 0;
  if (!y || !f_cond || !out) return -1;
  hipLaunchKernelGGL(ode_axpy_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, f_cond, f_uncond, cfg_scale, a, out, (long long)n);
  return (int)hipGetLastError();
}
int tfx_ode_stage(const float* y, const float* ym, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, float* x, int32_t H, int32_t Lq, int32_t dl,
                  const int32_t* rows0, void* s) {
  if (B <= 0 || Lc <= 0 || dl <= 0) return 0;
  if (!y || !ym || !ctl || !x || H < 1 || H > 2 || Lq < Lc || dl > dmax) return -1;
  const long long n = (long long)B * Lc * dl;
  hipLaunchKernelGGL(ode_stage_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, ym, ctl, B, Lc, dmax, x, H, Lq, dl, rows0);
  return (int)hipGetLastError();
}
int tfx_ode_update(float* y, float* ym, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq, int32_t dl,
                   float cfg_scale, const float* sel, const int32_t* rows0, void* s) {
  if (B <= 0 || Lc <= 0 || dl <= 0) return 0;
  if (!y || !ym || !ctl || !pred || H < 1 || H > 2 || Lq < Lc || dl > dmax) return -1;
  const long long n = (long long)B * Lc * dl;
  hipLaunchKernelGGL(ode_update_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, ym, ctl, B, Lc, dmax, pred, H, Lq, dl, cfg_scale, sel, rows0);
  return (int)hipGetLastError();
}
int tfx_ode_rk_axpy(const float* y, const float* k, int64_t k_stride, int32_t nk, float w0, float w1, float w2, float w3, const float* f_cond,
                    const float* f_uncond, float cfg_scale, float* k_out, float* out, int64_t n, void* s) {
  if (n <= 0) return 0;
  if (!y || !f_cond || (!out && !k_out)) return -1;
  if (nk < 0 || nk > TFX_ODE_MAX_STAGES - 1) return -2;
  if (nk > 0 && (!k || k_stride < n)) return -3;
  const tfx::RkWeights w = {{w0, w1, w2, w3}};
  hipLaunchKernelGGL(ode_rk_axpy_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, k, (long long)k_stride, nk, w, f_cond, f_uncond,
                     cfg_scale, k_out, out, (long long)n);
  return (int)hipGetLastError();
}
int tfx_ode_rk_stage(const float* y, const float* k, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, float* x, int32_t H, int32_t Lq, int32_t dl,
                     const int32_t* rows0, void* s) {
  if (B <= 0 || Lc <= 0 || dl <= 0) return 0;
  if (!y || !k || !ctl || !x || H < 1 || H > 2 || Lq < Lc || dl > dmax) return -1;
  const long long n = (long long)B * Lc * dl;
  hipLaunchKernelGGL(ode_rk_stage_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, k, ctl, B, Lc, dmax, x, H, Lq, dl, rows0);
  return (int)hipGetLastError();
}
int tfx_ode_rk_update(float* y, float* k, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq, int32_t dl,
                      float cfg_scale, const float* sel, const int32_t* rows0, void* s) {
  if (B <= 0 || Lc <= 0 || dl <= 0) return 0;
  if (!y || !k || !ctl || !pred || H < 1 || H > 2 || Lq < Lc || dl > dmax) return -1;
  const long long n = (long long)B * Lc * dl;
  hipLaunchKernelGGL(ode_rk_update_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, k, ctl, B, Lc, dmax, pred, H, Lq, dl, cfg_scale, sel, rows0);
  return (int)hipGetLastError();
}
int tfx_ode_ab_axpy(const float* y, const float* h0, const float* h1, const float* h2, float w0, float w1, float w2, float wg, const float* f_cond,
                    const float* f_uncond, float cfg_scale, float* g_out, float* out, int64_t n, void* s) {
  if (n <= 0) return 0;
  if (!y || !f_cond || !out) return -1;
  const tfx::AbHistory hs = {{h0, h1, h2}, {w0, w1, w2}};
  for (int j = 0; j < TFX_ODE_AB_HIST; j++)
    if (hs.w[j] != 0.f && !hs.h[j]) return -3;
  hipLaunchKernelGGL(ode_ab_axpy_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, hs, wg, f_cond, f_uncond, cfg_scale, g_out, out,
                     (long long)n);
  return (int)hipGetLastError();
}
int tfx_ode_ab_update(float* y, float* k, float* hist, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq,
                      int32_t dl, float cfg_scale, const float* sel, const int32_t* rows0, void* s) {
  if (B <= 0 || Lc <= 0 || dl <= 0) return 0;
  if (!y || !k || !hist || !ctl || !pred || H < 1 || H > 2 || Lq < Lc || dl > dmax) return -1;
  const long long n = (long long)B * Lc * dl;
  hipLaunchKernelGGL(ode_ab_update_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, y, k, hist, ctl, B, Lc, dmax, pred, H, Lq, dl, cfg_scale,
                     sel, rows0);
  return (int)hipGetLastError();
}
int tfx_scale_bf16_copy(const tfx_bf16* src, tfx_bf16* dst, int64_t n, float scale, void* s) {
  if (n <= 0) return 0;
  if (!src || !dst) return -1;
  hipLaunchKernelGGL(scale_copy_k, dim3((unsigned)((n / 8 + 256) / 256)), dim3(256), 0, (hipStream_t)s, src, dst, (long long)n, scale);
  return (int)hipGetLastError();
}
int tfx_cast_block_bf16(const float* src, int32_t ld_src, tfx_bf16* dst, int32_t ld_dst, int32_t R, int32_t C, void* s) {
  if (R <= 0 || C <= 0) return 0;
  if (!src || !dst || (C | ld_src | ld_dst) % 8 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return -1;
  const long long n = (long long)R * (C / 8);
  hipLaunchKernelGGL(cast_block_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, src, ld_src, dst, ld_dst, R, C / 8);
  return (int)hipGetLastError();
}
/* the K13 name of SURVEY 8(b): attention of a short block of NEW query rows per sample against keys / values that live in a KV cache
 * (`n_kv` > 0 rows per sample, per-row visible length in `kv_end`; the rows of a sample need not be ordered by visible length). */
int tfx_decode_attn(const tfx_attn_args* a, void* s) {
  if (!a || a->n_kv <= 0) return -10;
  if ((long long)a->b * a->h == 0 || a->n <= 0) return 0;
  // one or two rows per sample (text steps): the multi-row kernel; from there on the tiled forward kernel with its cache addressing is the faster
  // one - both read the layer's whole KV cache and are HBM-bound (86 MB per launch at 128 cache rows x 330 keys: 21.6 us for five rows per sample
  // here against 18.9 us there, rocprofv3 inside the continuous decode loop).  The multi-row kernel addresses the dense layout (rows b * n ..): a
  // compacted call (q_row0 / q_cnt) goes to the tiled kernel, which takes the row ranges, whatever n is
  const bool dense = !a->q_row0 && !a->q_cnt;
  if (dense && a->n == 1) return tfx::launch_decode_rows<1>(*a, (hipStream_t)s);
  if (dense && a->n == 2) return tfx::launch_decode_rows<2>(*a, (hipStream_t)s);
  return tfx::attn_fwd(*a, (hipStream_t)s);
}
}
