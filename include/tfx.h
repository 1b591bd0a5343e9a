/* tfx.h — C ABI of libtfx_hip.so: the MI355X (gfx950) Transfusion hot path.
 *
 * Plain C: raw device pointers, sizes, a hipStream_t passed as void*.  No torch types.
 * Every entry point enqueues work on `stream` and returns immediately (no host sync);
 * return value 0 = ok, non-zero = argument / launch error (hipError_t or negative code).
 * bf16 tensors are `uint16_t*` storage here (`__bf16` on the device).
 *
 * Reference interfaces replaced (file:line relative to /root/reference/transfusion_pytorch;
 * T = transfusion.py, MP = modality_processing.py):
 *
 *   tfx_gemm_nt / tfx_gemm_tn    every nn.Linear on the path and its backward: to_qk/to_v/to_gates/to_out
 *                                T:877-916, FeedForward T:845-853 (GEGLU epilogue T:831-834), skip_proj
 *                                T:1083,1214-1219, to_time_cond T:1068-1072, to_film/to_ada_ln_zero T:664-665,
 *                                latent_to_model / model_to_latent T:1478-1479, to_text_logits T:1507
 *   tfx_attn_fwd/_bwd_*          Attention.forward score pipeline T:998-1027 (softclamp T:280-281, mask
 *                                naive_attn_mask T:452-470 in prefix-extension form, sigmoid value gate T:1027)
 *   tfx_qk_norm_rope_*           q_norm/k_norm RMSNorm T:950-952,779-786 + apply_rotary_emb T:965 + q*scale T:998
 *   tfx_adaln_pre_* / _post_*    AdaptiveWrapper.forward T:721-775
 *   tfx_attnres_*                AttentionResidual.forward T:807-829
 *   tfx_rmsnorm_*                RMSNorm T:779-786 (final norm T:1250)
 *   tfx_embed_*                  text_embed gather + einx.where select T:3173-3184
 *   tfx_noise_mix                process_type_flat noising MP:654-656
 *   tfx_fourier                  RandomFourierEmbed T:617-635
 *   tfx_ce_* / tfx_mse_*         loss block T:3320-3376
 *   tfx_adam_*                   train_toy.py:55-57 (clip_grad_norm_ + Adam)
 *   tfx_muon_* / tfx_sumsq_det   the optimizer over Transfusion.muon_parameters() T:1657-1672 (train_image_only.py:90); the rule is
 *                                torch.optim.Muon's: torch/optim/_muon.py:24-92 (Newton-Schulz, lr adjustment), 258-293 (momentum, update)
 */
#ifndef TFX_H
#define TFX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#ifndef TFX_BF16_DEFINED
typedef uint16_t tfx_bf16;
#endif

/* ---- GEMM ------------------------------------------------------------------------------------ */
enum { TFX_EPI_BF16 = 0, TFX_EPI_F32 = 1, TFX_EPI_SILU = 2, TFX_EPI_RESID = 3, TFX_EPI_GEGLU = 4, TFX_EPI_GEGLU_BWD = 5, TFX_EPI_QKV_NORM_ROPE = 6 };

/* C[M,N] = A[M,K] . B[N,K]^T (+ epilogue).  K % 64 == 0; lda/ldb % 8 == 0; all bases 16-byte aligned.
 * Optional second A source A2 for k >= K1 (skip-proj concat without the cat copy, T:1214-1219).
 * a_rowmap: gather A rows (row index = a_rowmap[m]); rowmap: scatter output rows (negative = drop).
 * GEGLU layout: physical column c of the 2*dip-wide [value|gate] buffer: block j = c/64, c%64 < 32 is
 * value feature j*32 + c%32, else gate feature j*32 + c%64-32 (weights/bias shadows use the same order).
 * TFX_EPI_GEGLU (FeedForward T:845-853, GEGLU T:831-834): with a | g = acc + bias in that layout, C2 (ldc2 = dip) receives h = a gelu(g) and C (ldc = 2 dip)
 * receives what the backward needs, in the same layout: u = gelu(g) in the value slots and v = a gelu'(g) in the gate slots (round 5; the round-1..4 form
 * stored the pre-activations a | g).  TFX_EPI_GEGLU_BWD: acc = dh (N = dip), aux = that saved [u|v]; C (ldc = 2 dip) receives d[a|g] = dh u | dh v.
 * bias: the epilogues read it as whole f32x4 groups, the ragged last group of N % 4 != 0 included (add_bias of the register-staged kernel), so it must be
 * READABLE up to ceil(N / 4) * 4 floats and 16-byte aligned; what lies behind N is never used.  (ParamStore pads every segment to 4 floats for this.)
 * ldc / ldc2 (and ldr, ldaux): in elements, any value >= the written width (N; 2 N for GEGLU_BWD).  Multiples of 4 keep every bf16x4 (8-byte) / f32x4
 * (16-byte) store and side load of the epilogues naturally aligned; the staged 16-byte row stores of the LDS-DMA and 256 x 256 kernels, the persistent
 * one-wave kernel (plan kind 7) and the fused QKV_NORM_ROPE epilogue need ldc % 8 == 0 (ldc2 likewise), N % 8 == 0 and a 16-byte aligned C - without them the
 * launch takes the direct-store epilogue (kind 6 instead of 7; the norm as a second launch), same results.  Every other ldc, odd ones included, is inside
 * the contract: the vector stores are then under-aligned, which global memory instructions execute correctly on gfx950, only slower.  The engine relies on
 * it where a width is the model's to choose: the model-to-latent projections write fp32 rows of ldc = N = dim_latent, whatever dim_latent is.
 * tests/test_gemm_elementwise_gpu.py runs ldc = N = 6 and 5 on the register-staged kernel, ldc % 4 == 2 and odd ldc on the decode, skinny, mid, LDS-DMA,
 * ping-pong and one-wave kernels, and ldc = N + 8 everywhere else.  Nothing is written outside rows [0, M) (or the rows `rowmap` names) x the written width. */
typedef struct {
  const tfx_bf16* A; int32_t lda;
  const tfx_bf16* A2; int32_t lda2; int32_t K1;
  const tfx_bf16* B; int32_t ldb;
  int32_t M, N, K;
  int32_t epi;
  void* C; int32_t ldc;
  void* C2; int32_t ldc2;
  const float* bias;
  const tfx_bf16* R; int32_t ldr; int32_t resid_mapped;   /* residual row = scattered row if set */
  const int32_t* rowmap;
  const int32_t* a_rowmap;
  const tfx_bf16* aux; int32_t ldaux;
  /* TFX_EPI_QKV_NORM_ROPE (round 4; SURVEY K4, reference T:946-965): the fused [q | k | v | gates] projection.  C (bf16, ldc) receives the raw
   * projection as with TFX_EPI_BF16 (the backward of the norm reads it); C2 (bf16, ldc2 >= 2 qk_heads 64) receives q~ | k~ = QK-RMSNorm + RoPE
   * (+ the q scale) of the first 2 qk_heads 64 columns - exactly what tfx_qk_norm_rope_fwd computes from C, bit for bit, without the launch and
   * without reading q, k back.  The qk_* fields mirror tfx_qk_norm_rope_args (gammas [64], rot_pos [M], cos / sin tables [P, 32], scales, optional
   * soft-cap plan).  Decode steps: qk_cache (bf16 rows of ld_cache = [k~ (qk_heads 64) | v (qk_heads 64)]) + qk_cache_pos [M] append this step's
   * k~ and v rows at row qk_cache_pos[m] (< 0: skip) - the KV-cache append of tfx_qk_norm_rope_args.cache in the same epilogue (T:1005-1016).
   * Fused in the 256 x 256 kernel (training shapes) and in the decode-step kernel (M <= 1024); every other shape runs as the plain projection
   * followed by tfx_qk_norm_rope_fwd inside the call - same results bit for bit. */
  int32_t qk_heads;
  const float* qk_gamma_q; const float* qk_gamma_k;   /* both NULL: no RMS normalisation (tfx_qk_norm_rope_args); one NULL and one set: -5 */
  const int32_t* qk_rot_pos; const float* qk_cos; const float* qk_sin;
  float qk_q_scale, qk_norm_scale;
  float* qk_plan; float qk_softcap;
  tfx_bf16* qk_cache; int32_t qk_ld_cache; const int32_t* qk_cache_pos;
  /* Cold-operand prefetch (round 6, decode plans): `prefetch_bytes` bytes at `prefetch` - the weights of the NEXT GEMM of a launch list - are touched by
   * spare blocks of THIS launch (one load per 64 bytes, nothing written), so that they wait in the 256 MB Infinity Cache when their launch comes.  A decode
   * forward streams 25 MB of weights per layer through launches of a few dozen blocks whose time is a chain of memory round trips (tools/decode_cold_probe.py:
   * 10.1 us cold against 6.7 us warm for the out-projection at 64 rows).  Honoured by the small-M kernels (fewer than 512 tiles of 256 x 256), ignored when
   * null / 0.  Results do not depend on it. */
  const void* prefetch; int64_t prefetch_bytes;
} tfx_gemm_nt_args;
int tfx_gemm_nt(const tfx_gemm_nt_args* a, void* stream);
/* which kernel tfx_gemm_nt would launch for these arguments and on how many blocks, without launching (host logic only, no device needed):
 * 0 register-staged fallback, 1 LDS-DMA 128 x 128, 2 "mid" (<= one 128 x 128 tile per CU), 3 ping-pong 256 x 256 (8 waves: the fused epilogues, row-gathered /
 * split A), 4 skinny (M <= 512 ... 1024), 5 decode (M <= 1024, K split across the waves), 6 one wave per SIMD 256 x 256, one tile per block (fp32 outputs from
 * K = 1024, bf16 outputs with K < 192), 7 one wave per SIMD, persistent (bf16 outputs, K >= 192).  Kinds 6 / 7 since round 6 (they reported 3 before). */
int tfx_gemm_nt_plan(const tfx_gemm_nt_args* a, int32_t* kind, int32_t* grid);

/* Measurement aid (bench.py `roofline.measured_peak`; no reference counterpart): a register-resident loop of `iters` x 4 v_mfma_f32_32x32x16_bf16 per wave on
 * `blocks` blocks of 4 waves, operands = the 128 x 16 bytes at `ops` (lane-indexed; random bf16 for the power the data toggles cost, zeros read ~20 % higher),
 * no memory traffic inside the loop.  flops = 2 x 32 x 32 x 16 x 4 x iters x blocks x 4; the caller times the launch.  `out`: 2 floats of scratch. */
int tfx_mfma_peak_probe(const void* ops, float* out, int32_t iters, int32_t blocks, void* stream);

/* C[rowmap[n]][k] += alpha * sum_m A[m][n] * B[m][k]   (fp32 C, ALWAYS accumulates: split-M partial sums are
 * added with fp32 atomics, the caller zeroes C when it wants a plain product; `accumulate` is ignored).
 * a_cols/b_cols: number of readable columns of A/B (multiples of 8); k_valid: columns of the product that are written.
 * splits: number of M chunks (of a multiple of 64 rows) summed through the atomics; 1 = one block per output tile over all rows;
 * 0 = the library picks the count that fills the chip with the tiles of the kernel it launches. */
typedef struct {
  const tfx_bf16* A; int32_t lda; int32_t a_cols;
  const tfx_bf16* B; int32_t ldb; int32_t b_cols;
  int32_t M, N, K;
  float* C; int32_t ldc;
  const int32_t* rowmap;
  int32_t k_valid;
  int32_t splits;
  int32_t accumulate;
  float alpha;
  const int32_t* a_rowmap;    /* gather rows of A / B (row index = map[m]); NULL = identity */
  const int32_t* b_rowmap;
  float* colsum;              /* optional: colsum[rowmap[n]] += sum_m A[m][n] - the bias gradient that belongs to this weight gradient,
                                 folded into the GEMM (one extra MFMA against a ones operand in the blocks of the first K tile) */
  int32_t k_group;            /* 0 = off; else the K columns come in groups of 64 of which the first k_group are written, compacted:
                                 C column = (k / 64) * k_group + k % 64  (per-head padded operand -> unpadded weight gradient) */
  /* grouped launch (round 5): HOST pointer to the tfx_gemm_tn_args of another product over the same M rows (its own group_next continues the chain; at most 6
   * products; `splits` of the chain's head applies).  The weight-gradient products of a transformer layer - the FeedForward pair, to_out, to_qk/v/gates, the skip
   * projection's halves - then run as ONE launch whose output tiles fill the chip at 4 row chunks instead of 11-20 per product: half the fp32 atomics of the
   * split-M sums (which the chip retires at ~1.25 TB/s: 27-42 % of the ungrouped kernels) and 256 x 256 tiles for the 512 x 512 products.  Products the one-wave
   * kernel does not take (row-gathered operands, M % 64 != 0, chunks under 192 rows) make the library run the chain one by one - same results.  NULL = single. */
  const void* group_next;
  /* table launch (round 7): any number of products over the same M rows - the weight gradients of a RUN OF LAYERS - as ONE launch of the one-wave kernel, the problem
   * list in DEVICE memory instead of the kernel-argument segment that bounds a `group_next` chain at 6.  `table`: device pointer to `table_count` records of
   * tfx_gemm_tn_args followed by `table_count` int32 - the inclusive prefix sums of the records' 256 x 256 tile counts ceil(N / 256) * ceil(K / 256).  `table_host`:
   * the same bytes in host memory, owned by the caller like a `group_next` chain: the library plans the launch from it (tile sum, chunk count, whether every member
   * qualifies) and never uploads anything, so the launch replays from a captured graph.  The head struct is the table's first product with these fields set (its M and
   * `splits` apply to all; a record's own group_next / table fields are ignored).  With several hundred tiles the grid is several rounds of the chip at 2-4 row chunks
   * per tile where a layer's group needs 7-13: a quarter of the fp32 atomics, one launch instead of two per layer, and blocks that finish at different times, so one
   * block's atomics drain under the others' MFMAs.  splits == 0: the chunk count that minimises ceil(tiles x chunks / 256) x chunk length over chunks of >= 256
   * rows (multiples of 64), each block's 256 KiB of atomics charged at the chip's rate so that ragged tile counts do not run to 256-row chunks.  A table with a member the one-wave kernel does not take (row-gathered operands, M % 64 != 0, another M, a chunk under 192 rows) runs
   * its records one by one - same results.  `table` wins over `group_next`.  NULL = no table. */
  const void* table;
  const void* table_host;
  int32_t table_count;
  int32_t table_reserved;
} tfx_gemm_tn_args;
int tfx_gemm_tn(const tfx_gemm_tn_args* a, void* stream);
/* what tfx_gemm_tn would launch for these arguments, without launching (host logic only, no device needed): kernel form (-1 register-staged
 * fallback, 0 = 128 x 128 tiles / 4 waves, 2 = 256 x 256 / 8 waves, 3 = 256 x 256 / 4 waves of 128 x 128 (one wave per SIMD, round 5)), output tiles,
 * row chunks (`splits`, chosen when a->splits == 0), grid.  For the head of a `group_next` chain that runs as one launch: kind 3 with the chain's summed tiles, its
 * chunk count and grid; a chain that runs product by product reports the head's own plan.  The head of a `table` likewise: kind 3 with the table's summed tiles,
 * chunk count and grid (which may be several rounds of the chip), or the head's own plan when the table runs record by record. */
int tfx_gemm_tn_plan(const tfx_gemm_tn_args* a, int32_t* kind, int32_t* tiles, int32_t* splits, int32_t* grid);

/* ---- attention ------------------------------------------------------------------------------- */
/* q,k,v: bf16, token-major; element (token t, head h, i) at ptr[t*ld + h*64 + i]; dim_head == 64.
 * kv_end[t] (per token, relative to its sample): key j visible iff j < kv_end.  q_start[j]: first query
 * position that sees key j.  gate: logits at gate[t*ld_gate + h].  out: gated output og (bf16).
 * gate == NULL: no value gating (reference Attention(gate_values=False), T:901-904, T:1026-1027) - sigmoid(gate) reads as exactly 1 everywhere:
 *   forward (tfx_attn_fwd, and tfx_decode_attn on both of its kernels, dense and compacted): og = P v; under `laser`: og = log(P v')
 *   backward prep (tfx_attn_bwd): do_eff = dout (laser: dout exp(-og)), delta as with a gate of 1; `dgate` is NOT written and may be NULL
 * One wave-uniform branch per site.  With a gate pointer every kernel computes what it computed before NULL had a meaning, bit for bit, and a NULL
 * call gives the bits of the same call with gate logits whose sigmoid is 1 in fp32 (tests/test_ablation_gpu.py). */
typedef struct {
  const tfx_bf16 *q, *k, *v; int32_t ld_q, ld_k, ld_v;
  const tfx_bf16* gate; int32_t ld_gate;
  const int32_t* kv_end;
  const int32_t* q_start;
  tfx_bf16* out; int32_t ld_out;
  float* lse;                 /* [b, h, n] */
  int32_t b, h, n;
  float softcap;
  int32_t n_kv;               /* forward only: keys/values have n_kv rows per sample (KV-cache decode); 0 = n */
  /* backward */
  const tfx_bf16* dout; int32_t ld_dout;     /* grad wrt gated output */
  tfx_bf16* do_eff; int32_t ld_do;           /* scratch: dout * sigmoid(gate) */
  float* delta;                               /* [b, h, n] */
  tfx_bf16* dgate; int32_t ld_dgate;         /* grad wrt gate logits (not written, may be NULL, when gate == NULL) */
  tfx_bf16 *dq, *dk, *dv; int32_t ld_dq, ld_dk, ld_dv;
  int32_t order;              /* set by the library (block order of the launch); callers leave it 0 */
  const float* sc_plan;       /* optional, forward and backward: the layer's soft-cap plan (tfx_qk_norm_rope_args.sc_plan); NULL = decide from the scores.
                               * PRECONDITION: a plan of mode 0 / 1 is a polynomial fitted on [-B, B] and the kernels do NOT check the scores
                               * against B - every q and k row of this call (KV-cache rows included) must have been produced by tfx_qk_norm_rope_fwd (or the
                               * fused projection epilogue) under the SAME gammas / scales the plan was written from.  Rows from other gains, or without
                               * QK-norm, make the polynomial diverge silently outside [-B, B]: pass NULL for such inputs.  tfx_decode_attn (the
                               * matrix-core-free decode kernel) ignores the plan and evaluates the data-dependent form.  In the forward against a KV
                               * cache (n_kv > 0) the data-dependent form decides row by row, never from the wave's other rows: with or without a plan, a
                               * query row's out and lse bits do not depend on the rows the launch carries beside it. */
  /* forward with a KV cache, optional (compacted decode steps): sample s of the launch owns the query rows q_row0[s] .. q_row0[s] + q_cnt[s] - 1 of the
   * token arrays (q, gate, kv_end, out) instead of rows s * n .. (`n` stays the per-sample maximum and sizes the grid; q_cnt[s] = 0: nothing to do);
   * keys / values are still the sample's n_kv cache rows.  Device arrays of `b` int32 each; NULL = the dense layout. */
  const int32_t* q_row0; const int32_t* q_cnt;
  /* backward, optional (round 5): the backward of QK-RMSNorm + RoPE (+ the q scale; reference T:950-952, T:965, T:998 backwards) in the epilogues of the dQ and
   * dK/dV kernels.  With nr_qkv set, the kernels do not write d q~ / d k~ to dq / dk: each wave takes its 32 x 64 block through the staging image it stores
   * from anyway - 8 lanes per row, 8 contiguous columns each, the token-wise kernel's own shape - loads the raw (pre-norm) q / k chunk, applies
   * tfx_qk_norm_rope_bwd's arithmetic to the bf16-rounded d q~ / d k~ and writes d q | d k (raw) to nr_dqkv (q at column h*64, k at column h_total*64 + h*64,
   * the layout of tfx_qk_norm_rope_args.dqkv); the gain gradients accumulate per block and leave as 64 atomics per block and kernel.  One write + one read of
   * the [T, 2 h 64] d q~ | d k~ matrix and the tfx_qk_norm_rope_bwd launch drop out of a layer's backward.  All nr_* leading dimensions % 8 == 0, 16-byte
   * aligned bases; nr_norm_scale 0 = 8. */
  const tfx_bf16* nr_qkv; int32_t nr_ld_qkv;
  tfx_bf16* nr_dqkv; int32_t nr_ld_dqkv;
  const float* nr_gamma_q; const float* nr_gamma_k;   /* both NULL: no RMS normalisation (tfx_qk_norm_rope_args): d q = q_scale rope^T(d q~), d k = rope^T(d k~), bit for
                                                         * bit what tfx_qk_norm_rope_bwd writes; nr_qkv is not read, nr_dgamma_* are not touched and may be NULL */
  const int32_t* nr_rot_pos; const float* nr_cos; const float* nr_sin;
  float nr_q_scale, nr_norm_scale;
  float* nr_dgamma_q; float* nr_dgamma_k;
  /* LASER attention (reference T:979-983, T:1019-1022; Transformer(attn_laser=True)), forward, decode and backward.  0 = off: every kernel computes what it
   * computed before the field existed, bit for bit.  1: `v` holds v' = exp(c tanh(v / c)) (tfx_laser_v_fwd) and the forward writes og = sigmoid(gate) log(P v')
   * instead of sigmoid(gate) P v'; `lse` is unchanged.  The backward prep then takes L = og / sigmoid(gate) and hands the dK/dV and dQ kernels
   * do_eff = dout sigmoid(gate) exp(-L), delta = sum_d dout sigmoid(gate) (= do_eff . P v' exactly), dgate = sum_d dout og (1 - sigmoid(gate)); their dv is
   * d v', which tfx_laser_v_bwd turns into d v. */
  int32_t laser;
} tfx_attn_args;
int tfx_attn_fwd(const tfx_attn_args* a, void* stream);
int tfx_attn_bwd(const tfx_attn_args* a, void* stream);   /* prep + dK/dV kernel + dQ kernel */

/* decode step (reference T:2279-2349, T:2409-2419): the forward kernel addressed against a KV cache - `n` NEW query rows per
 * sample, keys / values in a per-sample buffer of `n_kv` > 0 rows, kv_end[t] = visible cache length of query row t (own prefix + the block
 * being decoded).  Fails with -10 when n_kv == 0.  One or two rows per sample in the dense layout run on a matrix-core-free rows kernel; three
 * rows and more, and every compacted call (q_row0 or q_cnt set, whatever `n` is: the rows kernel addresses rows b * n .. only), run on the
 * tiled forward kernel exactly as tfx_attn_fwd would. */
int tfx_decode_attn(const tfx_attn_args* a, void* stream);

/* LASER value transform (reference T:979-983: softclamp T:280-281, then exp): token-wise over T rows of H heads x 64 columns.
 *   forward:  vl[rowmap[t]] = bf16(exp(c tanh(v[t] / c))), computed in fp32 and rounded once; rowmap NULL = row t, rowmap[t] < 0 = skip
 *             (decode steps: this step's rows into a side cache of v', the rows the KV-cache append writes raw v to)
 *   backward: dv[t] = dvl[t] exp(c tanh(v[t] / c)) (1 - tanh(v[t] / c)^2), the factor recomputed in fp32 from the raw v; dv may alias dvl
 *             (in place over the d v' the attention backward wrote).  rowmap is ignored.
 * All leading dimensions % 8 == 0, 16-byte aligned bases; c > 0.  |c tanh| <= c, so v' needs no max-subtraction: [exp(-c), exp(c)]. */
typedef struct {
  int32_t T, H;
  const tfx_bf16* v; int32_t ld_v;            /* raw values */
  tfx_bf16* vl; int32_t ld_vl;                /* forward: v' out */
  const int32_t* rowmap;                      /* forward, optional: output row of input row t (< 0 = skip) */
  float c;                                    /* laser_softclamp_value (reference default 15, T:866) */
  const tfx_bf16* dvl; int32_t ld_dvl;        /* backward: d v' in */
  tfx_bf16* dv; int32_t ld_dv;                /* backward: d v out */
} tfx_laser_v_args;
int tfx_laser_v_fwd(const tfx_laser_v_args* a, void* stream);
int tfx_laser_v_bwd(const tfx_laser_v_args* a, void* stream);

/* ---- token-wise kernels ---------------------------------------------------------------------- */
/* NULL parameter-gradient outputs (frozen parameters: `requires_grad_(False)` on the Python side).  The column sums these kernels add into a parameter's
 * gradient may be switched off one by one by passing NULL for the output:
 *   tfx_adaln_pre_args.dgamma_text, .dtable            tfx_adaln_pre_bwd, tfx_adaln_pre_post_bwd (per-token and segment forms)
 *   tfx_adaln_post_args.dlayerscale, .dbias, .dtable   tfx_adaln_post_bwd, tfx_adaln_pre_post_bwd, tfx_attnres_pull_bwd's wrapper side (per-token and segment forms)
 *   tfx_rmsnorm_args.dgamma                   tfx_rmsnorm_bwd
 *   tfx_attnres_args.dgamma, .dpq             tfx_attnres_bwd (push form)
 *   tfx_attnres_src.dgamma, .dpq              tfx_attnres_finish (pull form; the d w accumulator src.dw is always formed)
 * NULL means: the block-level reduction of that sum is not formed and no atomic is issued for it.  Every other output of the call is bit-identical to the
 * same call with the pointer (rows, stored table gradients; atomically accumulated sums agree as two runs of one call do), and with the pointer the kernel
 * computes what it computed before NULL had a meaning.  Each pointer is independent.  One block-uniform branch per site (the pointer is a kernel argument).
 * `dtable` NULL: neither the per-token atomics nor the segment forms' stores of that side's table gradient are issued (in tfx_adaln_pre_post_bwd the two
 * sides' pointers are independent); the engine passes it when no trainable parameter sits behind the AdaLN tables (to_film.*, to_ada_ln_zero.*,
 * to_time_cond.*).
 * NOT NULL-able: ONE of dgamma_q / dgamma_k of the QK-norm kernels and attention epilogues (both NULL with both gains NULL only): the engine points a
 * frozen gain's sum at a 64-float scratch row. */
typedef struct {
  int32_t T, d;
  const tfx_bf16* x; tfx_bf16* u;            /* [T,d] */
  const int32_t* tok_inst;                    /* [T] instance id or -1 (text) */
  const float* table; int32_t ld_table;       /* fp32 [I, ld]; this wrapper's gamma at +0, beta at +d, z at +2d */
  const float* gamma_text;                    /* layernorm_gamma [d] */
  float* mean; float* rstd;                   /* [T] saved stats */
  /* backward */
  const tfx_bf16* du; tfx_bf16* dx;           /* dx += LN backward (in place accumulate) */
  float* dtable;                              /* fp32 [I, ld] (atomic accumulate) */
  float* dgamma_text;                         /* [d] (atomic accumulate) */
  /* optional segment mode (backward): runs of consecutive tokens sharing one tok_inst value; one wave owns a
   * segment, so an instance's FiLM gradients are reduced in registers and STORED (no atomics).  NULL or n_seg == 0 = per-token atomics */
  const int32_t* seg_start; const int32_t* seg_len; int32_t n_seg;
  const tfx_bf16* dx_add;                     /* backward, optional [T,d]: one more addend of dx (the gradient a U-Net skip hands to this layer's input) */
} tfx_adaln_pre_args;
int tfx_adaln_pre_fwd(const tfx_adaln_pre_args* a, void* stream);
int tfx_adaln_pre_bwd(const tfx_adaln_pre_args* a, void* stream);

typedef struct {
  int32_t T, d;
  const tfx_bf16* x; const tfx_bf16* y; tfx_bf16* out;   /* out = x + y * scale */
  const int32_t* tok_inst;
  const float* table; int32_t ld_table;       /* z logits at table[inst*ld + 2d + col] */
  const float* layerscale;                    /* [d] */
  /* backward: g = grad wrt out (also the residual grad, passed through untouched) */
  const tfx_bf16* g; tfx_bf16* dy;
  float* dtable; float* dlayerscale;
  const int32_t* seg_start; const int32_t* seg_len; int32_t n_seg;   /* optional segment mode, see tfx_adaln_pre_args */
  float* dbias;                               /* optional [d]: += column sums of dy (the bias gradient of the Linear that produced y) */
} tfx_adaln_post_args;
int tfx_adaln_post_fwd(const tfx_adaln_post_args* a, void* stream);
int tfx_adaln_post_bwd(const tfx_adaln_post_args* a, void* stream);

typedef struct {
  int32_t T, H;                               /* kernel layout: 64 columns per head; dim_head < 64 = zero columns past dim_head */
  const tfx_bf16* qkv; int32_t ld_qkv;        /* q at col h*64, k at col H*64 + h*64 (pre-norm) */
  tfx_bf16* qk; int32_t ld_qk;                /* post norm+rope(+q scale), same column layout */
  const float* gamma_q; const float* gamma_k; /* [64].  BOTH NULL: no RMS normalisation (reference Attention(qk_rmsnorm=False), T:948-952) -
                                               *   forward  q~ = rope(q) q_scale, k~ = rope(k);   backward  dq = q_scale rope^T(dq~), dk = rope^T(dk~)
                                               * `qkv` is not read by the backward, dgamma_* are not touched and may be NULL, norm_scale is ignored; the KV-cache
                                               * append works as before.  A given `sc_plan` receives mode 2 with B = +inf in slot 7: nothing bounds
                                               * unnormalised scores, so the polynomial modes are never chosen for them (the precondition of
                                               * tfx_attn_args.sc_plan).  The token-wise kernel, the fused GEMM epilogue (tfx_gemm_nt_args.qk_gamma_*) and the
                                               * attention backward's epilogues (tfx_attn_args.nr_gamma_*) share one spelling of the chunk (tfx_common.h) and agree
                                               * bit for bit.  One NULL and one set is an error (-4). */
  const int32_t* rot_pos;                     /* [T] */
  const float* cos_tab; const float* sin_tab; /* [P, 32] */
  float q_scale;
  /* backward */
  const tfx_bf16* dqk; int32_t ld_dqk;        /* grad wrt post-norm q,k */
  tfx_bf16* dqkv; int32_t ld_dqkv;            /* grad wrt pre-norm q,k (written) */
  float* dgamma_q; float* dgamma_k;           /* atomic accumulate */
  float norm_scale;                           /* sqrt(dim_head), the RMSNorm scale T:779-786; 0 = 8 (dim_head 64) */
  /* forward, decode steps (optional): KV-cache append fused in (T:1005-1016) - token t's k~ (H*64 columns) and v (the H*64 columns behind k in
   * `qkv`) are also written to cache row cache_pos[t] ([k~ | v], ld_cache elements per row; cache_pos < 0 = skip).  A decode step is launch-bound
   * (~4.5 us per kernel whatever its size): this removes two launches per layer */
  tfx_bf16* cache; int32_t ld_cache; const int32_t* cache_pos;
  /* forward, optional: the layer's soft-cap plan for the attention kernels (`tfx_attn_args.sc_plan`), 8 floats written by block 0.  QK-RMSNorm bounds
   * the scores, |q~ . k~| <= B = norm_scale^2 q_scale max|1 + gamma_q| max|1 + gamma_k| (x 1.02 for the bf16 rounding of q~, k~), so the degree of the
   * polynomial that replaces cap tanh(s / cap) is a property of the LAYER, not of the data: the attention kernels need not look at their scores to pick
   * it.  plan = {mode, p1, p3, p5, d1, d3, d5, B}: mode 0 (B / cap <= 0.2) cubic, mode 1 (<= 0.35) quintic - Chebyshev-economised on [-B, B],
   * s2 = s (p1 + p3 s^2 + p5 s^4) in the log2 domain and d tanh / dx = d1 + d3 s^2 + d5 s^4 its exact derivative; mode 2: the kernels decide
   * per wave from the scores as without a plan.  `softcap` must be the attention's. */
  float* sc_plan; float softcap;
} tfx_qk_norm_rope_args;
int tfx_qk_norm_rope_fwd(const tfx_qk_norm_rope_args* a, void* stream);
int tfx_qk_norm_rope_bwd(const tfx_qk_norm_rope_args* a, void* stream);
/* decode steps: AdaLN output side of one wrapper + AdaLN input side of the next in ONE launch (out = x + y * scale is written, then normalised and
 * modulated into `pre->u` exactly as tfx_adaln_pre_fwd would read it back: same bf16 rounding of `out`).  post->T/d/tok_inst must equal pre's. */
int tfx_adaln_post_pre_fwd(const tfx_adaln_post_args* post, const tfx_adaln_pre_args* pre, void* stream);

typedef struct {
  int32_t T, d, L;                            /* L = number of hiddens h_0..h_{L-1} */
  const tfx_bf16* hiddens; int64_t stride_h;  /* hiddens + l*stride_h -> [T,d] */
  const float* gamma; const float* pq;        /* norm_keys.gamma, pseudo_queries [d] */
  tfx_bf16* out;
  /* backward */
  const tfx_bf16* g; const tfx_bf16* g2;      /* grad wrt out (+ optional second addend) */
  tfx_bf16* dhiddens; int64_t stride_dh;      /* accumulate (or store if `first`) */
  int32_t first;
  float* dgamma; float* dpq;                  /* atomic accumulate */
  /* forward, optional (training plans): the depth softmax of every token is kept for the pull-form backward (tfx_attnres_pull_bwd):
   * save[(t * L + l) * 4 + {0, 1, 2}] = softmax weight a_l, 1 / |h_l|, score s_l = <h_l, w> / |h_l| */
  float* save;
  tfx_bf16* err;                              /* with `save`: [T,d] what the bf16 rounding of `out` dropped (exact mix - stored out), for <g, out> in the backward */
} tfx_attnres_args;
int tfx_attnres_fwd(const tfx_attnres_args* a, void* stream);
int tfx_attnres_bwd(const tfx_attnres_args* a, void* stream);
/* decode steps: the END of a layer in one launch - feed-forward AdaLN output side (writes hidden L - 1 = post->out), the layer's AttentionResidual
 * over hiddens 0 .. L - 1 (writes ar->out), and - when `pre` is non-NULL - the input side of the NEXT layer's attention wrapper on that output.
 * Same roundings as the three separate launches (every written row is re-read as bf16).  post->out must be hidden L - 1 of `ar`, pre->x == ar->out. */
int tfx_layer_end_fwd(const tfx_adaln_post_args* post, const tfx_attnres_args* ar, const tfx_adaln_pre_args* pre, void* stream);

/* AttentionResidual backward in PULL form (T:807-829; the training plans' form).  Hidden l feeds the AttentionResidual of every layer
 * j >= l - 1, so its gradient is   dh_l = sum_j [ a_jl g_j + k1_jl w_j - k2_jl h_l ],   k1 = ds inv_l, k2 = k1 s_jl inv_l,
 * ds_jl = a_jl (<g_j, h_l> - <g_j, out_j>)   (sum_l a_jl <g_j, h_l> = <g_j, out_j>: the forward output is the softmax mix of the hiddens).
 * The push form (tfx_attnres_bwd, one launch per layer) reads every earlier hidden and read-modify-writes every earlier gradient once per
 * layer: (3L + 2) passes of [T, d] per layer.  The pull form computes dh_l ONCE, when the backward reaches layer l - 1: it reads h_l and the
 * n_src output gradients g_j (all final by then), plus three saved scalars per (j, token) - (n_src + 2) passes, about 0.6x the bytes at
 * depth 8 and 0.5x at depth 24.  d w_j = sum_t sum_l k1_jl h_l accumulates in registers (n_src <= 8 at d <= 512) or in LDS, per launch, into
 * src[j].dw; tfx_attnres_finish turns it into d gamma / d pseudo_queries.
 * With `post` the feed-forward wrapper's output side (tfx_adaln_post_bwd on g = the dh_l just written) runs in the same launch. */
typedef struct {
  const tfx_bf16* g;                          /* [T,d] gradient wrt the output of this layer's AttentionResidual (final) */
  float* save;                                /* [T, L, 4] its saved forward state (tfx_attnres_args.save); entry [t][0][3] receives <g, out> in the backward */
  float* dsum;                                /* [T] <g, out>: written by the launch that lists this layer first with `out_own`, read by later ones */
  float* w; float* dw;                        /* [d] fp32: (1 + gamma) * pseudo_queries (tfx_attnres_prep); its gradient accumulator (atomics) */
  const float* gamma; const float* pq;        /* norm_keys.gamma, pseudo_queries [d] */
  float* dgamma; float* dpq;                  /* their gradients (tfx_attnres_finish, accumulate) */
  int32_t L; int32_t reserved;                /* hiddens this layer mixes */
} tfx_attnres_src;
typedef struct {
  int32_t T, d, l, n_src;                     /* hidden index l; 1 <= n_src <= 32 layers read it */
  const tfx_bf16* h;                          /* [T,d] hidden l */
  const tfx_attnres_src* src;                 /* DEVICE array [n_src], lowest layer first */
  const tfx_bf16* out_own;                    /* optional [T,d]: the forward output of src[0]'s AttentionResidual - its dsum is formed here */
  const tfx_bf16* out_err;                    /* optional [T,d]: what rounding that output to bf16 dropped (tfx_attnres_args.err) */
  const tfx_bf16* add;                        /* optional [T,d] addend (gradient that reaches the hidden directly) */
  tfx_bf16* dh;                               /* [T,d] result (stored) */
  const int32_t* seg_start; const int32_t* seg_len; int32_t n_seg;   /* token segments (tfx_adaln_pre_args); n_seg == 0: one token per wave */
  /* d w of the sources: with k1 == NULL (allowed for n_src <= 8, d <= 512) it accumulates inside the launch into src[j].dw; otherwise the launch
   * only writes k1[t * ld_k1 + j] = the per-token coefficient of source j (bf16, ld_k1 >= n_src, a multiple of 8) and the caller adds
   * dw[j] += sum_t k1[t][j] h[t]  with one tfx_gemm_tn (A = k1, B = h, C = src[0].dw, ldc = d: the dw rows of consecutive sources are contiguous) */
  tfx_bf16* k1; int32_t ld_k1;
} tfx_attnres_pull_args;
int tfx_attnres_prep(const tfx_attnres_src* src_dev, int32_t n, int32_t d, void* stream);     /* w = (1 + gamma) pq ; dw = 0, for n layers */
int tfx_attnres_pull_bwd(const tfx_attnres_pull_args* a, const tfx_adaln_post_args* post, void* stream);
int tfx_attnres_finish(const tfx_attnres_src* src_dev, int32_t n, int32_t d, void* stream);   /* dgamma += dw pq ; dpq += dw (1 + gamma) */
/* backward of two adjacent wrapper sides in one launch: tfx_adaln_pre_bwd(pre) (dx += LN backward, in place) followed by
 * tfx_adaln_post_bwd(post) with post->g == pre->dx: the residual-gradient row is written once and not read back.  Segment mode only
 * (pre->n_seg > 0, same segments); bit-identical to the two launches. */
int tfx_adaln_pre_post_bwd(const tfx_adaln_pre_args* pre, const tfx_adaln_post_args* post, void* stream);

typedef struct {
  int32_t T, d;
  const tfx_bf16* x; tfx_bf16* y; const float* gamma;
  const tfx_bf16* dy; tfx_bf16* dx; float* dgamma;
} tfx_rmsnorm_args;
int tfx_rmsnorm_fwd(const tfx_rmsnorm_args* a, void* stream);
int tfx_rmsnorm_bwd(const tfx_rmsnorm_args* a, void* stream);

/* text embedding gather into the token buffer (only tokens with tok_inst < 0), and its backward */
typedef struct {
  int32_t T, d;
  const int32_t* text_ids; const int32_t* tok_inst;
  const tfx_bf16* table;                      /* bf16 shadow of text_embed.weight [V, d] */
  tfx_bf16* x;
  const tfx_bf16* dx; float* dtable;          /* backward: fp32 [V, d] atomic accumulate */
} tfx_embed_args;
int tfx_embed_fwd(const tfx_embed_args* a, void* stream);
int tfx_embed_bwd(const tfx_embed_args* a, void* stream);

/* x_t = t*x + (1-t)*eps (bf16, padded to ld_xt with zeros), flow = x - eps (fp32)   MP:654-656 */
typedef struct {
  int32_t R, dl;
  const float* x; const float* eps;           /* [R, dl] */
  const int32_t* row_inst; const float* inst_time;
  tfx_bf16* xt; int32_t ld_xt;
  float* flow;                                /* [R, dl] (may be NULL) */
} tfx_noise_mix_args;
int tfx_noise_mix(const tfx_noise_mix_args* a, void* stream);

/* e[i,:] = [t, sin(2 pi t w), cos(2 pi t w)] bf16, zero padded to ld   T:617-635 */
typedef struct { int32_t I, half; const float* times; const float* w; tfx_bf16* out; int32_t ld; } tfx_fourier_args;
int tfx_fourier(const tfx_fourier_args* a, void* stream);

/* fused cross-entropy forward + backward over fp32 logits [T, ld] (V valid columns)   T:3320-3331 */
typedef struct {
  int32_t T, V; const float* logits; int32_t ld;
  const int32_t* labels;                      /* -1 = ignore */
  float grad_scale;                           /* text_loss_weight / total_tokens */
  tfx_bf16* dlogits; int32_t ld_d;            /* bf16 [T, ld_d], pad columns zeroed */
  float* acc;                                 /* acc[0] += sum of token CE, acc[1] += #valid */
} tfx_ce_args;
int tfx_ce_fwd_bwd(const tfx_ce_args* a, void* stream);

/* the same cross entropy SPLIT into a forward and a backward launch over a CHUNK of rows (engine.Plan `chunk`, Transfusion.set_text_head_chunking_): the
 * fp32 logits of T rows at a time live in one small buffer that the forward fills and the backward fills again with the same product, so a step never
 * holds [all rows, V] logits or their gradient.  The forward keeps one float per row - lse = log sum exp - and the backward forms the gradient from it:
 *   tfx_ce_fwd   one pass over the row (online max / sum, 16-byte loads): lse[t] = m + log sum_c exp(l_c - m), acc[0] += sum_t (lse[t] - l[label_t]), acc[1] += #valid;
 *                ignored rows (label -1) get lse 0 and are not read; a launch whose rows are all ignored leaves `acc` untouched.  Reads logits, labels; writes lse, acc.
 *   tfx_ce_bwd   one pass: dlogits[t, c] = bf16((exp(l_c - lse[t]) - [c == label_t]) * grad_scale * (scale_dev ? *scale_dev : 1)), columns V .. ld_d - 1 and
 *                ignored rows zero (bf16x8 stores).  Reads logits, labels, lse; writes dlogits.
 * Rows of at most 1024 logits (ld) run one wave per row, four rows per block; wider rows one block per row with an LDS combine of the waves' (max, sum) pairs.
 * Both: grid-stride over rows under a capped grid; two atomics into `acc` per block, as tfx_ce_fwd_bwd.  1 <= V <= ld, ld_d; ld and ld_d multiples of 8 and
 * logits / dlogits 16-byte aligned, or -1. */
typedef struct {
  int32_t T, V; const float* logits; int32_t ld;      /* a chunk: T rows */
  const int32_t* labels;                              /* -1 = ignore */
  float* lse;                                         /* [T]; ignored rows get 0 */
  float* acc;                                         /* acc[0] += sum CE, acc[1] += #valid  (as tfx_ce_fwd_bwd) */
  /* backward */
  float grad_scale; const float* scale_dev;           /* g *= grad_scale * (scale_dev ? *scale_dev : 1) */
  tfx_bf16* dlogits; int32_t ld_d;                    /* pad columns V..ld_d-1 and ignored rows zeroed */
} tfx_ce_chunk_args;
int tfx_ce_fwd(const tfx_ce_chunk_args* a, void* stream);
int tfx_ce_bwd(const tfx_ce_chunk_args* a, void* stream);

/* the cross entropy with its two REGULARISERS: a z-loss on the softmax normaliser (PaLM, Chameleon) and label smoothing.  For a valid row (label y >= 0) with
 * the launch's V valid columns, logits l_c, lse = log sum_c exp l_c, p_c = exp(l_c - lse), weights z = z_weight >= 0 and e = smoothing in [0, 1):
 *   row term     r = (1 - e) (lse - l_y) + e (lse - (1/V) sum_c l_c) + z lse^2
 *   d r / d l_c    = p_c (1 + 2 z lse) - (1 - e) [c == y] - e / V
 * With e > 0 and z = 0 this is torch.nn.functional.cross_entropy(..., ignore_index = -1, label_smoothing = e).  Ignored rows contribute nothing and get
 * exact zeros, pad columns V .. ld_d - 1 are exact zeros.  V is the launch's V: whoever narrows it (forward_text: the text tokens) narrows what is smoothed over.
 * The regularised row sums go where the plain ones go - acc[0] += sum_t r_t, acc[1] += #valid - so every normalisation of the plain loss holds.  `aux`
 * (two floats, required) receives what the plain loss would have been and the drift monitor: aux[0] += sum_t (lse - l_y), aux[1] += sum_t lse^2.
 * Entry points, kernel shapes, grid caps, argument rules and return codes are those of tfx_ce_fwd_bwd / tfx_ce_fwd / tfx_ce_bwd; a block issues its (now
 * four) atomics only when one of its rows is valid.  sum_c l_c is formed only when smoothing > 0.  The backward needs nothing of the forward but lse (and no
 * `acc` / `aux`).  z_weight < 0, smoothing outside [0, 1) or a non-finite weight: -1 before any launch.  z_weight = smoothing = 0 gives the plain kernels'
 * d logits to the bit. */
typedef struct {
  int32_t T, V; const float* logits; int32_t ld;
  const int32_t* labels;                      /* -1 = ignore */
  float grad_scale;
  tfx_bf16* dlogits; int32_t ld_d;            /* bf16 [T, ld_d], pad columns zeroed */
  float* acc;                                 /* acc[0] += sum of the regularised row terms, acc[1] += #valid */
  float z_weight, smoothing;
  float* aux;                                 /* aux[0] += sum (lse - l_y), aux[1] += sum lse^2 */
} tfx_ce_reg_args;
int tfx_ce_reg_fwd_bwd(const tfx_ce_reg_args* a, void* stream);

typedef struct {
  int32_t T, V; const float* logits; int32_t ld;      /* a chunk: T rows */
  const int32_t* labels;                              /* -1 = ignore */
  float* lse;                                         /* [T]; ignored rows get 0 */
  float* acc;                                         /* as tfx_ce_reg_args (forward) */
  /* backward */
  float grad_scale; const float* scale_dev;           /* g *= grad_scale * (scale_dev ? *scale_dev : 1) */
  tfx_bf16* dlogits; int32_t ld_d;                    /* pad columns V..ld_d-1 and ignored rows zeroed */
  float z_weight, smoothing;
  float* aux;                                         /* as tfx_ce_reg_args (forward) */
} tfx_ce_reg_chunk_args;
int tfx_ce_reg_fwd(const tfx_ce_reg_chunk_args* a, void* stream);
int tfx_ce_reg_bwd(const tfx_ce_reg_chunk_args* a, void* stream);

/* the regularised cross entropy with one LOSS WEIGHT PER ROW (per-token loss weights: which tokens of a packed sample are trained on, and how strongly).
 * The structs are the `_reg` ones plus `row_w`, [T] floats >= 0 (required; the host refuses negative and non-finite weights).  With w = row_w[t]:
 *   a row with label < 0 or w == 0 is ignored: its logits are not read, its d logits are exact zeros, the chunk forward writes lse = 0;
 *   any other row adds  acc[0] += w r,  acc[1] += w,  aux[0] += w (lse - l_y),  aux[1] += w lse^2   (r: the row term of tfx_ce_reg_args),
 *   and gets  d logits = (d r / d l_c) s  with  s = grad_scale w [* *scale_dev]  formed once per row, in that order.
 * So acc[0] / acc[1] is the weighted mean torch.nn.functional.cross_entropy(weight = ...) normalises to, w = 1.0f gives tfx_ce_reg_*'s d logits and lse to
 * the bit, and weights in {0, 1} give what those kernels give with the zero-weight labels set to -1.  Entry points, kernel shapes, width classes, grid caps,
 * argument rules and return codes are those of tfx_ce_reg_*; z_weight = smoothing = 0 is allowed (the plain weighted cross entropy); a block issues its
 * atomics only when one of its rows counts.  NULL row_w: -1 before any launch. */
typedef struct {
  int32_t T, V; const float* logits; int32_t ld;
  const int32_t* labels;                      /* -1 = ignore */
  float grad_scale;
  tfx_bf16* dlogits; int32_t ld_d;            /* bf16 [T, ld_d], pad columns zeroed */
  float* acc;                                 /* acc[0] += sum w r, acc[1] += sum w */
  float z_weight, smoothing;
  float* aux;                                 /* aux[0] += sum w (lse - l_y), aux[1] += sum w lse^2 */
  const float* row_w;                         /* [T] */
} tfx_ce_w_args;
int tfx_ce_w_fwd_bwd(const tfx_ce_w_args* a, void* stream);

typedef struct {
  int32_t T, V; const float* logits; int32_t ld;      /* a chunk: T rows */
  const int32_t* labels;                              /* -1 = ignore */
  float* lse;                                         /* [T]; ignored rows get 0 */
  float* acc;                                         /* as tfx_ce_w_args (forward) */
  /* backward */
  float grad_scale; const float* scale_dev;           /* g *= grad_scale * row_w[t] * (scale_dev ? *scale_dev : 1) */
  tfx_bf16* dlogits; int32_t ld_d;                    /* pad columns V..ld_d-1 and ignored rows zeroed */
  float z_weight, smoothing;
  float* aux;                                         /* as tfx_ce_w_args (forward) */
  const float* row_w;                                 /* [T], both directions */
} tfx_ce_w_chunk_args;
int tfx_ce_w_fwd(const tfx_ce_w_chunk_args* a, void* stream);
int tfx_ce_w_bwd(const tfx_ce_w_chunk_args* a, void* stream);

/* tfx_ce_w_fwd with the ROW TERMS as an output (per-token losses: Transfusion.set_token_losses_()): the forward fields of
 * tfx_ce_w_chunk_args plus `row_loss`, [T] floats (required).  lse, acc and aux are what tfx_ce_w_fwd writes, sum for sum - the same kernel, width classes,
 * 16-byte loads and grid caps - and a row that counts also stores  row_loss[t] = w r  (the very number it adds to acc[0]); an ignored row (label < 0 or
 * w == 0) is not read and stores row_loss[t] = 0.  There is no backward of its own: tfx_ce_w_bwd forms d logits from lse under whatever row weights the
 * caller hands it - for a function f of the row terms, row_w[t] (d f / d row_loss[t]).  NULL row_w or row_loss: -1 before any launch. */
typedef struct {
  int32_t T, V; const float* logits; int32_t ld;      /* a chunk: T rows */
  const int32_t* labels;                              /* -1 = ignore */
  float* lse;                                         /* [T]; ignored rows get 0 */
  float* acc;                                         /* as tfx_ce_w_args */
  float z_weight, smoothing;
  float* aux;                                         /* as tfx_ce_w_args */
  const float* row_w;                                 /* [T] */
  float* row_loss;                                    /* [T]: w r; ignored rows get 0 */
} tfx_ce_rows_args;
int tfx_ce_rows_fwd(const tfx_ce_rows_args* a, void* stream);

/* fused MSE forward + backward: pred/flow fp32 [R, dl]   T:3359-3362 */
typedef struct {
  int32_t R, dl; const float* pred; int32_t ld_pred; const float* flow;
  float grad_scale;                           /* 2 * weight / (R*dl) */
  tfx_bf16* dpred; int32_t ld_d;              /* bf16 [R, ld_d], pad columns zeroed */
  float* acc;                                 /* acc[0] += sum of squared error */
  int32_t accumulate;                         /* != 0: dpred += gradient (a second target on the same prediction: the
                                                 velocity-consistency term T:3394-3418), else dpred = gradient */
  /* model_output_clean (T:1297, MP:100-126): `pred` already holds (out - noised) / max(1 - t, clean_eps) (tfx_output_to_flow);
   * the gradient wrt the model output carries the same 1 / max(1 - t, clean_eps).  row_inst NULL = off */
  const int32_t* row_inst; const float* inst_time; float clean_eps;
  /* reconstruction loss (`reconstruction_loss_weight`, MP:177-200 / T:2840-2853): recon_w non-NULL switches the residual to
   *   (1 - t) pred - c flow,   t = recon_time[recon_inst[row]],   c = t (recon_mode 0: target = the noised latent, interleaved forward)
   *                                                               c = 1 (recon_mode 1: target = the clean latent, forward_modality)
   * - algebraically noised - (noise + pred (1 - t)) resp. clean - (noise + pred (1 - t)) with flow = clean - noise - and weights every row by
   * recon_w[row] (1 / (instances of the type x rows of the instance): the reference averages per-instance means); acc += sum w r^2,
   * d pred (+)= grad_scale w (1 - t) r */
  const float* recon_w; const int32_t* recon_inst; const float* recon_time; int32_t recon_mode;
} tfx_mse_args;
int tfx_mse_fwd_bwd(const tfx_mse_args* a, void* stream);
/* the same squared error with one LOSS WEIGHT PER ROW (row_w, [R] floats >= 0, required: NULL returns -1 before any launch) and without the
 * reconstruction form:  acc[0] += sum_r w_r sum_c err^2,  dpred (+)= grad_scale w_r err (clean factor).  A row with w_r == 0 is not read and writes exact
 * zeros (with `accumulate` it adds nothing); w_r = 1.0f gives tfx_mse_fwd_bwd's dpred to the bit.  The other fields are tfx_mse_args'. */
typedef struct {
  int32_t R, dl; const float* pred; int32_t ld_pred; const float* flow;
  float grad_scale;
  tfx_bf16* dpred; int32_t ld_d;
  float* acc;
  int32_t accumulate;
  const int32_t* row_inst; const float* inst_time; float clean_eps;
  const float* row_w;                         /* [R] */
} tfx_mse_w_args;
int tfx_mse_w_fwd_bwd(const tfx_mse_w_args* a, void* stream);
/* the forward half of tfx_mse_w_fwd_bwd with the ROW SUMS as an output (per-token losses):  acc[0] += sum_r w_r sum_c err^2  exactly as that kernel forms it
 * (the same element order: `ld_d` is the row pitch of the d pred its backward will write, a multiple of 64 here, so that a wave's 64 elements lie in one row),
 * and  row_sse[r] += w_r sum_c err^2  (row_sse: [R] floats the caller zeroes, as it zeroes acc; ld_d / 64 atomics per row that counts).  A row with w_r == 0
 * is not read and adds nothing.  No gradient is written - the `model_output_clean` factor scales only the gradient, so the forward carries none of its
 * fields; the backward is tfx_mse_w_fwd_bwd under the caller's row weights, its `acc` pointing at scratch.  NULL row_w or row_sse, ld_d % 64: -1. */
typedef struct {
  int32_t R, dl; const float* pred; int32_t ld_pred; const float* flow;
  int32_t ld_d;
  float* acc;
  const float* row_w;                         /* [R] */
  float* row_sse;                             /* [R], += */
} tfx_mse_rows_args;
int tfx_mse_rows_fwd(const tfx_mse_rows_args* a, void* stream);
/* fused cosine loss forward + backward over bf16 rows (the Self-Flow representation loss, default_rep_loss_fn: 1 - cosine_similarity(pred, target, -1).mean()):
 *   c_t = <x_t, y_t> / (max(|x_t|, 1e-8) max(|y_t|, 1e-8)),   acc[0] += sum of c_t over the rows that count (the host forms 1 - acc / N),
 *   dpred_t = -grad_scale (y_t / (|x_t| |y_t|) - c_t x_t / |x_t|^2)   in bf16, zero for the rows that do not count.
 * The rows are (b, n_pad) token rows of a plan: row t counts when t % n_pad < n_valid (n_pad == 0: every row).  fp32 arithmetic, one pass: each operand is read
 * once, dpred written once.  d a multiple of 64, <= 2048; leading dimensions multiples of 8. */
typedef struct {
  int32_t T, d; const tfx_bf16* pred; int32_t ld_pred; const tfx_bf16* target; int32_t ld_target;
  int32_t n_pad, n_valid;
  float grad_scale;                           /* weight / (number of rows that count) */
  tfx_bf16* dpred; int32_t ld_d;
  float* acc;
} tfx_cosine_args;
int tfx_cosine_fwd_bwd(const tfx_cosine_args* a, void* stream);
/* model_output_clean: pred[r][c] <- (pred[r][c] - noised[r][c]) / max(1 - t_r, clean_eps), noised = eps ? x*t + eps*(1-t) : x,
 * t_r = inst_time[row_inst[r]]   (get_model_output_to_flow_fn, MP:100-126) */
int tfx_output_to_flow(float* pred, const float* x, const float* eps, const int32_t* row_inst, const float* inst_time,
                       int32_t R, int32_t dl, float clean_eps, void* stream);

/* ---- sampling (sample_many, T:2082-2583) ------------------------------------------------------ */
/* sample_text_token (T:597-605) with min_p_filter (T:591-595), one row of fp32 logits [B, ld] (V valid columns) per sample, on the device:
 * temperature == 0 -> argmax (first index on ties); else p = softmax(logits / temperature), tokens with p < min_p * max p are removed and
 * the survivor whose cumulative mass (index order) crosses uniforms[row] * (surviving mass) is drawn.  Rows with active[row] == 0 are left
 * untouched (active NULL = all rows).  out_ids: int32 [B]. */
int tfx_sample_tokens(const float* logits, int32_t ld, int32_t B, int32_t V, float temperature, float min_p, const float* uniforms,
                      const int32_t* active, int32_t* out_ids, void* stream);
/* the same with the DRAW restricted to the first V_draw columns while the maximum (hence the min-p threshold, and the argmax at temperature 0)
 * still runs over all V: `generate_text_only` (T:2690-2698) filters over every logit, then masks everything but the text tokens.
 * Fallbacks of both entries, when the inverse-CDF scan ends without crossing the target: (1) fp32 rounding (uniforms[row] close to 1: the total and the
 * prefix sums add the same terms in different orders) -> the LAST surviving column below V_draw; (2) no column below V_draw survives the min-p filter
 * (only with V_draw < V: the maximum lies in a masked column) -> V_draw, the first masked column - the reference's masked logits are all -finfo.max
 * there and its argmax takes the first.  temperature < 0 is refused (-3) by both. */
int tfx_sample_tokens_range(const float* logits, int32_t ld, int32_t B, int32_t V, int32_t V_draw, float temperature, float min_p, const float* uniforms,
                            const int32_t* active, int32_t* out_ids, void* stream);
/* The range draw behind top-k and top-p (nucleus) filters next to min-p, one launch.  These two filters are NOT the reference's (it has min-p only);
 * they are pinned to this text.  Per row: V valid fp32 logits, candidates = the columns c < V_draw (V_draw <= V), temperature T > 0, min_p >= 0,
 * top_k >= 0, top_p > 0;  l_max = the maximum over ALL V columns,  r_c = exp((l_c - l_max) / T).
 *   top-k  (top_k == 0: off)  l_(k) = the k-th largest candidate logit; a candidate survives iff l_c >= l_(k).  Ties at the k-th place all survive;
 *          top_k >= V_draw keeps every candidate.  The comparison is on logits, not on r (-0 and +0 are equal).
 *   top-p  (top_p >= 1: off)  over the top-k survivors S:  M = sum of r over S,  G(x) = sum of r_c over c in S with r_c > x;  c survives iff
 *          G(r_c) < top_p M - the smallest descending prefix whose mass reaches top_p, ties at its boundary all kept.  A threshold set
 *          {r_c >= tau_p}, independent of the index order, never empty (the best candidate has G = 0).
 *   min-p  as above: r_c >= min_p, against the global maximum - which with V_draw < V may lie outside the draw range.
 * The surviving set is the intersection of the three (= the usual temperature -> top-k -> top-p -> min-p chain: min-p relative to the maximum does
 * not change under renormalisation), i.e. two thresholds per row: one on the logit, and max(tau_p, min_p) on r.  The mass pass and the inverse-CDF
 * scan then run as in tfx_sample_tokens_range, in index order, with its fallbacks: rounding at u close to 1 -> the last survivor below V_draw; no
 * survivor (only from min-p with V_draw < V) -> V_draw.  temperature == 0: the argmax over all V, filters ignored.  r_c is spelled once and the
 * membership test is the same, bit for bit, in the threshold searches, the mass pass and the scan.  With top_k == 0 and top_p >= 1 the ids are those of
 * tfx_sample_tokens_range for the same uniforms, exactly.  Returns -3 and launches nothing for temperature < 0, top_k < 0, top_p <= 0 or NaN,
 * V_draw < 1 or V_draw > V.
 * Method: both thresholds by a 16-way search over bit patterns, 4 bits per pass - top-k over the order-preserving integer key of the logit (the
 * largest t with count(key >= t) >= k), top-p over the bit pattern of r (the largest x with G(x) >= top_p M; fp32 addition in a fixed order is
 * monotone in every term, so the fp32 G does not grow with x).  Passes over the row: 1 (maximum) + 8 (top-k, if on) + 1 + 8 (M and top-p, if on)
 * + 2 (mass, scan); no host round trip.  Width classes: V <= TFX_SAMPLE_NARROW_MAX - one wave per row, four rows per block; wider - one block of
 * 16 waves per row, whose first wave alone makes the mass pass and the scan (so "filters off" is tfx_sample_tokens_range at every width).
 * Rounding of M and G (all terms >= 0, so relative to the sum itself): each thread adds its ceil(V_draw / (64 W)) columns in index order (W = 1 or
 * 16 waves per row), a 6-step wave tree follows, then the W wave totals are added in wave order:
 *     |error| <= (ceil(V_draw / (64 W)) + 6 + W - 1) 2^-24     W = 1: 1.3e-6 at 1024 columns;  W = 16: 1.5e-6 at 4100 and 3.2e-6 at 32 000 columns;
 * r itself carries the error of the hardware exponential, about 2e-6 relative at |argument| <= 20.  A row whose M (or top_p M) underflows to 0 in
 * fp32 is left unfiltered by top-p; no column of such a row with r == 0 is drawn. */
enum { TFX_SAMPLE_NARROW_MAX = 1024 };
int tfx_sample_tokens_filtered(const float* logits, int32_t ld, int32_t B, int32_t V, int32_t V_draw, float temperature, float min_p, int32_t top_k,
                               float top_p, const float* uniforms, const int32_t* active, int32_t* out_ids, void* stream);
/* ODE state update of the fixed-grid midpoint solver (torchdiffeq semantics; T:2468-2525) fused with classifier-free
 * guidance (T:2516-2521): f = f_uncond ? f_uncond + cfg_scale * (f_cond - f_uncond) : f_cond;  out = y + a * f   (fp32, n elements) */
int tfx_ode_axpy(const float* y, const float* f_cond, const float* f_uncond, float cfg_scale, float a, float* out, int64_t n, void* stream);
/* The same solver as a per-sample state machine (continuous decode schedule: in one forward every sample is at its OWN evaluation).
 * y, ym: fp32 [B][Lc][dmax] - the state at the start of a solver step and its midpoint; ctl: fp32 [2][B] = per sample (mode, coefficient a):
 *   mode 1  first evaluation of a step:  input y,  result ym = y + a f        mode 3  a finished block re-encoded at t = 1: input y, no update
 *   mode 2  second evaluation:           input ym, result y  = y + a f        mode 0  the sample is not inside a modality
 * tfx_ode_stage writes the evaluation inputs into the plan's latent rows: x[(h B + i) Lq + j][c] = input_i[j][c] (h < H halves, j < Lc, c < dl; x: [H B Lq][dl]).
 * tfx_ode_update applies the results: f = pred[i Lq + j] (H == 1) or, with guidance (H == 2, T:2516-2521), pu + cfg_scale (pc - pu) with
 * pc = pred[i Lq + j], pu = pred[(B + i) Lq + j]; samples with sel[i] == 0 are skipped (sel NULL = all: one call per modality type).
 * rows0 (optional, compacted decode steps): int32 [H B], the first latent row of the block of (half h, sample i) - rows0[h B + i] + j replaces
 * (h B + i) Lq + j in both kernels; a negative entry = that half carries no block this step (nothing written / read there). */
int tfx_ode_stage(const float* y, const float* ym, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, float* x, int32_t H, int32_t Lq, int32_t dl,
                  const int32_t* rows0, void* stream);
int tfx_ode_update(float* y, float* ym, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq, int32_t dl,
                   float cfg_scale, const float* sel, const int32_t* rows0, void* stream);
/* Explicit Runge-Kutta solvers on the same fixed grid, up to TFX_ODE_MAX_STAGES stages per step (transfusion_pytorch_amd/ode.py holds the tableaus:
 * euler, heun2, heun3, rk4 = torchdiffeq's 3/8 rule; the midpoint rule keeps the three entry points above).  With the guided derivative of a stage
 *   g = f_uncond ? fmaf(cfg_scale, f_cond - f_uncond, f_uncond) : f_cond
 * every state / stage input is formed by ONE prescribed fp32 sequence, the same in the three kernels:
 *   acc = y;  for j = 0 .. nk - 1 ascending: if (w_j != 0) acc = fmaf(w_j, k_j, acc);  [acc = fmaf(w_nk, g, acc) - the g term last]
 * A term whose weight is exactly 0 is skipped and its k_j is NOT read (a slot never written may hold anything); k_j with j >= nk is never read.
 *
 * tfx_ode_rk_axpy - the dense form, one launch per evaluation (n elements): k_j = k + j k_stride (j < nk <= 3; k may be NULL when nk == 0),
 *   g -> k_out (optional), fmaf(w_nk, g, acc) -> out (optional; the next stage's input, or the new state after the last stage).
 *   Returns -1 (y / f_cond missing, or neither output given), -2 (nk outside [0, 3]), -3 (nk > 0 without k, or k_stride < n).
 * tfx_ode_rk_stage / tfx_ode_rk_update - the per-sample state machine; B, Lc, dmax, H, Lq, dl, rows0, sel as in tfx_ode_stage / tfx_ode_update.
 *   y: fp32 [B][Lc][dmax];  k: fp32 [3][B][Lc][dmax], the stage derivatives k_0 .. k_2;  ctl: fp32 [9][B], per sample
 *     ctl[0] mode   ctl[1] stage index q   ctl[2..4] stage weights wa_0 .. wa_2   ctl[5..8] update weights wb_0 .. wb_3
 *     mode 1  a stage that is not the last of its step: input y + sum_{j<q} wa_j k_j, result k_q = g
 *     mode 2  the last stage of a step:                 same input,                   result y = y + sum_{j<q} wb_j k_j + wb_q g
 *     mode 3  a finished block re-encoded at t = 1: input y, no update        mode 0 (or anything else)  not inside a modality: nothing read or written
 *   The stage kernel writes the input to the latent rows of both halves exactly where tfx_ode_stage does.  Columns >= dl, samples with sel[i] == 0
 *   (update) and halves with a negative rows0 entry are neither read nor written.  The table lives on the device, so a stage index cannot be
 *   checked on the host: it is clamped to [0, 3], and a mode 1 sample at index 3 (no k slot) is skipped - k is never indexed past its 3 slots. */
enum { TFX_ODE_MAX_STAGES = 4 };
int tfx_ode_rk_axpy(const float* y, const float* k, int64_t k_stride, int32_t nk, float w0, float w1, float w2, float w3, const float* f_cond,
                    const float* f_uncond, float cfg_scale, float* k_out, float* out, int64_t n, void* stream);
int tfx_ode_rk_stage(const float* y, const float* k, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, float* x, int32_t H, int32_t Lq, int32_t dl,
                     const int32_t* rows0, void* stream);
int tfx_ode_rk_update(float* y, float* k, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq, int32_t dl,
                      float cfg_scale, const float* sel, const int32_t* rows0, void* stream);
/* Adams-Bashforth multistep rules on the same grid (ode.py: ab2 / ab3 / ab4 = order P): the first P - 1 steps are steps of a tableau rule above whose
 * stage-0 derivative is also kept in a ring of TFX_ODE_AB_HIST slots; every later step is ONE evaluation g = guided derivative at (t_n, y_n) and
 *   acc = y;  [state machine: the k terms j < q ascending, as above;]  for j = 0, 1, 2 in table order: if (w_j != 0) acc = fmaf(w_j, h_j, acc);
 *   new state = fmaf(w_g, g, acc);  g -> its slot
 * A history term whose weight is exactly 0 is skipped and its slot is NOT read.  Every read of an element comes before its writes, so the slot that
 * receives g may be one of the slots read (ab4: g_n replaces g_{n-3}).
 *
 * tfx_ode_ab_axpy - the dense form (n elements): h_j may be NULL when w_j == 0; g -> g_out (optional, may alias one h_j), the new state -> out.
 *   Returns 0 without a launch when n <= 0, -1 (y / f_cond / out missing), -3 (a nonzero w_j with h_j NULL).
 * tfx_ode_ab_update - tfx_ode_rk_update with the ring: hist fp32 [3][B][Lc][dmax]; ctl fp32 [16][B], rows 0..8 as tfx_ode_rk_update reads them,
 *     ctl[9] the slot that receives g (negative = none)   ctl[10..12] the slots read   ctl[13..15] their weights
 *   modes 1 and 2 with ctl[9] >= 0: g is also written to hist[slot];  mode 2: the history terms join the update as above.  Everything else - sel,
 *   rows0, H, columns >= dl, modes 0 and 3, the stage index clamp - as tfx_ode_rk_update; slot indices are clamped to [0, 2] likewise (the table
 *   lives on the device).  With ctl[9] negative and three zero weights the results are tfx_ode_rk_update's bits and hist is not touched.
 *   The inputs are staged by tfx_ode_rk_stage from rows 0..4 of the same block: a multistep evaluation is mode 2 at stage 0, its input y. */
enum { TFX_ODE_AB_HIST = 3 };
int tfx_ode_ab_axpy(const float* y, const float* h0, const float* h1, const float* h2, float w0, float w1, float w2, float wg, const float* f_cond,
                    const float* f_uncond, float cfg_scale, float* g_out, float* out, int64_t n, void* stream);
int tfx_ode_ab_update(float* y, float* k, float* hist, const float* ctl, int32_t B, int32_t Lc, int32_t dmax, const float* pred, int32_t H, int32_t Lq,
                      int32_t dl, float cfg_scale, const float* sel, const int32_t* rows0, void* stream);

/* ---- parameter plumbing ---------------------------------------------------------------------- */
/* dst[r][c] (bf16, ld_dst, Rd rows, Cd cols) = src[rowmap ? rowmap[r] : r][c] or 0 when out of range / map < 0 */
typedef struct { const float* src; int32_t ld_src, Rs, Cs; const int32_t* rowmap; tfx_bf16* dst; int32_t ld_dst, Rd, Cd; } tfx_cast_args;
int tfx_cast_rows(const tfx_cast_args* a, void* stream);
/* dst[c][r] = src[rowmap ? rowmap[r] : r][c]  (transposed shadow for the dX GEMMs).  Both return 0 without a launch when Rd == 0 or ld_dst == 0. */
int tfx_cast_rows_t(const tfx_cast_args* a, void* stream);
/* all shadows in one launch: `jobs_dev` is a DEVICE array of n_jobs jobs sorted by first_block; job j owns blocks
 * [first_block, first_block + nb) with nb = ceil(Rd*ld_dst/2048) (plain) or ceil(ld_dst/64)*ceil(Rd/64) (transposed);
 * n_blocks is the total; ld_dst % 8 == 0.  Fields as in tfx_cast_args. */
typedef struct { const float* src; int32_t ld_src, Rs, Cs; const int32_t* rowmap; tfx_bf16* dst; int32_t ld_dst, Rd, Cd; int32_t transposed, first_block; } tfx_cast_job;
int tfx_cast_batch(const tfx_cast_job* jobs_dev, int32_t n_jobs, int32_t n_blocks, void* stream);
/* out_f32[i] = gather of fp32 vector through a map (bias shadows): dst[i] = map[i] >= 0 ? src[map[i]] : 0 */
int tfx_gather_f32(const float* src, const int32_t* map, float* dst, int32_t n, void* stream);
/* out[t][c] (bf16, ld % 8 == 0) = 1 if token t is text and max(ids[t],0) == c else 0  (embedding-gradient GEMM operand) */
int tfx_onehot_bf16(const int32_t* ids, const int32_t* tok_inst, tfx_bf16* out, int32_t T, int32_t ld, void* stream);
/* dst[rowmap[r]][0:cols] = src[r][0:cols] for rowmap[r] >= 0   (KV-cache append; bf16, cols % 8 == 0) */
int tfx_scatter_rows_bf16(const tfx_bf16* src, int32_t ld_src, int32_t cols, tfx_bf16* dst, int32_t ld_dst, const int32_t* rowmap, int32_t R, void* stream);
int tfx_f32_to_bf16(const float* src, tfx_bf16* dst, int64_t n, void* stream);
/* dst[r][c] (bf16, row stride ld_dst) = src[r][c] (fp32, row stride ld_src) for an R x C block inside larger matrices (C, both strides and both base
 * offsets multiples of 8): the per-layer slice of the AdaLN table gradients, cast as soon as that layer's backward has finished */
int tfx_cast_block_bf16(const float* src, int32_t ld_src, tfx_bf16* dst, int32_t ld_dst, int32_t R, int32_t C, void* stream);
/* dst(bf16) = a(bf16) * silu'(pre(bf16))  (time-MLP backward) */
int tfx_silu_bwd(const tfx_bf16* dy, const tfx_bf16* pre, tfx_bf16* dx, int64_t n, void* stream);
/* column sums: out[c] += sum_r src[r][c]  (bias gradients); src bf16 or fp32.  tfx_colsum_bf16 takes two optional maps:
 *   rowmap [R]: row r of the sum is src[rowmap[r]]; an entry below 0 names no row and adds nothing (as in tfx_cast_rows, tfx_scatter_rows_bf16 and
 *               tfx_gather_f32); rows may repeat, and then count as often
 *   colmap [C]: column c is added to out[colmap[c]]; an entry below 0 drops the column; several columns may share one output, which receives their sum
 * A column whose sum is exactly zero does not touch `out`.  C % 8 == 0 && ld % 8 == 0 takes the 16-byte-load kernel (src 16-byte aligned), anything else the
 * scalar one.  R == 0 or C == 0 returns 0 and writes nothing. */
int tfx_colsum_bf16(const tfx_bf16* src, int32_t ld, int32_t R, int32_t C, const int32_t* colmap, const int32_t* rowmap, float* out, void* stream);
int tfx_colsum_f32(const float* src, int32_t ld, int32_t R, int32_t C, float* out, void* stream);
int tfx_add_bf16(const tfx_bf16* a, const tfx_bf16* b, tfx_bf16* out, int64_t n, void* stream);
/* x[i] *= *scale (in place; bf16 values, the fp32 scalar lives ON THE DEVICE so that no host sync is needed to read it).  A scale of
 * exactly 1.0 makes every block return before touching memory: `loss.backward()` with the default upstream gradient costs a launch,
 * not a pass over the loss seeds (autograd hands d total / d loss over as a device tensor, T: train_toy.py:53) */
int tfx_scale_bf16_dev(tfx_bf16* x, int64_t n, const float* scale, void* stream);
/* dst[i] = scale * src[i] (bf16, host scalar): the negated loss seed of the model-space model_output_clean backward */
int tfx_scale_bf16_copy(const tfx_bf16* src, tfx_bf16* dst, int64_t n, float scale, void* stream);

/* fused global-norm clip + Adam over flat fp32 buffers   train_toy.py:55-57
 * sumsq[0] must hold the sum of squared gradients (tfx_sumsq accumulates into it; zero it first).  g must be 16-byte aligned (16-byte loads): tfx_sumsq
 * returns -1 otherwise, as tfx_sumsq_det and tfx_ema_update do; n == 0 returns 0 and writes nothing. */
int tfx_sumsq(const float* g, int64_t n, float* sumsq, void* stream);
typedef struct {
  float* p; const float* g; float* m; float* v; int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
  int32_t step; const float* sumsq;
  /* grown at the end (zero / NULL = the behaviour before): DEVICE table of `nskip` sorted, disjoint [start, end) element ranges (2 nskip int64) the
   * kernel leaves untouched - p, m and v of the matrices another rule updates (tfx_muon_*).  Starts and ends are multiples of 4, the elements of one
   * thread (the flat buffer's segments are padded to 4): a group is skipped whole or not at all, and the arithmetic of every other element is the
   * kernel's own.  sumsq still covers the whole buffer. */
  const int64_t* skip; int32_t nskip;
} tfx_adam_args;
int tfx_adam_step(const tfx_adam_args* a, void* stream);

/* the same launch with parameter groups and decoupled (AdamW) weight decay.  The struct BEGINS with the fields of tfx_adam_args, in its order and
 * layout (tfx_adam_args itself keeps its size for the callers that pass it); what follows:
 *   decoupled   the ungrouped rule: 0 = L2 (g += weight_decay p, tfx_adam_step's), 1 = torch.optim.AdamW's (p *= 1 - lr weight_decay, then the Adam update
 *               without a decay term in g)
 *   ranges      DEVICE table of `nrange` sorted, disjoint [start, end) element ranges with a group index each: 3 nrange int64 (start, end, group).  Starts
 *               and ends are multiples of 4 (the elements of one thread: the flat buffer's segments are padded to 4, the padding belongs to the segment's
 *               range).  Elements in no range belong to group 0.  The group is decided once per block where the block's 1024 elements lie in one range,
 *               per thread only in blocks that straddle a boundary.
 *   group_*     the records of `ngroup` <= TFX_ADAM_MAX_GROUPS groups BY VALUE (a schedule changes lr every step: nothing to copy to the device); with
 *               nrange > 0 the kernel reads these in place of lr, beta1, beta2, eps, weight_decay and decoupled.  Bias corrections per group on the
 *               host side of the launch, from the ONE `step`.
 * nrange == 0 and decoupled == 0 IS tfx_adam_step (the same kernel on the same fields).  Otherwise the per-element operations are that kernel's, in its
 * order, with the group's scalars: groups that all carry the global values give its bits.  `skip` composes (skipped elements stay untouched whatever
 * their group), the clip coefficient (sumsq, max_norm, grad_scale) is one for all groups. */
enum { TFX_ADAM_MAX_GROUPS = 8 };
typedef struct {
  float* p; const float* g; float* m; float* v; int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
  int32_t step; const float* sumsq;
  const int64_t* skip; int32_t nskip;
  int32_t decoupled;
  const int64_t* ranges; int32_t nrange, ngroup;
  float group_lr[TFX_ADAM_MAX_GROUPS], group_beta1[TFX_ADAM_MAX_GROUPS], group_beta2[TFX_ADAM_MAX_GROUPS], group_eps[TFX_ADAM_MAX_GROUPS],
        group_weight_decay[TFX_ADAM_MAX_GROUPS];
  int32_t group_decoupled[TFX_ADAM_MAX_GROUPS];
} tfx_adam_group_args;
int tfx_adam_step_groups(const tfx_adam_group_args* a, void* stream);

/* the Adam-atan2 rule over the same flat buffers (Everett et al., "Scaling Exponents Across Parameterizations and Optimizers", 2024; the defaults a = 1.27,
 * b = 1 are the adam_atan2_pytorch package's as published).  RESTATED from the published definition and parity-unpinned: the package is not vendored with
 * the reference (train_image_only.py:90 imports it), so no run of it stands behind these bits.  Per element, fp32, every rounding spelled out:
 *   g = g coef;  w = p keep;  g = fma(l2, w, g) if l2 != 0;  m = fma(beta1, m, (1 - beta1) g);  v = fma(beta2, v, g ((1 - beta2) g))
 *   p = w - (lr a) atan2f(m (1 / bc1), sqrt(v) (b / sqrt(bc2)))          bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * coef, keep (1 - lr wd where decoupled, else 1), l2 (wd for the L2 form, else 0) and the moment updates are tfx_adam_step_groups'; 1 / bc1,
 * b / sqrt(bc2) and lr a are formed once per group on the host side of the launch, from the ONE `step`.  There is no eps: atan2(0, 0) = 0 (an element
 * with zero gradient and zero state does not move), the second argument is never negative, so every element moves by at most lr a pi / 2, and the
 * step does not change when every gradient is scaled by one factor.
 * The struct BEGINS with the fields of tfx_adam_group_args, in its order and layout (skip, ranges, groups and the clip coefficient mean what they
 * mean there); `eps` / `group_eps` are present and ignored.  One rule per launch: every group takes atan2.  Not built: the package's cautious_factor
 * and regen_reg_rate, and its own Muon arithmetic (FusedMuonAdamAtan2 keeps tfx_muon_*).
 * Supported magnitudes: g coef must be a normal fp32 number whose square is normal too, roughly 1e-18 <= |g coef| <= 1e18.  Below that v underflows to
 * zero and the rule returns +-pi / 2 where exact arithmetic would not; above it v overflows.  Gradients behind a global clip are far inside the range.
 * Returns non-zero, launching nothing, for atan2_a <= 0, atan2_b <= 0, step < 1 and whatever tfx_adam_step_groups rejects. */
typedef struct {
  float* p; const float* g; float* m; float* v; int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
  int32_t step; const float* sumsq;
  const int64_t* skip; int32_t nskip;
  int32_t decoupled;
  const int64_t* ranges; int32_t nrange, ngroup;
  float group_lr[TFX_ADAM_MAX_GROUPS], group_beta1[TFX_ADAM_MAX_GROUPS], group_beta2[TFX_ADAM_MAX_GROUPS], group_eps[TFX_ADAM_MAX_GROUPS],
        group_weight_decay[TFX_ADAM_MAX_GROUPS];
  int32_t group_decoupled[TFX_ADAM_MAX_GROUPS];
  float atan2_a, atan2_b;
} tfx_adam_atan2_args;
int tfx_adam_atan2_step(const tfx_adam_atan2_args* a, void* stream);

/* ---- Muon (torch/optim/_muon.py) ---------------------------------------------------------------
 * One optimizer step over ALL matrices of Transfusion.muon_parameters() (T:1657-1672) in a number of launches that does not depend on their count:
 *   tfx_sumsq_det (2 launches) -> tfx_muon_prep -> tfx_muon_norm -> ns_steps x { gram, poly, update: tfx_muon_gemm } -> tfx_muon_apply -> tfx_adam_step(skip)
 * (or tfx_adam_atan2_step(skip) at the end of the chain: the same launch count).  No atomics, no sum whose order varies: the path is run-to-run bit-deterministic.
 *
 * Orientation and padding (_muon.py:50-52): a rows x cols parameter is iterated as X, m x n with m = min, n = max (transposed when rows > cols).  The bf16
 * workspace keeps X (m_pad x n_pad) AND X^T (n_pad x m_pad), zero-padded to multiples of the 128 x 128 tile; zero rows / columns stay zero under the
 * iteration.  The "straight" copy has the parameter's own orientation (X when rows <= cols, else X^T), the "transposed" copy the other one. */
enum { TFX_SUMSQ_DET_PARTIALS = 1024 };
/* sumsq[0] = sum of g[i]^2 (overwritten, not accumulated) in a fixed order; partials: TFX_SUMSQ_DET_PARTIALS floats of scratch.  The clip norm of the Muon step
 * (clip_grad_norm_, train_toy.py:55): tfx_sumsq's atomic sum changes in the last bits from run to run.  n == 0 stores 0; g not 16-byte aligned returns -1.
 * tfx_muon_prep / _apply with nblk == 0 and tfx_muon_norm with nmat == 0 return 0 and write nothing. */
int tfx_sumsq_det(const float* g, int64_t n, float* partials, float* sumsq, void* stream);
/* host only: what a rows x cols parameter becomes - flip (rows > cols), m <= n, their padded sizes, output tiles of its gram / poly product (m_pad x m_pad)
 * and of its update product (n_pad x m_pad), 64 x 64 blocks of tfx_muon_prep / _apply.  Any output pointer may be NULL. */
int tfx_muon_plan(int32_t rows, int32_t cols, int32_t* flip, int32_t* m, int32_t* n, int32_t* m_pad, int32_t* n_pad, int32_t* gram_tiles,
                  int32_t* update_tiles, int32_t* prep_blocks);
/* host only: kernel launches of one optimizer step (the chain above) for ns_steps iterations over nmat matrices - the same for every nmat >= 1 */
int tfx_muon_step_launches(int32_t ns_steps, int32_t nmat);
typedef struct {
  int64_t off;                 /* element offset of the rows x cols fp32 matrix in the flat buffers (parameters, gradients, momentum) */
  int64_t s_off, t_off;        /* element offsets in the bf16 workspace of the straight copy (rows x ld_s) and the transposed copy (cols x ld_t) */
  int32_t rows, cols, ld_s, ld_t;
  int32_t blk0;                /* first 64 x 64 block of this matrix in the prep / apply grid (= its first entry in `partials`) */
  float lr_ratio;              /* _adjust_lr's ratio for this shape (_muon.py:65-77) */
} tfx_muon_mat;
/* momentum, Nesterov mix, bf16 X0 in both orientations, per-block sums of squares (_muon.py:280-282): block b works on matrix blk_mat[b].
 * g is scaled by grad_scale x the clip coefficient of tfx_adam_step (sumsq, max_norm) before it enters the momentum - the
 * product is rounded to fp32 on its own, as clip_grad_norm_ leaves it, so that `buf` stays within 2 ulp of torch.lerp on the same operands.  X0 is stored UNNORMALISED; tfx_muon_norm
 * turns the partials into 1 / max(|u|, eps) and its square per matrix, which the first gram product and the first update carry (scale_acc / scale_z).
 * Supported magnitudes: the first gram product sums u_i u_j in fp32 BEFORE 1 / |u|^2 is applied, so the products square the range: elements of u
 * below about 1e-19 in magnitude underflow there (contribute zero) and elements above about 1e19 overflow, where torch - which divides first - is
 * exact.  eps bounds 1 / |u|^2 (1e14 at the default 1e-7), so small inputs give zeros, never inf / NaN.  Gradients behind a global clip are far
 * inside the range. */
typedef struct {
  const tfx_muon_mat* mats; const int32_t* blk_mat; int32_t nmat, nblk;
  const float* g; float* buf; tfx_bf16* ws; float* partials;
  const float* sumsq; float max_norm, grad_scale, momentum; int32_t nesterov;
} tfx_muon_prep_args;
int tfx_muon_prep(const tfx_muon_prep_args* a, void* stream);
/* inv[2 i] = 1 / max(sqrt(sum of matrix i's partials), eps), inv[2 i + 1] = its square   (_muon.py:54) */
int tfx_muon_norm(const tfx_muon_mat* mats, int32_t nmat, const float* partials, float eps, float* inv, void* stream);
/* one problem of a grouped launch: C (M x N) = alpha scale_z Z + beta scale_acc P . Q^T, P: M x K, Q: N x K, all bf16, row-major, K contiguous, fp32
 * accumulation, one rounding of the result; Ct (optional) also receives the transposed result (N x M).  M, N multiples of 128, K of 64, leading dimensions of 8,
 * pointers 16-byte aligned: the kernel has no bounds predicate.  Z, Ct, scale_z, scale_acc may be NULL (no addend / no second copy / 1); the scales are DEVICE floats.
 * The three Newton-Schulz products (_muon.py:56-62): gram P = Q = X; poly P = Q = Z = A (A symmetric: A . A^T = A @ A); update P = Z = X^T, Q = B. */
typedef struct {
  const tfx_bf16* P; const tfx_bf16* Q; const tfx_bf16* Z; tfx_bf16* C; tfx_bf16* Ct;
  const float* scale_z; const float* scale_acc;
  int32_t M, N, K, ldp, ldq, ldz, ldc, ldct;
  int32_t tile0;               /* first tile of this problem in the launch's grid; its (M / 128) x (N / 128) tiles follow row-major */
  int32_t reserved;
} tfx_muon_gemm_problem;
/* table, tile_prob (problem index of every tile): DEVICE arrays; alpha, beta apply to every problem of the launch */
int tfx_muon_gemm(const tfx_muon_gemm_problem* table, const int32_t* tile_prob, int32_t ntiles, float alpha, float beta, void* stream);
/* p = p decay - lr lr_ratio O   (_muon.py:288-289; decay = 1 - lr weight_decay), O = the straight copy of the final iterate in `ws` */
typedef struct {
  const tfx_muon_mat* mats; const int32_t* blk_mat; int32_t nmat, nblk;
  float* p; const tfx_bf16* ws; float lr, decay;
} tfx_muon_apply_args;
int tfx_muon_apply(const tfx_muon_apply_args* a, void* stream);
/* exponential moving average of a flat parameter buffer: ema = decay * ema + (1 - decay) * online   (ema_pytorch EMA.update, used by
 * Transfusion.create_ema T:1681-1699) */
int tfx_ema_update(float* ema, const float* online, int64_t n, float decay, void* stream);

/* ---- data-parallel gradient exchange -----------------------------------
 * ONE all-reduce(sum) per range of the flat fp32 gradient buffer over RCCL / xGMI, one process per GPU (reference practice: DDP under
 * `accelerate`, train_mnist.py:114-126).  RCCL is bound at run time (dlopen), so a host that already carries a copy keeps using it.
 *   rank 0: tfx_allreduce_unique_id(id);  broadcast the 128 bytes by any host channel;  every rank: tfx_allreduce_init(rank, world, id)
 *   per step: tfx_allreduce_run(grad + offset, count, stream)  (in place, enqueued on `stream`; scale by 1 / world in tfx_adam_step.grad_scale) */
int tfx_allreduce_unique_id(void* out128);
int tfx_allreduce_init(int32_t rank, int32_t world, const void* unique_id128);
int tfx_allreduce_run(float* buf, int64_t count, void* stream);
int tfx_allreduce_destroy(void);

/* ---- LoRA adapters (transfusion_pytorch_amd/lora.py; csrc/lora.hip) ----------------------------------------
 * An adapted nn.Linear weight reads W_eff = W + s B A (A [r, d_in], B [d_out, r], fp32 parameters outside the flat buffer).
 *
 * tfx_lora_merge: Weff[n][k] = W[n][k] + s sum_j B[n][j] A[j][k], fp32 from fp32 operands, j ascending in one fma chain per element (no atomics,
 * no split): bit-identical from run to run.  An element whose low-rank sum is exactly zero (B = 0, r = 0) receives the bits of W.  r == 0 (A, B may
 * be NULL) is a plain copy.  Weff may not alias W.  The bf16 shadow casts of an adapted matrix then read Weff: one rounding, as for a trained master. */
typedef struct {
  const float* W; int32_t ldw;
  const float* B; int32_t ldb;          /* [N, r] */
  const float* A; int32_t lda;          /* [r, K] */
  float* Weff; int32_t ldo;
  int32_t N, K, r;
  float s;
} tfx_lora_merge_args;
int tfx_lora_merge(const tfx_lora_merge_args* a, void* stream);

/* tfx_lora_down: P[M, r_pad] = Q[M, K] . R[r_pad, K]^T, bf16 operands, fp32 accumulation on the matrix cores, bf16 P.  r_pad = 32 or 64 (rows of R past the
 * adapter's rank are zeros); K % 8 == 0, ldq % 8 == 0, ldr % 8 == 0, 16-byte aligned bases (columns from K on are never read); any ldp >= r_pad.  Q is read once:
 * a block owns 128 rows of Q and all of R's rows. */
typedef struct {
  const tfx_bf16* Q; int32_t ldq;
  const tfx_bf16* R; int32_t ldr;
  tfx_bf16* P; int32_t ldp;
  int32_t M, K, r_pad;
} tfx_lora_down_args;
int tfx_lora_down(const tfx_lora_down_args* a, void* stream);

/* tfx_lora_grad: G[j][k] (+)= alpha sum_m P[m][j] Q[m][k] for j < r, k < K: the skinny weight-gradient product of an adapter (P = the down projection of the
 * other operand, r <= r_pad in {32, 64} columns).  The M rows are cut into `chunks` runs (multiples of 64 rows); a block forms one (128-column, chunk) partial on
 * the matrix cores and writes it with plain stores into `partials` ([chunks, r_pad, ceil(K / 128) 128] fp32, owned by the caller: tfx_lora_grad_plan gives its
 * size); a second kernel adds the chunks in one fixed order (eight interleaved ascending chains, closed as a fixed tree), applies alpha and stores (accumulate == 0) or adds to (accumulate != 0) G.  No atomics: the result
 * is bit-identical from run to run.  The element (j, k) lands at G[j * g_row_stride + c * g_col_stride], c = colmap ? colmap[k] : k, columns with c < 0 are
 * dropped (physical operand layout -> the parameter's own order, and the transposed form dB [d_out, r] through g_row_stride = 1, g_col_stride = r).
 * K % 8 == 0, ldq % 8 == 0, 16-byte aligned Q; any ldp >= r_pad. */
typedef struct {
  const tfx_bf16* P; int32_t ldp;
  const tfx_bf16* Q; int32_t ldq;
  float* G; int64_t g_row_stride, g_col_stride;
  const int32_t* colmap;
  float* partials;
  int32_t M, K, r, r_pad;
  int32_t accumulate;
  float alpha;
} tfx_lora_grad_args;
int tfx_lora_grad(const tfx_lora_grad_args* a, void* stream);
/* what tfx_lora_grad would launch, without launching (host logic only): row chunks, blocks of the product kernel, floats of `partials` it needs */
int tfx_lora_grad_plan(const tfx_lora_grad_args* a, int32_t* chunks, int32_t* grid, int64_t* partial_floats);

/* ---- launch lists ------------------------------------------------------------------------------
 * The step is a STATIC list of launches over persistent buffers (engine.Plan), so the host replays it with ONE call instead of one
 * FFI round trip per kernel: `tfx_run_list` walks `n` items in order on `stream` (or the side stream, per item) and stops at the first non-zero return code
 * (its index is written to *failed_at).  `args` of a struct entry point is that entry point's args struct; entry points with
 * positional arguments take a `tfx_raw_args`: pointers fill p0.., integers i0.., floats f0 in declaration order. */
typedef struct { const void *p0, *p1, *p2, *p3, *p4; int64_t i0, i1, i2, i3; float f0; int32_t reserved; } tfx_raw_args;
enum { TFX_OP_GEMM_NT = 0, TFX_OP_GEMM_TN = 1, TFX_OP_ATTN_FWD = 2, TFX_OP_ATTN_BWD = 3, TFX_OP_ADALN_PRE_FWD = 4, TFX_OP_ADALN_PRE_BWD = 5,
       TFX_OP_ADALN_POST_FWD = 6, TFX_OP_ADALN_POST_BWD = 7, TFX_OP_QK_NORM_ROPE_FWD = 8, TFX_OP_QK_NORM_ROPE_BWD = 9, TFX_OP_ATTNRES_FWD = 10,
       TFX_OP_ATTNRES_BWD = 11, TFX_OP_RMSNORM_FWD = 12, TFX_OP_RMSNORM_BWD = 13, TFX_OP_EMBED_FWD = 14, TFX_OP_EMBED_BWD = 15,
       TFX_OP_NOISE_MIX = 16, TFX_OP_FOURIER = 17, TFX_OP_CE_FWD_BWD = 18, TFX_OP_MSE_FWD_BWD = 19, TFX_OP_CAST_ROWS = 20, TFX_OP_CAST_ROWS_T = 21,
       TFX_OP_ADAM_STEP = 22, TFX_OP_DECODE_ATTN = 23, TFX_OP_LASER_V_FWD = 24, TFX_OP_LASER_V_BWD = 25, TFX_OP_COSINE_FWD_BWD = 26,
       TFX_OP_ADAM_ATAN2_STEP = 27, TFX_OP_LORA_MERGE = 28, TFX_OP_LORA_DOWN = 29, TFX_OP_LORA_GRAD = 30, TFX_OP_CE_FWD = 31,
       /* positional entry points (args = tfx_raw_args) */
       TFX_OP_OUTPUT_TO_FLOW = 32, TFX_OP_GATHER_F32 = 33, TFX_OP_ONEHOT_BF16 = 34, TFX_OP_SCATTER_ROWS_BF16 = 35, TFX_OP_F32_TO_BF16 = 36,
       TFX_OP_SILU_BWD = 37, TFX_OP_COLSUM_BF16 = 38, TFX_OP_COLSUM_F32 = 39, TFX_OP_ADD_BF16 = 40, TFX_OP_SCALE_BF16_DEV = 41, TFX_OP_CAST_BLOCK_BF16 = 42, TFX_OP_SCALE_BF16_COPY = 43, TFX_OP_ADALN_POST_PRE_FWD = 44, TFX_OP_LAYER_END_FWD = 45,
       TFX_OP_ATTNRES_PREP = 46, TFX_OP_ATTNRES_PULL_BWD = 47, TFX_OP_ATTNRES_FINISH = 52, TFX_OP_ADALN_PRE_POST_BWD = 53,
       TFX_OP_CE_BWD = 54,                      /* (args = tfx_ce_chunk_args, as TFX_OP_CE_FWD: the struct codes below 32 are used up) */
       TFX_OP_CE_REG_FWD_BWD = 55,              /* (args = tfx_ce_reg_args) */
       TFX_OP_CE_REG_FWD = 56, TFX_OP_CE_REG_BWD = 57,      /* (args = tfx_ce_reg_chunk_args) */
       TFX_OP_CE_W_FWD_BWD = 58,                /* (args = tfx_ce_w_args) */
       TFX_OP_CE_W_FWD = 59, TFX_OP_CE_W_BWD = 60,          /* (args = tfx_ce_w_chunk_args) */
       TFX_OP_MSE_W_FWD_BWD = 61,               /* (args = tfx_mse_w_args) */
       TFX_OP_CE_ROWS_FWD = 62,                 /* (args = tfx_ce_rows_args) */
       TFX_OP_MSE_ROWS_FWD = 63,                /* (args = tfx_mse_rows_args) */
       /* stream control (args = any non-NULL pointer; `stream` = event slot 0..63):
          FORK: the library's side stream waits for everything enqueued so far on the caller's stream;
          JOIN_RECORD: mark "everything enqueued so far on the side stream";  JOIN_WAIT: the caller's stream waits for that mark;
          JOIN = JOIN_RECORD + JOIN_WAIT */
       TFX_OP_FORK = 48, TFX_OP_JOIN = 49, TFX_OP_JOIN_RECORD = 50, TFX_OP_JOIN_WAIT = 51 };
/* `stream`: 0 = the caller's stream, 1 = the library's side stream (a second HIP stream the weight-gradient GEMMs run on, next to
 * the data-gradient chain); for FORK / JOIN the event slot. */
typedef struct { int32_t op; int32_t stream; const void* args; } tfx_launch;
int tfx_run_list(const tfx_launch* list, int32_t n, void* stream, int32_t* failed_at);
/* hipGraph form of a launch list whose arguments live in DEVICE memory between replays (decode plans: token ids, cache positions, visible
 * lengths, rotary positions, times and latents are device arrays the host overwrites in place; every kernel argument is a fixed pointer or
 * size).  `tfx_graph_create` captures the list on a library-owned stream (nothing executes) and instantiates it; `tfx_graph_launch`
 * replays it on `stream`.  Kernel arguments are frozen at capture time: re-create the graph when an args struct of the list changes. */
int tfx_graph_create(const tfx_launch* list, int32_t n, void** graph_out);
/* the same capture with every item on ONE stream (FORK / JOIN items become no-ops, side-stream items run in list order): the chain form the training
 * lists are captured in (engine.replay_auto, TFX_TRAIN_GRAPH=1).  The single-stream mode holds for this call on this thread only - it does not touch
 * the process-wide switch of tfx_set_single_stream, so other threads' replays and fingerprints are unaffected. */
int tfx_graph_create_single(const tfx_launch* list, int32_t n, void** graph_out);
int tfx_graph_launch(void* graph, void* stream);
int tfx_graph_destroy(void* graph);
/* 64-bit fingerprint of everything a capture of the list would freeze: ops, stream tags, the bytes of every args struct (and of the host structs
 * the two-struct entry points point at), the single-stream switch.  A caller that replays a TRAINING list as a graph compares it with the
 * fingerprint the graph was captured under and re-captures (or replays the list) when a scalar / pointer of the step has changed. */
int tfx_list_fingerprint(const tfx_launch* list, int32_t n, int64_t* out);
/* on != 0: replay every item on the caller's stream (FORK / JOIN become no-ops) - same results, kernels one at a time (used to time a
 * kernel family without its side-stream neighbours); returns the previous setting.  PROCESS-wide: `loss.backward()` replays its list on PyTorch's
 * autograd thread, which must see what the main thread set. */
int tfx_set_single_stream(int32_t on);

const char* tfx_version(void);

#ifdef __cplusplus
}
#endif
#endif
