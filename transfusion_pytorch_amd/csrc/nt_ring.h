// The ring K loop of the 4-wave NT kernels: gemm.hip's glds / mid / skinny forms and muon.hip's grouped product.
//
// A block of 4 waves (2 x 2) owns a (64 MI) x 128 output tile, a wave (32 MI) x 64 of it = MI x 2 accumulators of v_mfma_f32_32x32x16_bf16 (operands
// multiplied swapped: a lane owns one output row and runs of 4 columns).  Both operands are K-contiguous and arrive by LDS-DMA, one 64-wide K-tile per
// ring slot, a slot = A [64 MI][64] then B [128][64] bf16; wave w stages rows [16 MI w, +16 MI) of A and [32 w, +32) of B in pieces of 8 rows x 128 B.
// The DMA writes lane-linear pieces, so the bank swizzle sits in the SOURCE address and in the read address: row r, 16-byte chunk c' holds global chunk
// c' ^ ((r >> 1) & 7) (ring_src_chunk / ldfrag), conflict-free for the ds_read_b128 lane groups.
//
// Per K-tile: wait until this wave's pieces of the tile have landed, barrier (everyone's have, and everyone finished reading the slot of the previous
// iteration), refill that slot with tile kt + ST - 1, four k-steps of MFMAs.  A wave's DMAs retire in order, so with `ahead` later tiles allowed in
// flight the wait is vmcnt(pieces per wave and tile x ahead): ring_wait generates the cases from the template parameters.  Every accumulator sums its
// K-tiles and k-steps front to back whatever MI / ST / DMA form: the forms give the same bits.
#pragma once
#include "tfx_common.h"

constexpr int RING_BN = 128, RING_BK = 64;
template <int MI> constexpr int ring_slot_elems = (64 * MI + RING_BN) * RING_BK;
template <int MI, int ST> constexpr int ring_bytes = ST * ring_slot_elems<MI> * 2;     // dynamic LDS of a launch; the epilogues restage in it (>= 64 KiB)

// piece j of wave w, in a tile of which every wave stages `per_wave` rows: the tile row this lane fetches, and the global chunk its LDS place must hold
TFX_DEV int ring_src_row(int w, int j, int per_wave) { return w * per_wave + j * 8 + ((threadIdx.x & 63) >> 3); }
TFX_DEV int ring_src_chunk(int row) { return (threadIdx.x & 7) ^ ((row >> 1) & 7); }

// s_waitcnt vmcnt(PER x min(ahead, MAXA)) as an if-chain over the immediates
template <int PER, int MAXA, int A = 0> TFX_DEV void ring_wait(int ahead) {
  if (A == MAXA || ahead == A) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER * A) : "memory");
  else if constexpr (A < MAXA) ring_wait<PER, MAXA, A + 1>(ahead);
}

// ASM_DMA: glds16_asm, which the compiler does not count, so ST - 2 tiles stay in flight across the wait; the builtin form (ST = 2) is drained by hipcc
// anyway.  a_src / b_src (piece j, k0) -> this lane's source of the K-tile at k0: row clamps, row maps and split operands are the caller's.
template <int MI, int ST, bool ASM_DMA, class SrcA, class SrcB>
TFX_DEV void nt_ring_loop(bf16* ring, int nk, f32x16 (&acc)[MI][2], SrcA a_src, SrcB b_src) {
  static_assert(ASM_DMA || ST == 2, "only the asm form may be left in flight");
  constexpr int BK = RING_BK, PA = 2 * MI, PB = 4, B0 = 64 * MI * BK;
  const int l = threadIdx.x & 63, hi = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto dma = [](const bf16* g, bf16* dst) { if constexpr (ASM_DMA) glds16_asm(g, dst); else glds16(g, dst); };
  auto issue = [&](int kt) {
    const int k0 = kt * BK;
    bf16* slot = ring + (kt % ST) * ring_slot_elems<MI>;
#pragma unroll
    for (int j = 0; j < PA; j++) dma(a_src(j, k0), slot + (w * 8 * PA + j * 8) * BK);
#pragma unroll
    for (int j = 0; j < PB; j++) dma(b_src(j, k0), slot + B0 + (w * 8 * PB + j * 8) * BK);
  };

  for (int kt = 0; kt < min(ST - 1, nk); kt++) issue(kt);
  __builtin_amdgcn_sched_barrier(0);                          // the accumulators are cleared under the flight of these DMAs, not ahead of them (16 MI x 2 writes)
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  const int arow0 = (w >> 1) * 32 * MI + (l & 31), brow0 = (w & 1) * 64 + (l & 31);
  // fragment addresses (bytes folded by the compiler): row r, k-step ks -> chunk (2 ks + hi) ^ ((r >> 1) & 7)
  auto ldfrag = [&](const bf16* base, int r, int ks) { return *(const bf16x8*)(base + r * BK + (((ks * 2 + hi) ^ ((r >> 1) & 7)) << 3)); };
  for (int kt = 0; kt < nk; kt++) {
    ring_wait<PA + PB, ST - 2>(min(ST - 2, nk - 1 - kt));     // K-tiles after kt that may still be in flight
    __builtin_amdgcn_s_barrier();
    if (kt + ST - 1 < nk) issue(kt + ST - 1);                 // its DMA overlaps the MFMAs of tile kt
    const bf16* as = ring + (kt % ST) * ring_slot_elems<MI>;
    const bf16* bs = as + B0;
    if constexpr (MI == 2) {
      bf16x8 af[2][2], bfr[2][2];                             // register double-buffered fragments: reads of k-step ks + 1 fly under the MFMAs of ks
#pragma unroll
      for (int i = 0; i < 2; i++) { af[0][i] = ldfrag(as, arow0 + i * 32, 0); bfr[0][i] = ldfrag(bs, brow0 + i * 32, 0); }
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const int c = ks & 1;
        if (ks + 1 < 4) {
#pragma unroll
          for (int i = 0; i < 2; i++) { af[c ^ 1][i] = ldfrag(as, arow0 + i * 32, ks + 1); bfr[c ^ 1][i] = ldfrag(bs, brow0 + i * 32, ks + 1); }
        }
        __builtin_amdgcn_sched_barrier(0);                    // keep the prefetch ahead of this k-step's MFMAs (distinct registers)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[c][j], af[c][i], acc[i][j], 0, 0, 0);
      }
    } else {                                                  // 64-row tile: plain reads
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const bf16x8 af = ldfrag(as, arow0, ks);
#pragma unroll
        for (int j = 0; j < 2; j++)
          acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ldfrag(bs, brow0 + j * 32, ks), af, acc[0][j], 0, 0, 0);
      }
    }
  }
}     // (a caller that reuses the ring, as the GemmNT epilogues do, puts a barrier first: other waves may still be reading the last tile)
