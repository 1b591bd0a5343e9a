// The staged block: a wave's 32 x 64 output block on its way from accumulator shape to 16-byte row-major stores (gemm.hip's staged epilogues,
// attention.hip's wave_block_store).
//
// Why stage at all.  In accumulator shape a lane owns one row and runs of 4 columns, so a direct bf16x4 store puts 64 different rows (64 cache
// lines) behind every store instruction; s_memtime stamps of the 256x256 kernel show that issuing them takes ~10k cycles per tile - as long as
// 3.3 K-tiles of MFMA work - because the address coalescer walks the lines one by one.  Staging the block through a wave-private 4 KiB LDS area
// (128-byte rows, chunk index XOR ((row >> 1) & 7): conflict-free for both the 8-byte writes and the 16-byte reads) turns them into 16-byte stores
// with 8 lanes per 128-byte row segment: 8 lines per instruction.  No block barrier: the area is wave-private and one wave's LDS operations
// execute in order.
//
// Shapes.  Fragment shape (what stage_put4 writes): lane l holds row l & 31, columns j * 32 + 8 g + 4 (l >> 5) .. + 3 of accumulator j, group g.
// Flush shape (what stage_read4 returns): pass q of 4 covers row q * 8 + (l >> 3), 16-byte chunk l & 7.  The layout functions below are the only
// place where a (row, column) becomes an LDS offset; the static_asserts check on every build that a write site and a read site cannot disagree.
#pragma once
#include "tfx_common.h"

// ---- layout: element offset of (row, col) in each image ------------------------------------------------------------------------------------------
constexpr int stage_chunk(int row, int ch) { return row * 64 + ((ch ^ ((row >> 1) & 7)) << 3); }                          // [32][64] bf16, 4 KiB: 16-byte chunk ch of a row
constexpr int stage_off(int row, int col) { return stage_chunk(row, col >> 3) + (col & 7); }
constexpr int stage_off32(int row, int col) { return row * 32 + (((col >> 3) ^ ((row >> 2) & 3)) << 3) + (col & 7); }     // [32][32] bf16: the GEGLU product h = a * gelu(g)
constexpr int stage_off_f32(int row, int col) { return row * 68 + col; }                                                  // [32][68] fp32 (272-byte rows; 64 columns used)
constexpr int stage_off_ag(int row, int col) { return row * 128 + (((col >> 3) ^ (row & 15)) << 3) + (col & 7); }         // [32][128] bf16: the saved [a|g] of the GEGLU backward
constexpr int STAGE_ELEMS = 32 * 64, STAGE32_ELEMS = 32 * 32, STAGE_F32_ELEMS = 32 * 68, STAGE_AG_ELEMS = 32 * 128;

// `off` maps the 32 x cols block one-to-one into [0, size), and every aligned run of `run` columns of a row onto `run` consecutive elements that start
// on a multiple of `run` (run = 4: what stage_put4 writes, 8 bytes; run = 8: a read-back chunk, 16 bytes; fp32: run = 4 is 16 bytes)
constexpr bool stage_layout_ok(int (*off)(int, int), int cols, int size, int run, bool onto) {
  bool seen[STAGE_AG_ELEMS] = {};
  for (int row = 0; row < 32; row++)
    for (int col = 0; col < cols; col++) {
      const int o = off(row, col);
      if (o < 0 || o >= size || seen[o]) return false;
      seen[o] = true;
      if (col % run == 0 ? o % run != 0 : o != off(row, col - 1) + 1) return false;
    }
  return !onto || 32 * cols == size;
}
static_assert(stage_layout_ok(stage_off, 64, STAGE_ELEMS, 4, true) && stage_layout_ok(stage_off, 64, STAGE_ELEMS, 8, true), "32 x 64 bf16 image");
static_assert(stage_layout_ok(stage_off32, 32, STAGE32_ELEMS, 4, true) && stage_layout_ok(stage_off32, 32, STAGE32_ELEMS, 8, true), "32 x 32 bf16 image");
static_assert(stage_layout_ok(stage_off_ag, 128, STAGE_AG_ELEMS, 4, true) && stage_layout_ok(stage_off_ag, 128, STAGE_AG_ELEMS, 8, true), "[32][128] [a|g] image");
static_assert(stage_layout_ok(stage_off_f32, 64, STAGE_F32_ELEMS, 4, false), "[32][68] fp32 image");

// ---- write side ------------------------------------------------------------------------------------------------------------------------------
TFX_DEV void stage_put4(bf16* st, int row, int col, f32x4 v) {
  bf16x4 o; o[0] = f2bf(v[0]); o[1] = f2bf(v[1]); o[2] = f2bf(v[2]); o[3] = f2bf(v[3]);
  *(bf16x4*)(st + stage_off(row, col)) = o;
}
TFX_DEV void stage_put4_32(bf16* st, int row, int col, f32x4 v) {
  bf16x4 o; o[0] = f2bf(v[0]); o[1] = f2bf(v[1]); o[2] = f2bf(v[2]); o[3] = f2bf(v[3]);
  *(bf16x4*)(st + stage_off32(row, col)) = o;
}
// the raw accumulator pair of one 32-row block, in fragment shape (r = l & 31, hi = l >> 5)
TFX_DEV void stage_put_acc(bf16* st, int r, int hi, const f32x16 (&a)[2]) {
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      f32x4 a4;
#pragma unroll
      for (int e = 0; e < 4; e++) a4[e] = a[j][4 * g + e];
      stage_put4(st, r, j * 32 + 8 * g + 4 * hi, a4);
    }
}

// ---- read-back and flush ----------------------------------------------------------------------------------------------------------------------
// the block in flush shape (ch = l & 7, handed in: the callers hold it).  All four LDS reads ahead of the (branch-guarded) stores: one LDS latency
// per block, not four.  CLAMP: rows past `last` read row `last` (attention's ragged blocks compute on them)
template <bool CLAMP = false>
TFX_DEV void stage_read4(const bf16* st, int l, int ch, bf16x8 (&v)[4], int last = 31) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int row = CLAMP ? min(q * 8 + (l >> 3), last) : q * 8 + (l >> 3);
    v[q] = *(const bf16x8*)(st + stage_chunk(row, ch));
  }
}
// pass q goes to row rows[q] (< 0: skip) of the matrix with leading dimension ld; blk = the block's first column in row 0 of that matrix, this lane
// stores chunk ch of it.  GUARD = false: no predicate at all around the stores.  (staged_epilogue_bf16 spells this loop out: see there.)
template <bool GUARD = true>
TFX_DEV void stage_store4(const bf16x8 (&v)[4], bool col_ok, bf16* blk, int ld, int ch, const int (&rows)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (!GUARD || (col_ok && rows[q] >= 0)) *(bf16x8*)(blk + (size_t)rows[q] * ld + ch * 8) = v[q];
}

// ---- side data in the two shapes ----------------------------------------------------------------------------------------------------------------
// Output rows of the flush passes: mo[i][q] = destination row of tile row m_w + i * 32 + q * (32 / PASSES) + (l >> SH), < 0 = past M (skip).
// PASSES = 4: bf16 blocks (8 lanes per row), 8: fp32 (16 lanes), 2: the 32-wide h block (4 lanes).
enum { ROWS_IDENT, ROWS_MAP_OR_IDENT, ROWS_MAP };                // no map read at all / map[m], null = identity (rowmap) / map[m], never null (qk_cache_pos)
template <int MODE, int NI, int PASSES>
TFX_DEV void stage_rows(int (&mo)[NI][PASSES], int m_w, int M, int l, const int32_t* map = nullptr) {
  constexpr int SH = PASSES == 2 ? 2 : PASSES == 4 ? 3 : 4;      // log2 of the lanes per row
  static_assert(2 * PASSES == 1 << SH, "PASSES is 2, 4 or 8");
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int q = 0; q < PASSES; q++) {
      const int m = m_w + i * 32 + q * (32 / PASSES) + (l >> SH);
      if constexpr (MODE == ROWS_IDENT) mo[i][q] = m < M ? m : -1;
      else if constexpr (MODE == ROWS_MAP_OR_IDENT) mo[i][q] = m < M ? (map ? map[m] : m) : -1;
      else mo[i][q] = m < M ? map[m] : -1;
    }
}
// The bias of this lane's fragment columns: b[j][g] = bias[n_w + j * 32 + 8 g + 4 hi .. + 3] (clamped into [0, N)), zeros without a bias.
// ONE branch around all eight loads: with a branch per load hipcc waits (`s_waitcnt vmcnt(0)`) at every join - eight serial round trips to L2.
// A constant nullptr issues no load at all.
TFX_DEV void stage_bias(f32x4 (&b)[2][4], const float* bias, int n_w, int hi, int N) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int g = 0; g < 4; g++) b[j][g] = zero4;
  if (bias) {
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int g = 0; g < 4; g++) b[j][g] = *(const f32x4*)(bias + min(n_w + j * 32 + 8 * g + 4 * hi, N - 4));
  }
}
