// attention_common.h — helpers shared by the attention kernels (attention.hip / attention_kernels.h; x3.hip / x3_attention.h):
// the swizzled LDS image of a [64][64] bf16 tile, register staging, MFMA operand fragments (row and transpose-read) and the workgroup -> (block, head) map.
#pragma once
#include <type_traits>
#include "common.h"

#define ATT_D 64
#define ATT_TILE_BYTES 8192  // 64 rows x 64 bf16

// LDS image of a [64 rows][64 d] bf16 tile: 16-B chunk c (0..7) of row r at r*128 + ((c ^ f(r)) << 4) with
// f(r) = ((r>>1)&1)<<2 | (r>>2)&3 : conflict-free for ds_write_b128 (staging), the 32-row ds_read_b128
// fragments and the 4-row x 64-B transpose reads (gfx950 bank model; tools/lds_bank_check.py).
__device__ __forceinline__ int att_off(int r, int c) { return r * 128 + ((c ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3))) << 4); }

// rows row0 .. row0+63 of a [*][rs] bf16 matrix, 2 x 16 B per thread.  The address is split into a WAVE-UNIFORM part (base + row0 * rs: scalar registers,
// advanced by the scalar unit) and a 32-bit per-lane byte offset that does not depend on the tile (hoisted out of the loop): the loads then use the
// scalar-base + vector-offset form and cost no vector instructions per tile (the 64-bit per-lane address arithmetic was 13 of dK/dV's ~170 vector
// instructions per tile, and the kernels' time follows that count: profiles/r03_attention_lab.txt).
__device__ __forceinline__ void att_gload(u32x4 (&r)[2], const uint16_t* __restrict__ base, int64_t rs, int row0, int t) {
  const int c = t & 7, r0 = t >> 3;
  const unsigned char* ub = reinterpret_cast<const unsigned char*>(base + (int64_t)row0 * rs);
  const unsigned lane_off = (unsigned)(r0 * (int)rs + c * 8) * 2u;
#pragma unroll
  for (int i = 0; i < 2; ++i) r[i] = *reinterpret_cast<const u32x4*>(ub + (size_t)(unsigned)(i * 32 * (int)rs * 2) + lane_off);
}
__device__ __forceinline__ void att_sstore(const u32x4 (&r)[2], unsigned char* tile, int t) {
  const int c = t & 7, r0 = t >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(tile + att_off(r0 + 32 * i, c)) = r[i];
}
// The same tile image written by LDS-DMA (global_load_lds, 16 B per lane): no staging registers, no ds_write pass.  The LDS destination of a wave
// instruction is lane-linear (base + lane * 16 B: 8 rows x 128 B), so the swizzle is applied to the lane's SOURCE address: slot p = lane & 7 of row r must
// receive chunk c = p ^ f(r).  Wave w of the four stages rows 16 w .. 16 w + 15 (two instructions per operand and tile).  The caller waits vmcnt(0) before the
// barrier that publishes the tile.
__device__ __forceinline__ unsigned att_dma_lane_off(int rs_elems, int lane, int i) {   // byte offset of this lane's 16 source bytes inside 8-row group i (0 | 1) of a wave's 16 rows
  const int rr = lane >> 3, p = lane & 7, r = rr + 8 * i;      // f(r) of att_off depends on r & 15 only (bits 1..3), and the wave's row base is a multiple of 16
  const int c = p ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3));
  return (unsigned)(rr * rs_elems + c * 8) * 2u;
}
__device__ __forceinline__ void att_dma_tile(const uint16_t* __restrict__ base, int64_t rs, int row0, unsigned char* tile, int wave, unsigned lane_off0, unsigned lane_off1) {
  const unsigned char* ub = reinterpret_cast<const unsigned char*>(base + (int64_t)(row0 + wave * 16) * rs);
  // the lane offsets are made opaque HERE: their widening to 64 bits then happens next to the request, which lets instruction selection take the
  // scalar-base + 32-bit-vector-offset form of the instruction.  Hoisted out of the tile loop (what the optimizer does with a loop-invariant
  // widening) every offset occupies a register PAIR for the whole kernel and every request costs a 64-bit vector add into a third pair.
  asm volatile("" : "+v"(lane_off0));
  asm volatile("" : "+v"(lane_off1));
  __builtin_amdgcn_global_load_lds((const GLB_AS void*)(ub + lane_off0), (LDS_AS void*)(tile + (wave * 16) * 128), 16, 0, 0);
  __builtin_amdgcn_global_load_lds((const GLB_AS void*)(ub + (size_t)(unsigned)(8 * (int)rs * 2) + lane_off1), (LDS_AS void*)(tile + (wave * 16 + 8) * 128), 16, 0, 0);
}
// ---- the ragged last tile of an image (token counts that are no multiple of 64: the *_tail_* kernels) ------------------------------------------------
// Rows row0 .. n_rows - 1 of the tile exist.  Every source row is clamped to the image's last row: nothing outside the tensor (or inside the next
// image) is read, and the rows of the LDS image past the end hold finite values (their probabilities are exactly 0, and 0 x NaN would be NaN).
// The lane offsets of att_dma_tile are tile-invariant; this tile computes its own (once per workgroup pass, outside the counted reads).
__device__ __forceinline__ void att_gload_clamped(u32x4 (&r)[2], const uint16_t* __restrict__ base, int64_t rs, int row0, int n_rows, int t) {
  const int c = t & 7, r0 = t >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) r[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)min(row0 + r0 + 32 * i, n_rows - 1) * rs + c * 8);
}
__device__ __forceinline__ void att_dma_tile_clamped(const uint16_t* __restrict__ base, int64_t rs, int row0, int n_rows, unsigned char* tile, int wave, int lane) {
  // (opaque: this tile's address arithmetic stays where the tile is requested.  It is invariant in the tile loop, and hoisted out of it it holds
  // registers for the whole kernel — the forward went from 126 to 194 that way)
  asm volatile("" : "+s"(n_rows));
  const int wrow = min(row0 + wave * 16, n_rows - 1);      // wave-uniform: the scalar base stays inside the image, the lane offsets stay non-negative
  const int lim = n_rows - 1 - wrow;
  const unsigned char* ub = reinterpret_cast<const unsigned char*>(base + (int64_t)wrow * rs);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rr = lane >> 3, p = lane & 7, r = rr + 8 * i;
    const int c = p ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3));      // the swizzle follows the DESTINATION row (att_dma_lane_off)
    unsigned off = (unsigned)(min(r, lim) * (int)rs + c * 8) * 2u;
    asm volatile("" : "+v"(off));      // (scalar base + 32-bit vector offset, as att_dma_tile)
    __builtin_amdgcn_global_load_lds((const GLB_AS void*)(ub + off), (LDS_AS void*)(tile + (wave * 16 + 8 * i) * 128), 16, 0, 0);
  }
}
// what a key row past the end adds to its log2-domain score (through the MFMA C operand): large, negative and FINITE (the attention objects are built
// with -fno-honor-nans; no infinity is relied on).  exp2 of it is exactly 0, and it never reaches the row maximum: every tile holds a valid key.
#define ATT_MASK_BIAS (-1.0e30f)
// accumulator register r of key block kb of a 64-key tile is key kb*32 + 8*(r>>2) + 4*hi + (r&3)
__device__ __forceinline__ float att_key_bias(int kb, int r, int hi, int n_keys) { return kb * 32 + 8 * (r >> 2) + 4 * hi + (r & 3) < n_keys ? 0.f : ATT_MASK_BIAS; }

// 32x32x16 operand fragment, rows = tile rows rb + (lane&31), k = d: ds*16 + hi*8 + 0..7
__device__ __forceinline__ s16x8 att_frag_row(const unsigned char* tile, int rb, int ds, int l31, int hi) {
  return *reinterpret_cast<const s16x8*>(tile + att_off(rb + l31, ds * 2 + hi));
}
// 32x32x16 operand fragment contracted over TILE ROWS: index = column cb*32 + (lane&31); k-slot (hi, j) is tile
// row rbase + 8*(j>>2) + 4*hi + (j&3)  — exactly the rows a lane holds in accumulator registers 8*c2 + j of a
// 32x32 C tile whose row block starts at rbase - 16*c2 (so P / dS go from registers to the next MFMA unmoved).
__device__ __forceinline__ s16x8 att_frag_tr(const unsigned char* tile, int rbase, int cb, int lane) {
  const int G = lane >> 4, s = lane & 15;
  const int row = rbase + 4 * (G >> 1) + (s >> 2);
  const int cch = cb * 4 + (G & 1) * 2 + ((s & 3) >> 1);
  const int sub = (s & 1) * 8;
  const s16x4 lo = lds_tr_read_b64(tile + att_off(row, cch) + sub);
  const s16x4 hi = lds_tr_read_b64(tile + att_off(row + 8, cch) + sub);
  s16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
  o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
// ---- fragment reads the kernel counts itself (the LDS-DMA kernels of attention.hip) ---------------------------------------------------------------
// The compiler's wait-count pass cannot separate a read of the tile ring from the global_load_lds that fills the ring's OTHER stage, and puts
// s_waitcnt vmcnt(0) in front of the first such read of a tile: the prefetch is drained where it was meant to run under the tile's MFMAs (common.h,
// lds_tr_read_b64_asm).  These reads are inline asm, which that pass does not see; the kernel owns their ordering:
//   * a stage is read only behind the vmcnt(0) AND the barrier that close the tile before it, and every read of a tile is taken (waited for) by the
//     MFMA that consumes it, i.e. before the barrier that lets the next request overwrite the stage;
//   * att_take_* is the wait: s_waitcnt lgkmcnt(PEND) with the fragment's registers as read-write operands, so the consuming MFMA depends on the
//     wait through its operand and cannot be scheduled above it (cdna_hip_programming.md §5.7 item 1, form ii), while the vector arithmetic
//     between the MFMAs stays free to move.  LDS operations complete in order: PEND = the LDS operations the kernel itself issued behind the
//     fragment's own.  Operations the compiler adds in between (the statistics of dK/dV) only make the wait stricter; no scalar load runs in the loops.
// tools/isa_lint.py attention_pipeline() checks on the shipped library that no instruction touches a fragment's registers between request and wait.
typedef unsigned long long att_u64;
__device__ __forceinline__ unsigned att_lds_addr(const void* p) { return (unsigned)(uintptr_t)(LDS_AS const void*)p; }
// per-lane byte offsets of the two fragment kinds inside a tile image (the tile-row block and the operand are added as immediates, the stage by att_ring_advance):
// row fragment ds (att_frag_row with rb = 0) and the two halves of transpose fragment cb (att_frag_tr with rbase = 0)
__device__ __forceinline__ unsigned att_row_lane_off(int ds, int l31, int hi) { return (unsigned)att_off(l31, ds * 2 + hi); }
__device__ __forceinline__ unsigned att_tr_lane_off(int cb, int lane, int half) {
  const int G = lane >> 4, s = lane & 15;
  return (unsigned)(att_off(4 * (G >> 1) + (s >> 2) + 8 * half, cb * 4 + (G & 1) * 2 + ((s & 3) >> 1)) + (s & 1) * 8);
}
// a lane's eight fragment addresses (row fragments ds = 0..3, transpose fragments cb = 0 | 1 x lower | upper half) in stage 0 of a ring of two-tile
// stages ([stage][operand][ATT_TILE_BYTES]), and their move to the other stage behind a tile read from stage st
__device__ __forceinline__ void att_ring_addresses(unsigned (&ra)[4], unsigned (&ta)[2][2], const void* ring, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) ra[i] = att_lds_addr(ring) + att_row_lane_off(i, lane & 31, lane >> 5);
#pragma unroll
  for (int i = 0; i < 4; ++i) ta[i >> 1][i & 1] = att_lds_addr(ring) + att_tr_lane_off(i >> 1, lane, i & 1);
}
__device__ __forceinline__ void att_ring_advance(unsigned (&ra)[4], unsigned (&ta)[2][2], int st) {
  const unsigned adv = st ? 0u - 2u * ATT_TILE_BYTES : 2u * ATT_TILE_BYTES;
#pragma unroll
  for (int i = 0; i < 4; ++i) { ra[i] += adv; ta[i >> 1][i & 1] += adv; }
}
template <int OFF>
__device__ __forceinline__ void att_req_row(u32x4& f, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(addr), "i"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void att_req_tr(att_u64& lo, att_u64& hi, unsigned addr_lo, unsigned addr_hi) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(addr_lo), "i"(OFF) : "memory");
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(addr_hi), "i"(OFF) : "memory");
}
template <int PEND>
__device__ __forceinline__ s16x8 att_take_row(u32x4& f) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "i"(PEND) : "memory");
  return __builtin_bit_cast(s16x8, f);
}
template <int PEND>
__device__ __forceinline__ s16x8 att_take_tr(att_u64& lo, att_u64& hi) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(lo), "+v"(hi) : "i"(PEND) : "memory");
  typedef __attribute__((ext_vector_type(2))) att_u64 u64x2;
  const u64x2 o = {lo, hi};
  return __builtin_bit_cast(s16x8, o);
}
// f(integral_constant<int, B>) .. f(integral_constant<int, E - 1>): a loop whose index is a constant expression (immediate offsets, wait counts)
template <int B, int E, typename F>
__device__ __forceinline__ void att_static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    att_static_for<B + 1, E>(f);
  }
}

template <typename OT>
__device__ __forceinline__ s16x8 pack8(const float* p) {
  u32x4 u = {pack2<OT>(p[0], p[1]), pack2<OT>(p[2], p[3]), pack2<OT>(p[4], p[5]), pack2<OT>(p[6], p[7])};
  return __builtin_bit_cast(s16x8, u);
}
// Every global load of a kernel's prologue (Q / dO / K / V fragments, statistics) is waited for HERE, before the tile loop: the compiler's wait-count
// pass merges the loop-entry state into the loop body, so a fragment load still pending at entry made it wait, in EVERY iteration, for the oldest of
// the tile prefetch loads issued a few instructions earlier (s_waitcnt vmcnt(3) .. vmcnt(0) in front of the first MFMAs: the whole L2 latency exposed
// once per key tile — found in round 3 by reading the ISA).
#define ATT_LOOP_ENTRY() do { __builtin_amdgcn_s_waitcnt(0x0070); __builtin_amdgcn_sched_barrier(0); } while (0)
// pins a fragment loaded in the prologue: the value must be IN its registers at this point (IR-level sinking otherwise moves the load into the loop
// preheader, behind ATT_LOOP_ENTRY, and the pending-at-entry state is back)
__device__ __forceinline__ void att_pin(s16x8& f) {
  u32x4 u = __builtin_bit_cast(u32x4, f);
  asm volatile("" : "+v"(u));
  f = __builtin_bit_cast(s16x8, u);
}
// max(a, b, c) in ONE instruction (v_max3_f32).  Written as nested maxima the COMPILER sees: the attention objects are built with -fno-honor-nans, so no
// operand is canonicalised first (v_max_f32 x, x, x: seven instructions for a 4-way maximum, cdna_hip_programming.md "Fused attention" pitfalls) and the
// backend fuses the pair into v_max3_f32.  Round 4 used inline asm for this — and inline asm is invisible to the hazard recognizer: the first v_max3
// behind the S products read the MFMA's destination registers BEFORE the matrix pipe had written them (no s_nop in between), i.e. a stale maximum.  Any
// reference maximum gives a valid softmax, so every parity test passed; but the result bits changed from launch to launch (tools/attn_det_probe.py,
// found in round 5 by the graph-replay bit-identity test).  tests/test_isa_lint.py now refuses inline-asm VALU in the attention kernels' hot loops.
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
// combine a per-lane value with the other half-wave's (lane ^ 32) through one v_permlane32_swap (no LDS round trip).  Verified semantics
// (profiles/hw_probe_r01.txt P4): with both operands = v, every lane receives (v[lane & 31], v[(lane & 31) + 32]).
__device__ __forceinline__ float xhalf_max(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}

#define ATT_FENCE() __builtin_amdgcn_sched_barrier(0)
// (the kernels are templates over the operand type tag OT = BF16 | F16, common.h: `OT` must name it where this macro is used)
#define MFMA32(a, b, c) mfma32<OT>((a), (b), (c))

// Workgroup -> (block-within-head, head) mapping.  Hardware places workgroup L on XCD L % 8 (each XCD has a private L2), and the nblk
// workgroups of one (batch, head) all stream the SAME K/V (or Q/dO) — so they are given ids that are congruent mod 8 and adjacent in
// dispatch order: the head's 256 KiB of K/V is then fetched into ONE L2 and re-used there, instead of once per XCD (8x the fabric traffic).
__device__ __forceinline__ bool att_block_coords(int nblk, int n_heads_total, int& blk, int& head) {
  const int L = blockIdx.x;
  const int xcd = L & 7, r = L >> 3;
  head = (r / nblk) * 8 + xcd;
  blk = r % nblk;
  return head < n_heads_total;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
#define ATT_LOG2E 1.4426950408889634f
#define ATT_LN2 0.6931471805599453f
// the tail forms' launches (attention_tail.hip, x3_tail.hip), behind the argument checks of the C ABI functions that call them for N % 64 != 0
int enh_attention_tail_forward(const enh_h16* qkv, int B, int N, int H, float scale, int q_prescaled, enh_h16* out, float* lse, int dtype, void* stream);
int enh_attention_tail_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N, int H, float scale, int q_prescaled,
                                enh_h16* dqkv, float* delta_ws, int dtype, void* stream);
int enh_attention_tail_forward_x3(const enh_bf16* qkv_hi, const enh_bf16* qkv_lo, int B, int N, int H, float scale, enh_bf16* out3, enh_bf16* out_bf16, float* lse,
                                  void* stream);
