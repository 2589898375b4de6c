// w256_loop.h — the two-slot, one-wave-per-SIMD K loop of the 256-wide kernels, written once.  It is run by gemm_w256_body (gemm_kernels.h) and by
// conv_igemm_w256_kernel, conv_igemm_w512_kernel and conv_wgrad_w256_kernel (conv_igemm.hip); the persistent gemm_w256p_kernel runs its K-step inside
// a tile loop of its own, gemm_w256r_kernel uses its MFMA and fragment-read forms.  (The two K loops of the 128 x 128 x 64 kernels: t128_loop.h.)
//
// "w256": a 256 x 256 x 64 workgroup tile (512 x 128 in conv_igemm_w512_kernel), FOUR waves of 128 x 128 — one wave per SIMD, 256 accumulator
// registers (AGPRs) + ~170 VGPRs.  Round-2 design, measured step by step in tools/probe/gemm_lab.cpp (profiles/r02_gemm_lab.txt):
//   * one wave per SIMD reads each LDS byte once per 128 x 128 sub-tile: 32 fragment reads per 64 MFMAs (the removed 8-wave kernel's 128 x 64 waves
//     needed 48), and there is no second wave group to keep in phase — ONE barrier per K stage instead of eight;
//   * an in-order wave stalls the matrix pipe whenever an instruction takes longer to issue than the ~28 cycles of cover one MFMA gives, so
//     nothing is issued in bursts: fragment reads go one per MFMA under the first 8 MFMAs of every k16 step (all four waves hit the one LDS
//     at once: a burst of 32 reads costs ~128 cycles), global_load_lds one per two MFMAs (texture addresser ~64 B/clk per CU);
//     measured MFMA utilisation inside the K loop: 96 % without loads, 90 % with L2-resident operands, 70-80 % streaming from HBM;
//   * operands are staged as WHOLE 128-byte lines (64-deep K stages): fetching each line as two 64-byte halves one stage apart (a 4-slot
//     ring of 32-deep stages, which would allow a deeper prefetch) costs 7-11 % utilisation on HBM-streamed operands, while one stage less
//     of prefetch depth costs only 1-2 %;
//   * two LDS slots of one K stage each.  The barrier sits after the reads of the last k-step: the slot is then free and the loads of stage j+2
//     are spread over the next 32 MFMAs; every load gets 32-64 MFMAs (1-2 K-steps x 4) to land and the wait at the next barrier is vmcnt(0)
//     with nothing newer in flight — a count, not a drain.
//
// Form: hook macros.  A kernel defines the hooks below, expands W256_MAINLOOP (or W256_KSTEP) in its body and #undefs the hooks behind it.  A
// __forceinline__ function template taking the hooks as lambdas compiled conv_wgrad_w256_kernel<OT, false> to other code (3983 -> 4235
// instructions, 476 -> 492 VGPRs; the extra instructions are address and predicate code of the requests, BETWEEN the MFMAs of the loop), while
// the macro form left the instruction stream of every kernel of the library as it was when the four copies were merged (tools/isa_lint.py --diff).
//
// In scope at the point of expansion: OT, lane, f32x16 acc[4][W256_NJ] (W256_CLEAR clears it), s16x8 fa0[4], fb0[4], fa1[4], fb1[4].  Hooks:
//   W256_NJ                        column blocks of 32 per wave: 4 * NJ MFMAs and 4 + NJ fragment reads per k16 step
//   W256_LGKM0                     true if fragments come by the asm transpose reads, which the compiler's wait-count pass does not see: a k-step
//                                  then opens with lgkmcnt(0) (its fragments were read >= 8 MFMAs ago)
//   W256_READ(FA, FB, SLOT, S, U)  fragment U (0..3: A row-blocks into FA, 4..: B column-blocks into FB) of k16 step S of slot SLOT
//   W256_REQUEST(SLOT, HALF, Q)    the staging requests that go under MFMA Q of a k-step that carries half HALF (0 / 1) of a K stage into slot SLOT
//   W256_PROLOGUE()                requests of stage 0 -> slot 0, W256_ADVANCE(), first half of stage 1 -> slot 1, s_waitcnt vmcnt(stage 0 landed)
//   W256_ADVANCE()                 moves the staging state to the next K stage
#pragma once
#include "gemm_tiles.h"

#define W256_FENCE() __builtin_amdgcn_sched_barrier(0)
// MFMA Q of a k16 step, onto the accumulator / onto a zero C operand `zero16` (persistent kernels: the first k-step of a tile; nothing is cleared)
#define W256_MM(Q, FA, FB)                                                                                                        \
  acc[(Q) / (W256_NJ)][(Q) % (W256_NJ)] = mfma32<OT>(FB[(Q) % (W256_NJ)], FA[(Q) / (W256_NJ)], acc[(Q) / (W256_NJ)][(Q) % (W256_NJ)])
#define W256_MMZ(Q, FA, FB)                                                                                                       \
  acc[(Q) / (W256_NJ)][(Q) % (W256_NJ)] = mfma32<OT>(FB[(Q) % (W256_NJ)], FA[(Q) / (W256_NJ)], zero16)
// W256_READ for fragments that lie in the sub-tiles ATILE / BTILE of a slot (TRA / TRB: contraction-major image, transpose reads)
#define W256_READ_TILES(FA, FB, TRA, TRB, ATILE, BTILE, S, U)                                                                     \
  do {                                                                                                                            \
    if ((U) < 4) FA[(U) & 3] = frag32<TRA>(ATILE, ((U) & 3) * 32, S, lane);                                                       \
    else FB[(U) & 3] = frag32<TRB>(BTILE, ((U) & 3) * 32, S, lane);                                                               \
  } while (0)

// one k16 step: 4 * NJ MFMAs (MM: W256_MM or W256_MMZ) on (FA, FB), ONE per fence; under the first 4 + NJ one fragment read each (k-step RS of slot
// RSLOT into RA / RB); under MFMA q whatever W256_REQUEST puts there
#define W256_KSTEP_MM(MM, FA, FB, RA, RB, RSLOT, RS, DO_READ, GSLOT, HALF, DO_REQUEST)                                            \
  do {                                                                                                                            \
    if (W256_LGKM0) __builtin_amdgcn_s_waitcnt(0xC07F);                                                                           \
    W256_FENCE();                                                                                                                 \
    _Pragma("unroll") for (int q_ = 0; q_ < 4 * (W256_NJ); ++q_) {                                                                \
      MM(q_, FA, FB);                                                                                                             \
      if ((DO_READ) && q_ < 4 + (W256_NJ)) { W256_READ(RA, RB, RSLOT, RS, q_); }                                                  \
      if (DO_REQUEST) { W256_REQUEST(GSLOT, HALF, q_); }                                                                          \
      W256_FENCE();                                                                                                               \
    }                                                                                                                             \
  } while (0)
#define W256_KSTEP(FA, FB, RA, RB, RSLOT, RS, DO_READ, GSLOT, HALF, DO_REQUEST)                                                   \
  W256_KSTEP_MM(W256_MM, FA, FB, RA, RB, RSLOT, RS, DO_READ, GSLOT, HALF, DO_REQUEST)
// the first k16 step of a tile in the persistent kernel: C operand = 0 instead of cleared accumulators; reads k-step RS, requests nothing
#define W256_KSTEP_Z(FA, FB, RA, RB, RSLOT, RS) W256_KSTEP_MM(W256_MMZ, FA, FB, RA, RB, RSLOT, RS, true, 0, 0, false)

// the usual W256_REQUEST and W256_PROLOGUE: a wave stages 16 one-KiB pieces per K stage by ONE(SLOT, U), one under every odd MFMA
#define W256_REQUEST_ODD(ONE, SLOT, HALF, Q)                                                                                      \
  do {                                                                                                                            \
    if ((Q) & 1) { ONE(SLOT, (HALF) * 8 + ((Q) >> 1)); }                                                                          \
  } while (0)
#define W256_PROLOGUE_16(ONE)                                                                                                     \
  do {                                                                                                                            \
    _Pragma("unroll") for (int u = 0; u < 16; ++u) ONE(0, u);                                                                     \
    W256_ADVANCE();                                                                                                               \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) ONE(1, u);                                                                      \
    __builtin_amdgcn_s_waitcnt(0x0F78); /* vmcnt(8): stage 0 landed */                                                            \
  } while (0)

// the K loop of one tile over NST >= 2 stages
#define W256_MAINLOOP(NST)                                                                                                        \
  do {                                                                                                                            \
    /* prologue: stage 0 -> slot 0 completely; the first half of stage 1 -> slot 1 (the second half follows under the first k-step) */ \
    W256_PROLOGUE();                                                                                                              \
    __builtin_amdgcn_s_barrier();                                                                                                 \
    _Pragma("unroll") for (int u = 0; u < 4 + (W256_NJ); ++u) W256_READ(fa0, fb0, 0, 0, u);                                       \
    W256_FENCE();                                                                                                                 \
    /* invariant at the top of iteration j: the staging state is at stage j+1, whose first half is already requested into slot (j+1)&1 */ \
    int j = 0;                                                                                                                    \
    for (; j + 2 < (NST); ++j) {                                                                                                  \
      const int slot = j & 1;                                                                                                     \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot, 1, true, slot ^ 1, 1, true);   /* + second half of stage j+1 */                         \
      W256_ADVANCE();                                                                                                             \
      W256_KSTEP(fa1, fb1, fa0, fb0, slot, 2, true, 0, 0, false);                                                                 \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot, 3, true, 0, 0, false);                                                                 \
      __builtin_amdgcn_s_waitcnt(0x0070); /* vmcnt(0): stage j+1 landed (nothing newer outstanding) ; lgkmcnt(0): this slot is read out */ \
      __builtin_amdgcn_s_barrier();                                                                                               \
      W256_FENCE();                                                                                                               \
      W256_KSTEP(fa1, fb1, fa0, fb0, slot ^ 1, 0, true, slot, 0, true);   /* + first half of stage j+2 into the slot just vacated */ \
    }                                                                                                                             \
    { /* tail: stages NST-2 and NST-1 */                                                                                          \
      const int slot = j & 1;                                                                                                     \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot, 1, true, slot ^ 1, 1, true);   /* + second half of stage NST-1 */                       \
      W256_KSTEP(fa1, fb1, fa0, fb0, slot, 2, true, 0, 0, false);                                                                 \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot, 3, true, 0, 0, false);                                                                 \
      __builtin_amdgcn_s_waitcnt(0x0070);                                                                                         \
      __builtin_amdgcn_s_barrier();                                                                                               \
      W256_FENCE();                                                                                                               \
      W256_KSTEP(fa1, fb1, fa0, fb0, slot ^ 1, 0, true, 0, 0, false);                                                             \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot ^ 1, 1, true, 0, 0, false);                                                             \
      W256_KSTEP(fa1, fb1, fa0, fb0, slot ^ 1, 2, true, 0, 0, false);                                                             \
      W256_KSTEP(fa0, fb0, fa1, fb1, slot ^ 1, 3, true, 0, 0, false);                                                             \
      W256_KSTEP(fa1, fb1, fa0, fb0, 0, 0, false, 0, 0, false);                                                                   \
    }                                                                                                                             \
  } while (0)

// the accumulators of a wave, cleared (a macro like the rest: as a function template taking the array it moved conv_wgrad_w256_kernel's address code)
#define W256_CLEAR(ACC)                                                                                                           \
  do {                                                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                                 \
      _Pragma("unroll") for (int j = 0; j < (W256_NJ); ++j)                                                                       \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) ACC[i][j][r] = 0.f;                                                        \
  } while (0)
