// t128_loop.h — the two K loops of the 128 x 128 x 64 kernels, written once.  The register-staged loop is run by gemm_kernel (gemm_kernels.h) and by
// conv_igemm_kernel and conv_wgrad_igemm_kernel (conv_igemm.hip); the "pipe2" loop by gemm_pipe2_kernel (gemm_kernels.h) and conv_igemm_glds_kernel
// (conv_igemm.hip).
//
// "t128": a 128 x 128 x 64 workgroup tile, 4 waves (2 x 2) of 64 x 64, each 4 x 4 v_mfma_f32_16x16x32 per k32 half-step, two LDS stages of
// [A tile | B tile] (32 KiB each), two workgroups per CU.  It serves every shape the 256-wide tiles (w256_loop.h) do not take.
//
// Form: hook macros, as in w256_loop.h and for the same reason (a __forceinline__ function template with a lambda for the gather gave
// conv_igemm_kernel another scalar register allocation and conv_wgrad_igemm_kernel one instruction more; the macros leave every kernel's instruction
// stream as it was, tools/isa_lint.py --diff).  A kernel defines the hooks of the loop it runs, expands the loop and #undefs the hooks behind it.
//
// In scope at the point of expansion of either loop: OT, smem (the two stages), wm, wn, lg, l16, f32x4 acc[4][4] (the loop clears it).
#pragma once
#include "gemm_tiles.h"

#define T128_STAGE_BYTES (2 * G_TILE_BYTES)
#define T128_CLEAR()                                                                                                              \
  do {                                                                                                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                                              \
      _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) acc[i_][j_] = (f32x4){0.f, 0.f, 0.f, 0.f};                                 \
  } while (0)
// the wave's 4 + 4 fragments of k32 half-step KS of the stage at STAGE (TA / TB: contraction-major image, transpose reads)
#define T128_READ(FA, FB, TA, TB, STAGE, KS)                                                                                      \
  do {                                                                                                                            \
    const unsigned char* sa_ = (STAGE);                                                                                           \
    const unsigned char* sb_ = sa_ + G_TILE_BYTES;                                                                                \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) FA[i_] = tile_frag<TA>(sa_, wm * 64 + i_ * 16, KS, lg, l16);                 \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) FB[j_] = tile_frag<TB>(sb_, wn * 64 + j_ * 16, KS, lg, l16);                 \
  } while (0)
// the 16 MFMAs of a half-step (operands swapped: a lane ends up with 4 consecutive output columns of one row)
#define T128_MMA(FA, FB)                                                                                                          \
  do {                                                                                                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                                              \
      _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) acc[i_][j_] = mfma16<OT>(FB[j_], FA[i_], acc[i_][j_]);                     \
  } while (0)

// =================================================================================================
// Register-staged loop over NK >= 0 K steps: load step kt+1 into registers, 2 x 16 MFMAs on the LDS stage of step kt, store the registers into
// the other stage, __syncthreads().  For operands that need per-lane predication or zero-fill (partial K tiles, gathered pixels), which
// global_load_lds cannot do.  Also in scope: t, u32x4 ra[4], rb[4] (one register set: a second one, loading two K steps ahead, was measured
// slower in conv_igemm_kernel, 285-383 vs 405 TF/s — the allocator then fills all 256 registers and spills).  Hook:
//   T128_GATHER(KT)   fills ra (A tile) and rb (B tile) for K step KT of this workgroup, zeros where the operand does not exist
// =================================================================================================
#define T128_REG_MAINLOOP(TA, TB, NK)                                                                                             \
  do {                                                                                                                            \
    T128_CLEAR();                                                                                                                 \
    if ((NK) > 0) {                                                                                                               \
      T128_GATHER(0);                                                                                                             \
      tile_sstore<TA>(ra, smem, t);                                                                                               \
      tile_sstore<TB>(rb, smem + G_TILE_BYTES, t);                                                                                \
    }                                                                                                                             \
    __syncthreads();                                                                                                              \
    for (int kt = 0; kt < (NK); ++kt) {                                                                                           \
      const int stage = kt & 1;                                                                                                   \
      if (kt + 1 < (NK)) { T128_GATHER(kt + 1); }                                                                                 \
      const unsigned char* sa = smem + stage * T128_STAGE_BYTES;                                                                  \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                                          \
        s16x8 fa[4], fb[4];                                                                                                       \
        T128_READ(fa, fb, TA, TB, sa, ks);                                                                                        \
        T128_MMA(fa, fb);                                                                                                         \
      }                                                                                                                           \
      if (kt + 1 < (NK)) {                                                                                                        \
        unsigned char* na = smem + (stage ^ 1) * T128_STAGE_BYTES;                                                                \
        tile_sstore<TA>(ra, na, t);                                                                                               \
        tile_sstore<TB>(rb, na + G_TILE_BYTES, t);                                                                                \
      }                                                                                                                           \
      __syncthreads();                                                                                                            \
    }                                                                                                                             \
  } while (0)

// =================================================================================================
// "pipe2" loop over NK >= 0 K steps: direct-to-LDS loads (global_load_lds: no staging registers, no ds_write pass; every K slice a multiple
// of 64), software-pipelined around ONE mid-iteration barrier:
//     read F1 = fragments (kt, k 32..63)            | LDS latency of F1 hides under ...
//     16 MFMAs on F0 = fragments (kt, k 0..31)      | ... these MFMAs
//     lgkmcnt(0) ; vmcnt(0) ; s_barrier             <- every wave now holds ALL of stage kt in registers, and its
//                                                      share of stage kt+1 (issued one full iteration ago) has landed
//     global_load_lds stage kt+2 -> the buffer of stage kt   (free: nobody reads it any more)
//     read F0 = fragments (kt+1, k 0..31)           | latency hides under ...
//     16 MFMAs on F1                                | ... these MFMAs
// so loads get a whole iteration to arrive with only two 32-KiB buffers (two workgroups per CU), and no ds_read latency is exposed in
// steady state.  Raw s_barrier + explicit waits: __syncthreads() would drain differently.
//   * The 8 loads of stage kt+2 are spread one per two MFMAs of the second half instead of issued as a burst: a burst is back-pressured by
//     the texture addresser (~64 B/clk/CU) and the in-order wave cannot issue MFMAs meanwhile.
//   * The waits inside the loop are __builtin_amdgcn_s_waitcnt, not inline assembly: the compiler's wait-count pass sees a builtin and adds no
//     conservative wait of its own at the loop top; the lgkmcnt(0) behind the prologue's read gives both edges into the loop header the same
//     state.
// Also in scope: s16x8 fa0[4], fb0[4], fa1[4], fb1[4].  A wave stages 8 one-KiB slabs per stage: slabs wave*4 + 0..3 of the A and of the B tile.
// Hooks:
//   T128_P2_STAGE(S)            prologue: all 8 requests of K step S (0 or 1) into stage S, whatever pointer work they need included
//   T128_P2_POINTERS(KT, EXISTS) between the barrier and the second half: pointer work the requests of step KT = kt+2 need, done only if EXISTS
//                               (an expression the hook evaluates itself; the hook may be empty, and `more` is then first computed behind the fence)
//   T128_P2_REQUEST(STAGE, I, JJ) the ONE request of step kt+2 that goes under MFMA pair (I, JJ), I = 0..3, JJ = 0..1, into the stage at STAGE
// =================================================================================================
// slab I (0..3) of this wave in tile WHICH (0 = A, 1 = B) of the stage at STAGE
#define T128_P2_LOAD(PTR, STAGE, WHICH, I)                                                                                         \
  __builtin_amdgcn_global_load_lds((const GLB_AS void*)(PTR),                                                                     \
                                   (LDS_AS void*)((STAGE) + (WHICH) * G_TILE_BYTES + (wave * 4 + (I)) * 1024), 16, 0, ENH_GLDS_AUX)
#define T128_P2_MAINLOOP(TA, TB, NK)                                                                                              \
  do {                                                                                                                            \
    T128_CLEAR();                                                                                                                 \
    if ((NK) > 0) {                                                                                                               \
      T128_P2_STAGE(0);                                                                                                           \
      if ((NK) > 1) {                                                                                                             \
        T128_P2_STAGE(1);                                                                                                         \
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); /* stage 0 landed (stage 1's 8 loads may be outstanding) */              \
      } else {                                                                                                                    \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                          \
      }                                                                                                                           \
      __builtin_amdgcn_s_barrier();                                                                                               \
      T128_READ(fa0, fb0, TA, TB, smem, 0);                                                                                       \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0): same state on both edges into the loop header */                         \
    }                                                                                                                             \
    int buf = 0;                                                                                                                  \
    for (int kt = 0; kt < (NK); ++kt) {                                                                                           \
      T128_READ(fa1, fb1, TA, TB, smem + buf * T128_STAGE_BYTES, 1);                                                              \
      __builtin_amdgcn_sched_barrier(0);                                                                                          \
      T128_MMA(fa0, fb0);                                                                                                         \
      __builtin_amdgcn_sched_barrier(0);                                                                                          \
      __builtin_amdgcn_s_waitcnt(0x0070); /* vmcnt(0) lgkmcnt(0): F1 in registers, my share of stage kt+1 landed */               \
      __builtin_amdgcn_s_barrier();                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                                          \
      if (kt + 1 < (NK)) T128_READ(fa0, fb0, TA, TB, smem + (buf ^ 1) * T128_STAGE_BYTES, 0);                                     \
      T128_P2_POINTERS(kt + 2, kt + 2 < (NK));                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                          \
      const bool more = kt + 2 < (NK);                                                                                            \
      unsigned char* const vacated = smem + buf * T128_STAGE_BYTES;                                                               \
      /* second half: the 8 loads of stage kt+2 (into the buffer stage kt just vacated) one per two MFMAs */                      \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                             \
        _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) {                                                                        \
          acc[i][jj * 2] = mfma16<OT>(fb1[jj * 2], fa1[i], acc[i][jj * 2]);                                                       \
          acc[i][jj * 2 + 1] = mfma16<OT>(fb1[jj * 2 + 1], fa1[i], acc[i][jj * 2 + 1]);                                           \
          if (more) { T128_P2_REQUEST(vacated, i, jj); }                                                                          \
          __builtin_amdgcn_sched_barrier(0);                                                                                      \
        }                                                                                                                         \
      }                                                                                                                           \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0) only: the next F0 has arrived under the MFMAs above */                    \
      buf ^= 1;                                                                                                                   \
    }                                                                                                                             \
  } while (0)
