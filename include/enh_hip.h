/*
 * enh_hip.h — C ABI of libenh_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the stage-1
 * ViT-VQGAN / RQ-VAE training path of thuanz123/enhancing-transformers.
 *
 * Boundary contract:
 *   - extern "C", plain pointers and sizes only; no torch / C++ types cross this boundary.
 *   - Every pointer is a DEVICE pointer owned by the caller (the Python host side allocates them as
 *     torch tensors and passes data_ptr()).  The library never allocates, frees or retains memory and
 *     never synchronises: all work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - Return value: 0 (ENH_OK) or a negative ENH_E_* code; a HIP launch error is returned as
 *     -(1000 + hipError_t).  enh_last_error() gives a thread-local human-readable message.  This mirrors
 *     the reference's native-op precedent, where TORCH_CHECK failures surface as a Python RuntimeError
 *     (enhancing/losses/op/fused_bias_act.cpp:9-15); the Python wrapper raises RuntimeError on rc != 0.
 *   - All functions are stateless and re-entrant (they are called from autograd worker threads too), EXCEPT the explicit library
 *     state behind the enh_*_set_* / enh_set_cu_budget / enh_debug_* setters (process-global kernel-family switches, meant for A/B measurements).
 *     Device-bound state — the CU count, the CU budget and the persistent GEMMs' tile-claim counters — is keyed by the calling thread's CURRENT
 *     device (hipGetDevice) since round 6: a process may drive several GPUs through this ABI (the library still never sets a device).
 *
 * The reference reaches this path through stock PyTorch ops, not an FFI; each entry
 * below cites the reference lines whose arithmetic it replaces.  Paths are relative to the reference
 * repository root.
 */
#ifndef ENH_HIP_H
#define ENH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENH_OK 0
#define ENH_E_BADARG (-1)      /* null pointer / non-positive size */
#define ENH_E_SHAPE (-2)       /* unsupported shape or alignment */
#define ENH_E_WORKSPACE (-3)   /* workspace too small */
#define ENH_E_HIP_BASE (-1000) /* rc = ENH_E_HIP_BASE - hipError_t */

/* 16-bit operand types.  Every MFMA operand of the product path is a 16-bit float in ONE of two formats, selected per call by the `dtype`
 * argument (always the parameter in front of `stream`):
 *   ENH_DT_BF16  bfloat16 (8 significand bits, f32's exponent range)         — v_mfma_f32_*_bf16, v_cvt_pk_bf16_f32
 *   ENH_DT_F16   IEEE binary16 (11 significand bits, max 65504, min normal 6.1e-5) — v_mfma_f32_*_f16, v_cvt_pk_f16_f32
 * Both roundings are round-to-nearest-even, accumulation is f32 in both, and the two run at the same MFMA rate.  fp16 is the reference's own
 * mixed-precision dtype (main.py:25,52: --use_amp -> Lightning precision=16 = fp16 autocast + GradScaler): its operand rounding is 8x smaller than
 * bf16's, which is what brings the activations within 1e-3 of the fp32 reference in ONE MFMA pass; gradients need a loss scale (enh_nonfinite_flag,
 * enh_adamw_step skip_flag).  Every 16-bit tensor of one call has the call's dtype; entries whose names still say "bf16" and take no dtype (the x3
 * split-operand family) are bf16-only.  The channels-last convolution family (discriminator, LPIPS trunk) takes the dtype too (round 6). */
#define ENH_DT_BF16 0
#define ENH_DT_F16 1
#define ENH_DT_F32 2   /* enh_im2col / enh_col2im only: f32 columns for the exact-f32 GEMM (the discriminator's parity instrument) */
typedef uint16_t enh_h16;  /* raw 16-bit float bits: bfloat16 or binary16, per the call's dtype */
typedef enh_h16 enh_bf16;  /* raw bfloat16 bits (bf16-only entries) */

const char* enh_last_error(void);
/* The symbol — as a profiler prints it: template arguments, no parameter list, e.g. "gemm_w256r_kernel<F16, false, 2, true>" — of the main kernel that
 * the calling thread's most recent enh_gemm_h16 / enh_gemm_h16_ws / enh_gemm_h16_dtanh_colsum / enh_gemm_bf16_split / enh_attention_forward(_dh) / stage-2 (gpt_decode, gpt_rows, gpt_prefill) call
 * enqueued: the GEMM or attention kernel, not the helpers that ride along (split-K second pass, column sums).  "" before the first such call.  The
 * launch records plain data; the string is composed here, into a thread-local buffer that the next call on the thread overwrites.  Timing labels are
 * taken from this (enhancing/_C.py KernelTimer), so a label is the kernel the planner launched and never a second guess at its decision. */
const char* enh_last_kernel(void);
#define ENH_ABI_VERSION 37/* bumped whenever a signature below changes; the bindings check it at load */
int enh_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Vector / residual quantizer  — enhancing/modules/stage1/quantizers.py:38-92
 * ------------------------------------------------------------------------------------------------
 * Code width d = embed_dim: any multiple of 8 in [8, 256] (every shipped config uses 32: configs/imagenet_vitvq_*.yaml:17-19); anything else
 * is ENH_E_SHAPE.  A width-d call runs on the compiled width DW = the smallest of {32, 64, 128, 256} that is >= d, as that width on the
 * inputs zero-padded to DW columns (loads masked to d, padding never stored): appended exact zeros change no sum below, so every d <= 32
 * is bit-for-bit the width-32 contract on zero-padded rows.
 * Arithmetic contract at width DW (the DW = 32 case is restated bit-exactly by oracle/vq_oracle.c):
 *   n(x) = x / max(sqrt(S(x)), 1e-12),  S(x) = c_0 + c_1 + ... + c_{DW/16-1} added left to right, c_j = chain(x[16j..16j+15]),
 *   chain = ascending fmaf chain from 0 (DW = 32: S = chain(x[0..15]) + chain(x[16..31]));  zz = S(zn), ee_k = S(en_k);
 *   dot_k = f32 MFMA 32x32x2 accumulation (exact f32) over the column order 0, DW/2, 1, DW/2+1, ..., DW/2-1, DW-1
 *           (DW = 32: 0,16,1,17,...,15,31);
 *   d_k = (zz + ee_k) - 2*dot_k ; idx = argmin_k d_k, lowest k on ties  (quantizers.py:78-83).
 * Losses are means over the true M*d elements.  The same bits on every run at every width.
 */

/* bytes of scratch needed by enh_vq_forward / enh_vq_backward for a codebook of n_embed codes of width embed_dim and M tokens.
 * Scale: the backward keeps one contribution vector per (token, depth), M*depth*embed_dim floats — at M = 131 072, depth 8 and
 * embed_dim 256 that alone is 1 GiB. */
size_t enh_vq_workspace_bytes_d(int64_t M, int n_embed, int embed_dim, int depth);
/* the same at embed_dim 32 */
size_t enh_vq_workspace_bytes(int64_t M, int n_embed, int depth);

/* Forward of BaseQuantizer.forward + VectorQuantizer.quantize (quantizers.py:38-63,74-92).
 *   z        [M,d] f32    quantizer input (pre_quant output)
 *   codebook [K,d] f32    quantizer.embedding.weight
 *   depth    1 = plain VQ ; >1 = residual quantizer with one shared codebook (use_residual, num_quantizers); <= 8 when d > 32
 *   zq_out   [M,d] f32    straight-through VALUE  z + (sum_i en_i - z)          (quantizers.py:61)
 *   zq_h16   [M,d] 16-bit optional (may be NULL): same, rounded to `dtype` (operand of post_quant GEMM)
 *   idx_out  [M,depth] i64 code indices (stacked on the last axis as quantizers.py:55)
 *   loss_out [1] f32      mean_i( beta*mean((en_i-zn_i)^2) + mean((en_i-zn_i)^2) ) (quantizers.py:56,89-90)
 */
int enh_vq_forward(const float* z, const float* codebook, int64_t M, int n_embed, int embed_dim,
                   float beta, int depth, int use_norm, float* zq_out, enh_h16* zq_h16,
                   int64_t* idx_out, float* loss_out, void* workspace, size_t workspace_bytes,
                   int dtype, void* stream);

/* Backward (derived from the reference autograd graph):
 *   g_out   [M,d] f32   grad wrt returned z_q;  g_loss_dev: optional device scalar multiplying g_loss
 *   use_residual: 1 when the forward ran the residual loop (z is detached at quantizers.py:43, so the
 *           encoder then receives g_out only, and the codebook grad gets the cross-depth term)
 *   dz      [M,d] f32   (VQ: g_out + beta-term through the normalise Jacobian; RQ: g_out only)
 *   dz_h16 optional 16-bit copy (`dtype`) ; d_codebook [K,d] f32 is ACCUMULATED into (caller zeroes it).
 */
int enh_vq_backward(const float* z, const float* codebook, const int64_t* idx, const float* g_out,
                    float g_loss, const float* g_loss_dev, int64_t M, int n_embed, int embed_dim,
                    float beta, int depth, int use_residual, int use_norm, float* dz, enh_h16* dz_h16,
                    float* d_codebook, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* decode_codes front half (vitvqgan.py:81-87): out[m] = sum_i n(codebook[idx[m,i]]) ([M,d]) as f32 and as a 16-bit operand (`dtype`) */
int enh_vq_lookup(const float* codebook, const int64_t* idx, int64_t M, int n_embed, int embed_dim,
                  int depth, int use_norm, float* out, enh_h16* out_h16, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused Gumbel-softmax quantizer — GumbelQuantizer.quantize, enhancing/modules/stage1/quantizers.py:103-126 (one level; the residual
 * loop of quantizers.py:38-63 is the caller's)
 * ------------------------------------------------------------------------------------------------
 *   zn = n(z), en = n(E)   (n = F.normalize, eps 1e-12, or the identity when use_norm = 0; sums as in the quantizer contract above)
 *   l_k = (2 zn.en_k - |zn|^2) - |en_k|^2     the dot on the exact-f32 MFMA, column order 0,16,1,17,...,15,31       (quantizers.py:107-109)
 *   y = softmax((l + g) / tau),  z_q = y @ en                                                                      (quantizers.py:111-114)
 *   p = softmax(l),  loss = mean over the M tokens of sum_k p_k (log p_k + log K)                                  (quantizers.py:117-118)
 *   idx = argmax_k (l_k + g_k), lowest k on ties                                                                   (quantizers.py:120)
 * No [M,K] buffer is written by any entry but the noise dump.  embed_dim: a multiple of 8 in [8, 32] (width 32, zero padding), else ENH_E_SHAPE.
 * The same bits on every run (no float atomics).
 *
 * Noise:  g(seed, call, m, k) = -log(-log(u)),  u = (x >> 9) * 2^-23 + 2^-24  (23 bits: u in [2^-24, 1 - 2^-24], open at both ends),
 *   x = word (k & 3) of Philox4x32-10 with key (k0, k1) = (seed & 0xffffffff, seed >> 32) and counter
 *   (c0, c1, c2, c3) = (k >> 2, m & 0xffffffff, m >> 32, call);  the logs are the hardware log2 times ln 2 (the inner one clamped below at 5e-8).
 *   m = token row, k = code.  Nothing else enters: not M, K, the launch geometry, or which entry asks.  One device function serves all entries. */

/* bytes of scratch of enh_gumbel_forward / enh_gumbel_backward: the prepared codebook, and for the backward the normalised tokens [M,32]
 * and up to 64 slab partials of the codebook gradient [Kpad,32] */
size_t enh_gumbel_workspace_bytes(int64_t M, int n_embed, int embed_dim);

/* Forward (quantizers.py:103-126).
 *   z [M,d] f32, codebook [K,d] f32;  tau > 0;  hard: 0 = z_q is y @ en, 1 = z_q is en[idx] (the value of y_hard - y.detach() + y)
 *   zq_out    [M,d] f32
 *   zq_soft   [M,d] f32   hard = 1 only, optional: y @ en, which enh_gumbel_backward needs (hard = 0: zq_out is that already; ignored)
 *   idx_out   [M] i64,  loss_out [1] f32
 *   stats_out [5,M] f32   saved for the backward: max and sum of exp of both softmaxes (l, then (l+g)/tau), and the token's loss term */
int enh_gumbel_forward(const float* z, const float* codebook, int64_t M, int n_embed, int embed_dim, float tau, int hard, int use_norm,
                       uint64_t seed, uint32_t call, float* zq_out, float* zq_soft, int64_t* idx_out, float* loss_out, float* stats_out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above (the autograd graph of quantizers.py:103-122).  hard = 1: the gradient through y is that of the soft y, as with hard = 0;
 * en's own term of z_q = y_st @ en takes the one-hot value, y_hard^T g_zq in place of y^T g_zq, so the forward's idx [M] is needed (hard = 0: unused,
 * may be NULL).
 *   zq_soft, stats: the forward's outputs;  seed, call, tau, hard, use_norm: the forward's
 *   g_zq [M,d] f32 grad wrt z_q;  g_loss * (g_loss_dev ? *g_loss_dev : 1) = grad wrt the loss
 *   dz [M,d] f32;  d_codebook [K,d] f32 is ACCUMULATED into (caller zeroes it) */
int enh_gumbel_backward(const float* z, const float* codebook, const float* zq_soft, const float* stats, const float* g_zq, float g_loss,
                        const float* g_loss_dev, int64_t M, int n_embed, int embed_dim, float tau, int hard, const int64_t* idx,
                        int use_norm, uint64_t seed, uint32_t call, float* dz, float* d_codebook, void* workspace, size_t workspace_bytes,
                        void* stream);

/* the noise the two entries above use in place of F.gumbel_softmax's draw (torch/nn/functional.py gumbel_softmax, called at quantizers.py:111):
 * out [M,K] f32, out[m,k] = g(seed, call, m, k).  For tests and debugging. */
int enh_gumbel_noise(uint64_t seed, uint32_t call, int64_t M, int n_embed, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm — nn.LayerNorm(dim), eps 1e-5, biased variance (enhancing/modules/stage1/layers.py:85-92,143)
 * ------------------------------------------------------------------------------------------------ */
/* y = (x-mean)*rstd*w + b.  x [M,D] f32; y_h16 [M,D] (GEMM operand, `dtype`) and/or y_f32 (either may be NULL);
 * mean,rstd [M] f32 saved for backward (may be NULL for inference).  D % 4 == 0, D <= 2048. */
int enh_layernorm_forward(const float* x, const float* w, const float* b, int64_t M, int D, float eps,
                          enh_h16* y_h16, float* y_f32, float* mean, float* rstd, int dtype, void* stream);
/* dx = LN-backward(dy) [+ dres];  the upstream gradient [M,D] is passed EITHER as dy (f32) OR as dy_h16 (the 16-bit output of the dgrad
 * GEMM that produced it) — exactly one non-NULL;  dres optional f32 residual-stream gradient that is added;
 * dx_f32 [M,D] f32 and optional dx_h16 copy; dw,db [D] f32 are ACCUMULATED (atomics; caller zeroes);
 * dx_colsum [D] f32, optional: += column sums of dx — the bias gradient of the Linear whose output feeds this
 * residual stream (to_out / fc2), fused here so no separate reduction pass over dx is needed. */
int enh_layernorm_backward(const float* dy, const enh_h16* dy_h16, const float* x, const float* w, const float* mean,
                           const float* rstd, const float* dres, int64_t M, int D, float* dx_f32,
                           enh_h16* dx_h16, float* dw, float* db, float* dx_colsum, int dtype, void* stream);
/* Deterministic form: the per-workgroup column partials of dw / db / dx_colsum go to `ws` (enh_layernorm_backward_workspace_bytes) and a second pass
 * adds them in a fixed order — bit-reproducible from run to run; enh_layernorm_backward uses f32 atomics instead. */
size_t enh_layernorm_backward_workspace_bytes(int64_t M, int D);
int enh_layernorm_backward_ws(const float* dy, const enh_h16* dy_h16, const float* x, const float* w, const float* mean,
                              const float* rstd, const float* dres, int64_t M, int D, float* dx_f32, enh_h16* dx_h16, float* dw,
                              float* db, float* dx_colsum, void* ws, size_t ws_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 16-bit-operand MFMA GEMM with fused epilogue — every nn.Linear / patch conv on the path
 * (layers.py:99-101,118,120,169,204; vitvqgan.py:38-39) and their dgrad / wgrad.
 * ------------------------------------------------------------------------------------------------
 * C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ),  A, B (and aux, c_h16) in `dtype`, f32 accumulation on v_mfma_f32_32x32x16_{bf16,f16} /
 * v_mfma_f32_16x16x32_{bf16,f16}.  Shapes, plans, tile order and split-K decisions do not depend on dtype.
 *   trans_a = 0: A stored [M][K] (lda elements between rows) ; 1: A stored [K][M]
 *   trans_b = 0: B stored [N][K] (nn.Linear.weight layout)   ; 1: B stored [K][N]
 *   epilogue, in this order:  v = acc ; v += bias[n] (f32, optional) ; v = tanh(v) if act == 1 ;
 *     v *= (1 - aux[m,n]^2) if act == 2 (aux = saved tanh output: tanh backward) ;
 *     v += res[(m % res_rows), n] (f32, optional; res_rows = M for a residual, n_tokens for a pos-embed) ;
 *     v += C_old if accumulate ;  store to c_f32 and/or c_h16 (ldc).
 *   Requirements: K % 8 == 0, lda/ldb % 8 == 0, 16-byte aligned bases; for trans_a M % 8 == 0; trans_b N % 8 == 0.
 */
#define ENH_ACT_NONE 0
#define ENH_ACT_TANH 1
#define ENH_ACT_DTANH 2
int enh_gemm_h16(const enh_h16* A, int64_t lda, int trans_a, const enh_h16* B, int64_t ldb, int trans_b,
                 int64_t M, int64_t N, int64_t K, const float* bias, int act, const enh_h16* aux,
                 int64_t ldaux, const float* res, int64_t ldres, int64_t res_rows, int accumulate,
                 float* c_f32, enh_h16* c_h16, int64_t ldc, int dtype, void* stream);

/* The same with a caller-owned split-K workspace.  Weight-gradient-shaped calls (accumulate = 1, f32 output only, no bias / act / res) whose
 * output tiles cannot fill the chip are split along K; with a workspace of enh_gemm_h16_workspace_bytes() the K slices write partial slabs
 * [splits][M][N] and a second pass adds them to C in a fixed order: bit-reproducible, no f32 atomics (needs ldc == N).  workspace = NULL
 * (what enh_gemm_h16 passes) falls back to f32 atomicAdd into C.  Replaces the autograd wgrad of every nn.Linear (layers.py:99-101,118,120).
 * Round 6 (the reference's shipped batch sizes, configs/imagenet_vitvq_large.yaml:31: 2 images per GPU): with a workspace, calls WITHOUT an activation whose
 * 128 x 128 tiles cover less than half of the resident workgroup slots and whose K >= 2048 are split as well — f32 output with any of bias / residual /
 * accumulate, or a plain 16-bit output; the second pass then carries the epilogue (bias, residual row m mod res_rows, previous C; or the one RNE pack).
 * Same bits for the same call and workspace size; a workspace smaller than enh_gemm_h16_workspace_bytes() simply means "do not split" for these calls.
 * Never chosen at training sizes (M >= 8192 token rows with N >= 768 has >= 256 tiles). */
int enh_gemm_h16_ws(const enh_h16* A, int64_t lda, int trans_a, const enh_h16* B, int64_t ldb, int trans_b,
                    int64_t M, int64_t N, int64_t K, const float* bias, int act, const enh_h16* aux,
                    int64_t ldaux, const float* res, int64_t ldres, int64_t res_rows, int accumulate,
                    float* c_f32, enh_h16* c_h16, int64_t ldc, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* C[M,N] = (A B) * (1 - aux^2) -> 16-bit AND colsum[n] (+)= sum_m C[m][n] over the stored (rounded) values: the input gradient through a tanh plus the
 * bias gradient of the Linear in front of it — the autograd of `nn.Linear -> nn.Tanh` in FeedForward (layers.py:99-101).  On whole 256 x 256 tiles
 * the tanh' kernel's epilogue leaves one partial row per 128 rows in `ws` and a fixed-order second pass adds them (bit-reproducible; the separate
 * column-sum kernel re-reads all of C: 805 MB per layer at the base config); any other shape runs enh_gemm_h16 then enh_colsum_h16_ws.
 * A is [M][K] (never transposed here); trans_b as in enh_gemm_h16. */
size_t enh_gemm_h16_dtanh_colsum_workspace_bytes(int trans_b, int64_t M, int64_t N, int64_t K);
int enh_gemm_h16_dtanh_colsum(const enh_h16* A, int64_t lda, const enh_h16* B, int64_t ldb, int trans_b, int64_t M, int64_t N, int64_t K,
                              const enh_h16* aux, int64_t ldaux, enh_h16* c_h16, int64_t ldc, float* colsum, int accumulate_colsum,
                              void* ws, size_t ws_bytes, int dtype, void* stream);
/* bytes of workspace the split-K plan of this shape needs, whichever kind of call (weight-gradient or forward kind) would split it (0 = never split) */
size_t enh_gemm_h16_workspace_bytes(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K);

/* name of the kernel family enh_gemm_h16 launches for this shape (measurement aid: lets callers label timings with
 * the symbol a profiler will report); the choice is per shape */
const char* enh_gemm_h16_variant(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K);
/* the same for a call with a given fused epilogue (epi_mode: 0 generic, 1 16-bit, 2 16-bit + bias + tanh, 3 16-bit * tanh', 4 f32 + bias + residual stream,
 * 5 f32, 6 / 7 split-K partials): forward / input-gradient calls of modes 1-5 on whole 256 x 256 tiles run a PERSISTENT form of the 256 x 256
 * kernel — "gemm_w256p_kernel": one workgroup per CU walks the tiles, the next tile's operands are requested before the stores of this one;
 * "gemm_w256r_kernel" (modes 1, 2, 5; an even number >= 6 of 64-deep K stages): the same with the A operand staged through registers two
 * stages ahead, which lets its requests stay in flight 1.75 stages instead of 0.75 */
const char* enh_gemm_h16_variant_mode(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, int epi_mode);
/* A/B measurement aid: force a kernel family for every later call that it can serve (-1 = per-shape choice [default], 0 = register-staged
 * fallback, 3 = pipe2 128x128, 7 = w256 256x256 / 4 waves with one tile per workgroup everywhere, 8 = w256 with the persistent form w256p where it
 * serves, 9 = as 8 plus w256r where that serves [what the default picks]).  Process-global, set explicitly by the caller (the Python
 * binding maps the ENH_GEMM_KERNEL environment variable onto it); the library itself reads no environment. */
int enh_gemm_set_kernel(int family);
/* Tile schedule of the persistent 256 x 256 kernels: 1 [default] = tiles are CLAIMED from one queue per XCD (atomic counters in library-owned device
 * words; the queue order is the static walk's, so operand slices still meet in one L2) — a workgroup that gets its CU late finds the queue empty and
 * exits, the launch slows by (CUs held by others) / CUs; 0 = static partition (workgroup b walks tiles b, b + grid, ...: every workgroup must run, a
 * collective's kernel holding k CUs at dispatch costs up to 2x on that launch).  Same result bits either way.  Process-global measurement switch. */
int enh_gemm_set_scheduler(int dynamic);
/* CU budget: the number of CUs GEMM launches may count on (persistent grid size, one-round split-K plans); 0 = all CUs of the device [default].
 * Data-parallel training sets it to (CUs - the collective's channels) while gradient buckets are in flight (engine/ddp.py; reference main.py:54-57 is
 * DDP over NCCL).  enh_get_cu_budget returns the effective value. */
int enh_set_cu_budget(int n_cus);
int enh_get_cu_budget(void);
/* Measurement aid: holds n_wg CUs (one workgroup each, the CU's whole LDS) for ms milliseconds (clamped to 2000) on `stream` — the stand-in for a
 * collective's kernel in the one-GPU contention experiment (tools/comm_contention.py). */
/* measurement only (results are WRONG while it is on): the split-K weight-gradient loop with 1 = plain 16-byte fragment reads instead of the
 * transposing ones (same LDS bytes), 2 = no fragment reads, 3 = neither fragment reads nor staging requests (MFMAs + barriers), 4 = every second
 * staging request, 5 = all fragment reads, no staging requests, 6 .. 9 = the shipped loop with cache-policy bits sc0 / nt / sc1 / sc0 + sc1 on its
 * staging requests (correct results); 0 = off (tools/wgrad_lab.py, profiles/r04_gemm_fill_lab.txt) */
int enh_debug_gemm_lab(int variant);
/* Measurement aid (results unchanged): tile order of the forward / input-gradient GEMMs — `grp_rows` row panels per group (8, rows fastest: the 32
 * workgroups of an XCD have an 8 x 4 patch of tiles in flight), col_fast = 1: columns fastest inside a group (a few rows x ALL column tiles in flight:
 * every A panel is fetched by one XCD once).  grp_rows = 0: the library's per-shape default (col_fast for K >= 2048).  tools/gemm_ld_lab.py,
 * profiles/r05_gemm_landing_lab.txt */
int enh_debug_gemm_order(int grp_rows, int col_fast);
/* Measurement aid: force the number of K slices of the split-K plans (weight gradients); 0 = the planner's choice.  With 8 x (tiles per slice)
 * workgroups every XCD holds whole slices (profiles/r05_gemm_landing_lab.txt §5). */
int enh_debug_gemm_splits(int splits);
int enh_debug_occupy_cus(int n_wg, float ms, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused attention — Attention.forward layers.py:122-132 without materialising the N x N matrix
 * ------------------------------------------------------------------------------------------------
 * qkv [B,N,3*H*64] 16-bit (`dtype`) packed exactly as to_qkv emits it (q | k | v thirds, head-major, layers.py:123-124);
 * out [B,N,H*64] 16-bit in the 'b n (h d)' layout to_out consumes (layers.py:130); lse [B,H,N] f32 =
 * row log-sum-exp of the scaled scores (saved for backward).  dim_head = 64; N any positive int: every (image, head) attends over its own keys
 * 0 .. N-1.  N % 64 == 0 runs the aligned kernels; any other N their TAIL forms (attn_fwd_tail_* / attn_bwd_tail_*: the ragged last 64-row tile is
 * read with its rows clamped to the image, its keys >= N get probability exactly 0, stores are per row) — nothing outside the tensors is read or written.
 * q_prescaled = 1: the q third already holds q * scale * log2(e) (the caller folded the softmax scale into the projection's q rows, once, in
 * fp32 before the 16-bit rounding).  The score products are then log2-domain logits and the kernels feed -max / -lse / -delta through the MFMA C
 * operand instead of spending vector instructions on them (the kernels are vector-issue bound, profiles/r03_attention_lab.txt).  Semantics are
 * unchanged: out / lse are those of softmax(q k^T scale) v for the UNSCALED q, dqkv's q third is the gradient with respect to the unscaled q.
 */
/* NaN note: the attention objects are built with -fno-honor-nans (the row maxima must fuse into v_max3_f32 without canonicalising moves): scores that
 * contain NaN (a diverged run) are NOT guaranteed to propagate as NaN through out / lse — check the loss / the gradients (enh_nonfinite_flag) instead. */
int enh_attention_forward(const enh_h16* qkv, int B, int N, int H, float scale, int q_prescaled, enh_h16* out, float* lse,
                          int dtype, void* stream);
/* kernel family per pass for A/B measurements (explicit library state, like enh_gemm_set_kernel), 0 = the library's choice:
 *   fwd: 1 four-wave kernel (round 2; serves both q conventions), 5 the same skeleton with the running reference as the MFMA C operand, a packed exact row
 *        sum and the K / V tiles by LDS-DMA (round 5; pre-scaled q, otherwise family 1) [default]
 *   dq : 1 round-2 arithmetic, 3 -delta (-lse too when q is pre-scaled) as MFMA C operands [default since round 5]
 *   dkv: 1 round-2 arithmetic, 2 -delta (-lse too when q is pre-scaled) as MFMA C operands [default]
 * (the software-pipelined round-3 kernels and the eight-wave antiphase kernels of round 4 were measured slower and are deleted.)
 * Same results up to rounding: every family passes the same parity and bit-reproducibility tests.
 * The families are the ALIGNED kernels.  With N % 64 != 0 the selection is accepted and ignored: there is one tail kernel per pass and q convention
 * (the tail form of the default family; forward with plain q: of family 1), and it runs whatever is selected here. */
int enh_attention_set_kernel(int fwd, int dq, int dkv);
/* dqkv [B,N,3*H*64] 16-bit ; delta_ws [B,H,N] f32 scratch.  With ENH_DT_F16 the caller keeps dout inside fp16's range (loss scale): p o (dP - delta) is
 * packed to fp16 before the dQ / dK products. */
int enh_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse,
                           int B, int N, int H, float scale, int q_prescaled, enh_h16* dqkv, float* delta_ws, int dtype, void* stream);
/* The same two calls with the head width as an argument D = dim_head — the reference's Attention takes it as a constructor argument
 * (layers.py:108-120; ViTEncoder / ViTDecoder pass it on, layers.py:154-155,186-187).  Layouts as above with 64 -> D: qkv / dqkv [B,N,3*H*D] packed
 * q | k | v head-major, out / dout [B,N,H*D], lse / delta_ws [B,H,N] f32; q_prescaled, scale and the meaning of dqkv's q third as above.
 *   D = 64            forwards to enh_attention_forward / enh_attention_backward: the same kernels (enh_attention_set_kernel, tail forms), the same bits
 *   D = 32 | 96 | 128 the attn_dh_* kernels (csrc/attention_dh.h): one kernel per pass for ANY N >= 1 and both q conventions — every tile is read with
 *                     its rows clamped to the image, keys >= N get probability exactly 0, stores are per row; dQ and dK/dV are separate kernels without
 *                     atomics (bit-reproducible); enh_attention_set_kernel does not apply
 *   anything else     ENH_E_SHAPE (80 and the other multiples of 16 would need padded output blocks)
 * The split-bf16 (x3) attention below exists for D = 64 only. */
int enh_attention_forward_dh(const enh_h16* qkv, int B, int N, int H, int D, float scale, int q_prescaled, enh_h16* out, float* lse,
                             int dtype, void* stream);
int enh_attention_backward_dh(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse,
                              int B, int N, int H, int D, float scale, int q_prescaled, enh_h16* dqkv, float* delta_ws, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * "x3" split-bf16 operands — the parity-grade ENCODER forward (round 4).  The reference's forward is fp32 end to end
 * (layers.py:118-132,145-150; vitvqgan.py:61-66; quantizers.py:74-92 consumes its output); bf16 operands flip ~2 % of the argmin decisions
 * downstream.  A value v is carried as hi = bf16(v), lo = bf16(v - hi) and a product as a_hi b_hi + a_lo b_hi + a_hi b_lo in the fp32 MFMA
 * accumulator: ~1e-5 relative end to end at a third of the bf16 MFMA rate (the exact-f32 MFMA has a sixteenth).
 * A GEMM is ONE enh_gemm_h16 (ENH_DT_BF16) call with K' = 3K on K-concatenated rows  A' = [a_hi | a_lo | a_hi],  B' = [b_hi | b_hi | b_lo].
 * ------------------------------------------------------------------------------------------------ */
/* y3[m] = the x3 row of f(x[m] (+ bias)), f = identity (act 0) or tanh (act 1: FeedForward's activation, layers.py:99-100);
 * order 0: [hi | lo | hi] (A operand), order 1: [hi | hi | lo] (B operand = weights).  x f32 [M,K] (ldx), y3 bf16 [M,3K] (ldy3),
 * y_hi optional bf16 [M,K] (ldy_hi): the hi plane alone (= what the bf16 path stores; the backward's operand).  K % 8 == 0. */
int enh_split3_bf16(const float* x, int64_t ldx, int64_t M, int64_t K, const float* bias, int act, int order, enh_bf16* y3, int64_t ldy3,
                    enh_bf16* y_hi, int64_t ldy_hi, void* stream);
/* hi[i] = bf16(x[i]), lo[i] = bf16(x[i] - hi[i]); n % 8 == 0 (the packed q | k | v projection for enh_attention_forward_x3) */
int enh_split2_bf16(const float* x, int64_t n, enh_bf16* hi, enh_bf16* lo, void* stream);
/* The x3 producers fused into the GEMM that computes their input (round 5): v = A B^T (A [M][K'], B [N][K'] row-major, K' = 3K x3 rows) or
 * v = tanh(A B^T + bias) — reference layers.py:118 (to_qkv) and :99-100 (Linear + Tanh) — leaves hi = bf16(v) in `hi` (and in `hi2`, `hi3` where non-null)
 * and lo = bf16(v - hi) in `lo` (each [M][N] with its own leading dimension), i.e. enh_gemm_h16 (f32 out) + enh_split2_bf16 / enh_split3_bf16 without the f32
 * round trip; plain mode bit-identical to that pair.  act: ENH_ACT_NONE (bias must be null) | ENH_ACT_TANH (bias required).  Served where the persistent
 * 256 x 256 kernel serves: enh_gemm_bf16_split_fused(M, N, K') == 1 (M, N multiples of 256, enough tiles to fill the chip); ENH_E_SHAPE otherwise. */
int enh_gemm_bf16_split_fused(int64_t M, int64_t N, int64_t K);
int enh_gemm_bf16_split(const enh_bf16* A, int64_t lda, const enh_bf16* B, int64_t ldb, int64_t M, int64_t N, int64_t K, const float* bias, int act,
                        enh_bf16* hi, int64_t ldhi, enh_bf16* lo, int64_t ldlo, enh_bf16* hi2, int64_t ldhi2, enh_bf16* hi3, int64_t ldhi3, void* stream);
/* enh_layernorm_forward that writes the x3 row y3 [M,3D] (and, optionally, the plain bf16 / f32 outputs); same statistics bits */
int enh_layernorm_forward_x3(const float* x, const float* w, const float* b, int64_t M, int D, float eps, enh_bf16* y3, enh_bf16* y_bf16,
                             float* y_f32, float* mean, float* rstd, void* stream);
/* enh_attention_forward on split operands: qkv_hi / qkv_lo [B,N,3*H*64] (unscaled q); S = Q K^T and O = P V as three MFMA passes each,
 * softmax statistics in fp32.  out3 [B,N,3*H*64] = the x3 row [hi | lo | hi] of the 'b n (h d)' output (A operand of to_out);
 * out_bf16 optional [B,N,H*64] (= the hi plane, what enh_attention_backward reads); lse as enh_attention_forward.  N any positive int (N % 64 != 0:
 * attn_fwd_tail_x3_kernel, as above). */
int enh_attention_forward_x3(const enh_bf16* qkv_hi, const enh_bf16* qkv_lo, int B, int N, int H, float scale, enh_bf16* out3,
                             enh_bf16* out_bf16, float* lse, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Patch (un)embedding data movement, pixel loss, reductions, optimizer
 * ------------------------------------------------------------------------------------------------ */
/* 'b c h w -> (b gy gx) (c ph pw)' gather of Conv2d(k=s=p) as a GEMM operand (layers.py:168-171,178);
 * also maps an image-layout gradient to the patch layout (same permutation). */
int enh_patchify(const float* img, int B, int C, int H, int W, int p, enh_h16* patches, int dtype, void* stream);
/* Inverse scatter of ConvTranspose2d(k=s=p) (layers.py:202-205,212) fused with the pixel losses
 * (vqperceptual.py:113-114): pix [M, C*p*p] f32 (to_pixel GEMM output incl. bias) -> xrec [B,C,H,W] f32;
 * if target != NULL: sums[0] += sum|xrec-x|, sums[1] += sum (xrec-x)^2 (f64 atomics; caller zeroes) and
 * dpix_h16 [M, C*p*p] (`dtype`) = (w_l1*sign(diff) + w_l2*2*diff) / numel  (grad of w_l1*L1 + w_l2*L2), optional; grad_scale_dev (optional device
 * float) multiplies dpix only — the loss scale of an ENH_DT_F16 backward, kept on the device (enh_loss_scale_update); the sums are unaffected. */
int enh_unpatchify_loss(const float* pix, const float* target, int B, int C, int H, int W, int p, float w_l1,
                        float w_l2, float* xrec, double* sums, enh_h16* dpix_h16, const float* grad_scale_dev, int dtype, void* stream);
/* out[n] (+)= sum_m x[m,n] (bias gradients); x 16-bit [M,N] (`dtype`) */
int enh_colsum_h16(const enh_h16* x, int64_t M, int64_t N, int64_t ldx, float* out, int accumulate, int dtype, void* stream);
/* deterministic form: per-row-chunk partials in `ws` (enh_colsum_h16_workspace_bytes), added in a fixed order; enh_colsum_h16 uses f32 atomics */
size_t enh_colsum_h16_workspace_bytes(int64_t M, int64_t N);
int enh_colsum_h16_ws(const enh_h16* x, int64_t M, int64_t N, int64_t ldx, float* out, int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream);
/* f32 -> 16-bit cast, round-to-nearest-even (weight shadows) */
int enh_cast_f32_h16(const float* x, enh_h16* y, int64_t n, int dtype, void* stream);
/* y[i] = h16(x[i] * (i < n_scaled ? alpha : 1)), n_scaled % 4 == 0: forward operand of a packed q | k | v projection weight whose leading q rows carry
 * the softmax scale * log2(e) (one rounding from the fp32 master; see enh_attention_forward, q_prescaled) */
int enh_cast_f32_h16_head_scaled(const float* x, enh_h16* y, int64_t n, int64_t n_scaled, float alpha, int dtype, void* stream);
/* the same for `count` equally spaced blocks (block b reads x + b*x_stride, writes y + b*y_stride; strides in elements, multiples of 4): the to_qkv weights of
 * every layer of a tower in one launch */
int enh_cast_f32_h16_head_scaled_strided(const float* x, int64_t x_stride, enh_h16* y, int64_t y_stride, int64_t n, int64_t n_scaled, float alpha,
                                         int count, int dtype, void* stream);
/* torch.optim.AdamW(lr, betas=(0.9,0.99), weight_decay=1e-4) step over one flat buffer (vitvqgan.py:160),
 * also refreshes the 16-bit operand shadow p_h16 (`dtype`) used by the GEMMs.  grad_scale multiplies g first (DDP mean / accumulation / 1 / loss scale).
 * skip_flag (optional device float): non-zero = drop this step — nothing is written (p, m, v, p_h16 unchanged): the inf / nan skip of
 * torch.cuda.amp.GradScaler.step under the reference's --use_amp (main.py:25,52); the flag comes from enh_nonfinite_flag.
 * loss_scale_dev (optional device float): g is additionally divided by it (GradScaler's unscale folded into the step).
 * clip_coef_dev (optional device float): multiplied into the gradient scale after the loss-scale division — the coefficient of
 * torch.nn.utils.clip_grad_norm_, from enh_grad_clip_coef (out + 1).  clip_value (0 = off): the unscaled gradient g * scale is clamped to
 * [-clip_value, clip_value] before the moments (Lightning's gradient_clip_algorithm="value"; a nan stays a nan).  With NULL and 0 the step is the
 * step without these operands, bit for bit.
 * step_state (optional device double[3], 8-byte aligned; ABI v34): the step number lives on the device — (t, 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) with t
 * the number of APPLIED steps; `step` is then not read.  A one-thread launch in front of the AdamW kernel advances t and forms the two factors for it
 * unless skip_flag is set: a dropped step leaves the count where it was, as GradScaler.step leaves AdamW's (start from (t0, any, any); only t is state).
 * With NULL the bias corrections are those of `step` (>= 1), formed on the host: the launch of before. */
int enh_adamw_step(float* p, const float* g, float* m, float* v, enh_h16* p_h16, int64_t n, int step, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float grad_scale, const float* skip_flag, const float* loss_scale_dev,
                   const float* clip_coef_dev, float clip_value, double* step_state, int dtype, void* stream);
/* GradScaler.update() on the device: found_inf != 0 -> *scale *= backoff_factor, *growth_tracker = 0; otherwise ++*growth_tracker and after
 * growth_interval clean steps in a row *scale *= growth_factor (growth_interval = 0: never grow = a static scale with backoff).  *scale is kept
 * inside [1, 2^24].  torch defaults: growth 2, backoff 0.5, interval 2000, initial scale 65536. */
int enh_loss_scale_update(float* scale, const float* found_inf, int* growth_tracker, float growth_factor, float backoff_factor, int growth_interval,
                          void* stream);
/* flag[0] = 1.0f if any of x[0..n) is inf or nan, otherwise untouched (the caller zeroes it once per step): GradScaler's found-inf check over one flat
 * gradient buffer, one pass at HBM rate.  x 16-byte aligned. */
int enh_nonfinite_flag(const float* x, int64_t n, float* flag, void* stream);
/* Gradient-norm clipping over one flat gradient g[0..n) (f32, 16-byte aligned), the arithmetic of torch.nn.utils.clip_grad_norm_ (what Lightning's
 * Trainer(gradient_clip_val, track_grad_norm=2) does around the reference's optimizers, main.py:51-61):
 *   out[0] = total_norm = sqrt(sum g_i^2) * grad_scale / (loss_scale_dev ? *loss_scale_dev : 1)
 *   out[1] = coef       = min(1, max_norm / (total_norm + 1e-6))          (out: device f32[2]; pass out + 1 to enh_adamw_step as clip_coef_dev)
 * max_norm = +inf: coef = 1 exactly (the norm is measured, nothing is clipped).  found_inf (optional device float): set to 1.0f when g holds an inf or
 * nan, otherwise untouched — enh_nonfinite_flag's check in the same pass, so a loss-scaled step that wants the norm reads g once, not twice.
 * One pass over g at HBM rate (16-byte loads, the grid of enh_nonfinite_flag) + a one-workgroup finishing launch, both on `stream`: no host round
 * trip, safe to capture into a HIP graph.  The four squares of a load are added in f32, everything above that in f64 in a fixed order, no atomics:
 * relative error of the sum <= 4 * 2^-24 at any n, and the same bits on every run.  ws: enh_grad_clip_coef_workspace_bytes(n) bytes, 8-byte aligned.
 * A non-finite norm without found_inf (an engine without a loss scale) follows plain arithmetic, like torch: norm = inf -> coef = 0 (the finite
 * elements then contribute 0 and the inf ones nan), or nan when max_norm is inf as well; norm = nan -> coef = nan. */
size_t enh_grad_clip_coef_workspace_bytes(int64_t n);
int enh_grad_clip_coef(const float* g, int64_t n, float max_norm, float grad_scale, const float* loss_scale_dev, float* found_inf, float* out,
                       void* ws, size_t ws_bytes, void* stream);
/* One torch.optim.Adam step (no amsgrad, no maximize) of the stage-2 GPT (reference modules/stage2/transformer.py:132-194: betas (0.9, 0.96), L2 weight
 * decay 0.01 on the Linear weights only) over flat f32 p, g, m, v [n] (16-byte aligned, n % 64 == 0, int64 indices), in ONE launch driven by a device
 * segment table (csrc/gpt_adam.hip).  segments: nseg entries of 32 bytes {int64 begin, int64 end, int64 dst16, float weight_decay, int32 0}, sorted by
 * begin, disjoint, every bound a multiple of 64; elements outside every segment are never written.  Per element, in f32:
 *   gg = g * grad_scale / *loss_scale_dev * *clip_coef_dev;  clamp to +-clip_value if > 0;  gg += weight_decay * p;
 *   m = m + (gg - m) * (1 - beta1);  v = v * beta2 + gg * gg * (1 - beta2);  p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
 * (grad_scale, loss_scale_dev, clip_coef_dev, clip_value and skip_flag as in enh_adamw_step; 1 - beta is formed in double and rounded to float once).
 * dst16 >= 0: the new p of the segment is also written, round-to-nearest-even in the call's `dtype`, to arena[dst16 + (e - begin)] (dst16 % 8 == 0;
 * arena: arena_n 16-bit elements, may be NULL with arena_n = 0); other arena bytes are never written.
 * state: device double[4] = {t, beta1^t, beta2^t, unused}, {0, 1, 1, 0} before the first step.  A one-workgroup launch advances it when skip_flag is
 * NULL or zero; the step then uses bc1 = 1 - state[1], bc2 = 1 - state[2].  With a non-zero skip_flag NOTHING is written: p, m, v, arena and state keep
 * their bits (torch.cuda.amp.GradScaler does not advance the optimizer's step when it drops one).  No host round trip, no atomics; the same bits on
 * every run.  A gradient multiplied by a power of two S with *loss_scale_dev = S gives the bits of the plain gradient with loss_scale_dev NULL. */
int enh_adam_step_segments(float* p, const float* g, float* m, float* v, int64_t n, enh_h16* arena, int64_t arena_n, const void* segments, int nseg,
                           double* state, float lr, double beta1, double beta2, float eps, float grad_scale, const float* skip_flag,
                           const float* loss_scale_dev, const float* clip_coef_dev, float clip_value, int dtype, void* stream);
/* enh_adam_step_segments with the two moments held as bf16 (m16, v16: uint16_t [n], 16-byte aligned): 22 bytes per element instead of 30.  Everything
 * not listed here is enh_adam_step_segments' contract: the segment table, padding never written, the arena image, the device step state advanced by the
 * one-workgroup launch, and skip (a non-zero skip_flag writes nothing, m16 and v16 included).  No atomics.
 * Per element: the old moments are widened exactly (bf16 << 16); gg, the new m and the new v are computed in f32 by the expressions above; p is updated
 * from the UNROUNDED f32 new moments (a step's own rounding never enters its own update); only what is stored for the next step is rounded.
 * Stored rounding of an f32 bit pattern u with a 16-bit word r: a finite u is stored as (u + r) >> 16 — stochastic rounding: up with probability
 * (low half) / 2^16 — and where that would carry a finite value to infinity, as the largest finite bf16 of that sign; a nan or an infinity is stored
 * by truncation with the quiet bit kept (nan stays nan, inf stays inf).  Integer arithmetic only, so the same through subnormals.
 * The words: the 4 consecutive elements of group G = e / 4 take one call
 *   philox4x32_10((uint32)sr_seed, (uint32)(sr_seed >> 32), {(uint32)G, (uint32)(G >> 32), (uint32)t, (uint32)(t >> 32)})
 * with t = the number of applied steps after the advance (state[0]); word k serves element 4G + k: its low 16 bits round m, its high 16 bits v.  A
 * dropped step consumes no randomness (t does not move); the same seed gives the same bits on every run.  sr_words (optional, uint32 [n], 16-byte
 * aligned; tests only) replaces the Philox words with sr_words[e], laid out the same way (low half m, high half v). */
int enh_adam_step_segments_s16(float* p, const float* g, uint16_t* m16, uint16_t* v16, int64_t n, enh_h16* arena, int64_t arena_n, const void* segments,
                               int nseg, double* state, float lr, double beta1, double beta2, float eps, float grad_scale, const float* skip_flag,
                               const float* loss_scale_dev, const float* clip_coef_dev, float clip_value, uint64_t sr_seed, const uint32_t* sr_words,
                               int dtype, void* stream);

/* Device-side tail of the input pipeline (enhancing/dataloader/imagenet.py:26-54: ... RandomCrop / CenterCrop -> RandomHorizontalFlip -> ToTensor):
 * src uint8 [B,Hs,Ws,3] (decoded + resized images, each in the top-left corner of its slot), meta int32 [B,3] = (y0, x0, flip) -> out f32 [B,3,R,R] in [0,1].
 * The window (y0..y0+R, x0..x0+R) must lie inside the image; exact (uint8 / 255.0f). */
int enh_crop_flip_u8(const uint8_t* src, int B, int Hs, int Ws, const int32_t* meta, int R, float* out, void* stream);
/* Resize of the reference's dataset transforms (torchvision T.Resize = PIL.Image.resize(size, BILINEAR), enhancing/dataloader/imagenet.py:31,49) for a batch
 * of decoded 8-bit RGB images of ragged sizes, bit-exact with Pillow's antialiased separable resampler (horizontal pass, then vertical, 22-bit fixed-point
 * weights).  src [B][HS][WS][3] / dst [B][HD][WD][3]: image b occupies the top-left corner of its slot.  meta [B][10] int32 per image:
 * {h_in, w_in, h_out, w_out, hb_off, hk_off, hks, vb_off, vk_off, vks}: the horizontal pass reads bounds[hb_off + 2x] = (first input column, taps) and
 * weights[hk_off + x*hks + tap]; the vertical pass likewise (tables: enhancing/dataloader/resize.py, Pillow's precompute_coeffs / normalize_coeffs_8bpc).
 * workspace: enh_resize_u8_workspace_bytes(B, HS, WD) bytes (the horizontal pass's uint8 result). */
size_t enh_resize_u8_workspace_bytes(int B, int HS, int WD);
int enh_resize_u8(const uint8_t* src, int B, int HS, int WS, const int* meta, const int* bounds, const int* weights, uint8_t* dst, int HD, int WD,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * StyleGAN2-discriminator native ops ("next" row) — drop-ins for the reference's two pybind ops
 * ------------------------------------------------------------------------------------------------ */
/* fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale) — enhancing/losses/op/fused_bias_act.cpp:17-31.
 * y = lrelu(x + bias[(i / step_b) % size_b]) * scale (grad = 0) or (x + bias) * (ref > 0 ? 1 : alpha) * scale (grad = 1: first and
 * second derivative, gated by the saved output).  f32, contiguous; bias / ref may be NULL; only act = 3 (leaky-relu) is used. */
int enh_fused_bias_act(const float* x, const float* bias, const float* ref, float* y, int64_t n, int64_t step_b, int size_b,
                       int act, int grad, float alpha, float scale, void* stream);
/* out[c] (+)= sum_{b,i} x[b,c,i] : the bias gradient `grad_input.sum(dim)` of fused_act.py:37-41 */
int enh_channel_sum_f32(const float* x, int B, int C, int64_t inner, float* out, int accumulate, void* stream);
/* upfirdn2d_op.upfirdn2d(input [major,in_h,in_w,1], kernel [kh,kw], up, down, pads) — enhancing/losses/op/upfirdn2d.cpp:17-30;
 * out [major, out_h, out_w], out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y (same for w).  f32; pads >= 0. */
int enh_upfirdn2d(const float* in, const float* kernel, float* out, int64_t major, int in_h, int in_w, int kh, int kw, int up_x,
                  int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* Equalised-lr convolution lowering (EqualConv2d, enhancing/losses/layers.py:163-185: conv2d(x, weight*scale, stride, padding),
 * k in {1,3}, stride in {1,2}) onto enh_gemm_h16 / enh_gemm_f32:  cols[(b,ho,wo), c*k*k + kh*k + kw] = x[b,c,ho*stride-pad+kh,wo*stride-pad+kw]
 * (zero outside the image) in `dtype` (ENH_DT_BF16 / ENH_DT_F16: 16-bit MFMA operands; ENH_DT_F32: the exact-f32 instrument), row stride ld = C*k*k
 * rounded up to a multiple of 8 with the pad columns zeroed.  The image is addressed as x[b*stride_b + c*stride_c + h*W + w], so [B,C,H,W] and
 * channel-major [C,B,H,W] activations are both accepted.  enh_col2im is the adjoint (the convolution's input gradient given dcols = dy^T . W, in
 * `dtype`): dx (f32) is overwritten, no atomics. */
int enh_im2col(const float* x, int64_t stride_b, int64_t stride_c, int B, int C, int H, int W, int k, int stride, int pad,
               int Ho, int Wo, void* cols, int64_t ld, int dtype, void* stream);
int enh_col2im(const void* dcols, int64_t ld, int B, int C, int H, int W, int k, int stride, int pad, int Ho, int Wo,
               float* dx, int64_t stride_b, int64_t stride_c, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolutions on channels-last bf16 activations [B,H,W,C] (no im2col tensor): EqualConv2d forward, input gradient and
 * weight gradient of the StyleGAN2 discriminator (enhancing/losses/layers.py:163-185; the three roles conv2d_gradfix differentiates
 * through, enhancing/losses/op/conv2d_gradfix.py:81-195) and the 3x3 convolutions of the LPIPS VGG16 trunk.
 * ------------------------------------------------------------------------------------------------ */
/* One description for every role.  GEMM row m = (b, y, x) of a logical grid Hm x Wm; contraction index = (tap (jy, jx), channel c);
 * operand element = src[b, y*gs + oy0 + jy*sty, x*gs + ox0 + jx*stx, c] (zero outside the source); the result row goes to pixel
 * (y*os + oph, x*os + opw) of the output tensor [B,HO,WO,N].
 *   forward  (stride s, padding p, k x k): src = x,  gs = s, oy0 = ox0 = -p, sty = stx = +1, nty = ntx = k, (Hm,Wm) = (HO,WO) = output size, os = 1
 *   dgrad, s = 1:  src = dy, gs = 1, oy0 = ox0 = +p, sty = stx = -1, nty = ntx = k, (Hm,Wm) = (HO,WO) = input size, weights packed transposed
 *   dgrad, s = 2:  one launch per output parity class (ph, pw): taps kh = kh0 + 2 jy with kh0 = (ph + p) & 1, oy0 = (ph + p - kh0) / 2, sty = -1,
 *                  Hm = (H - ph + 1) / 2, os = 2, oph = ph (same in x); a class without taps (nty*ntx = 0) writes zeros
 *   wgrad:         src = x, (Hm,Wm) = dy's spatial size, gs / oy0 / sty / nty as in forward, N = channels of dy (output fields unused) */
typedef struct enh_conv_geom {
  int B;
  int Hs, Ws, C;               /* source tensor [B,Hs,Ws,C], C % 8 == 0 */
  int Hm, Wm;                  /* logical grid enumerated as GEMM rows */
  int gs, oy0, ox0, nty, ntx, sty, stx;
  int N;                       /* output channels, N % 8 == 0 */
  int HO, WO, os, oph, opw;    /* output tensor and the placement of the logical grid in it */
} enh_conv_geom;
/* out[o, n] = epilogue( sum_{tap,c} src[...] * wt[n][tap*C + c] ), wt [N][nty*ntx*C] bf16 (enh_conv_pack_weight), o = output pixel of the row
 *   mode 0: relu(acc + bias[n])                     mode 1: (acc + add[o,n]) * (aux[o,n] > 0)   (add optional)      mode 2: acc
 *   mode 3: lrelu(acc + bias[n], slope p0) * p1     (EqualConv2d + FusedLeakyReLU, layers.py:220-264 / fused_act.py:48-76; bias optional)
 *   mode 4: acc + p0 * add[o,n]                     (StyleBlock's (out + skip) / sqrt(2), layers.py:262, folded into the skip convolution) */
int enh_conv_nhwc_h16(const enh_h16* src, const enh_h16* wt, const enh_conv_geom* g, int mode, const float* bias, const enh_h16* aux,
                      const enh_h16* add, float p0, float p1, enh_h16* out, int dtype, void* stream);
/* The same with a caller-provided workspace of enh_conv_workspace_bytes(g) bytes (0 = none needed): grids of less than half a round of workgroups
 * (the <= 16^2 layers at 16 images) are then split over the contraction — f32 partial slabs, added in ascending order by a second kernel that
 * applies the epilogue (deterministic).  ws == NULL or too small: not split. */
size_t enh_conv_workspace_bytes(const enh_conv_geom* g);
int enh_conv_nhwc_h16_ws(const enh_h16* src, const enh_h16* wt, const enh_conv_geom* g, int mode, const float* bias, const enh_h16* aux,
                         const enh_h16* add, float p0, float p1, enh_h16* out, void* ws, size_t ws_bytes, int dtype, void* stream);
/* kernel choice of enh_conv_nhwc_h16 / enh_conv_wgrad_nhwc_h16 for A/B measurements (explicit library state, like enh_gemm_set_kernel):
 * 0 = per shape (256-row tiles when C % 64 == 0, N % 128 == 0, at least four K stages and one tile per CU; else the 128 x 128 LDS-DMA kernel when
 * C % 64 == 0; else register-staged), 1 = register-staged everywhere, 2 = never the 256-row kernels (the round-2 choice), 3 = the 256-row kernels
 * wherever the shape allows them, however few tiles */
int enh_conv_set_kernel(int variant);
/* dw[n][tap*C + c] = sum over pixels (b,y,x) of dy[b,y,x,n] * src[b, y*gs + oy0 + jy*sty, x*gs + ox0 + jx*stx, c]   (f32, overwritten).
 * The pixel axis is split over the grid; partial slabs go to `ws` (enh_conv_wgrad_workspace_bytes) and are added in a fixed order. */
size_t enh_conv_wgrad_workspace_bytes(const enh_conv_geom* g);
int enh_conv_wgrad_nhwc_h16(const enh_h16* src, const enh_h16* dy, const enh_conv_geom* g, float* dw, void* ws, size_t ws_bytes, int dtype, void* stream);
/* parameter layout [Cout][Cin][k][k] f32 (x scale) -> packed bf16 operand, taps (kh0 + jy*kstep, kw0 + jx*kstep):
 *   transposed = 0: out[co][(jy*ntx+jx)*cols_padded + ci]  (forward)      transposed = 1: out[ci][(jy*ntx+jx)*cols_padded + co]  (input gradient)
 * rows / columns beyond the real channel counts are zero.  enh_conv_unpack_wgrad: dw[co][ci][kh][kw] = scale * dwp[co][(kh*k+kw)*cin_padded + ci] */
int enh_conv_pack_weight(const float* w, int Cout, int Cin, int k, float scale, int transposed, int kh0, int kw0, int kstep, int nty, int ntx,
                         int rows_padded, int cols_padded, enh_h16* out, int dtype, void* stream);
int enh_conv_unpack_wgrad(const float* dwp, int Cout, int Cin, int cin_padded, int k, float scale, float* dw, void* stream);
/* Blur (layers.py:140-160 -> upfirdn2d with unit up / down): out[b,oy,ox,c] = sum_{i,j} w(i,j) x[b, oy+i-pad_y0, ox+j-pad_x0, c] with
 * w(i,j) = kernel[kh-1-i][kw-1-j] (flip = 0, upfirdn2d's convention) or kernel[i][j] (flip = 1, the adjoint); out is [B, H+pad_y0+pad_y1-kh+1, W+..., C];
 * pads may be negative (crop) */
/* kernel choice of enh_blur_nhwc_h16 (explicit library state): 0 = per shape (4 x 4 filters: the row-marching kernel, bit-identical results),
 * 1 = the one-row kernel everywhere */
int enh_blur_set_kernel(int variant);
int enh_blur_nhwc_h16(const enh_h16* x, const float* kernel, int B, int H, int W, int C, int kh, int kw, int pad_y0, int pad_y1, int pad_x0,
                      int pad_x1, int flip, enh_h16* out, int dtype, void* stream);
/* y = g * (ref > 0 ? 1 : slope) * scale — the first / second derivative of FusedLeakyReLU through its saved output (fused_act.py:21-45);
 * ref == NULL: y = g * scale.  n % 8 == 0 */
int enh_lrelu_gate_h16(const enh_h16* g, const enh_h16* ref, int64_t n, float slope, float scale, enh_h16* y, int dtype, void* stream);
/* Minibatch standard deviation (layers.py:358-367, stddev_feat = 1) fused with the concatenation and the channel padding of the final convolution's input:
 * x [B,HW,C] bf16 -> out [B,HW,Cp] bf16 with out[..,0..C-1] = x, out[..,C] = mean over (h,w,c) of sqrt(var over the group + 1e-8) of the sample's slot
 * (sample b is in slot b % (B/group); biased variance), out[..,C+1..] = 0.  Backward: dx [B,HW,C] from g [B,HW,Cp].  B % group == 0, C % 8 == 0, Cp % 8 == 0, Cp > C. */
int enh_minibatch_stddev_nhwc(const enh_h16* x, int B, int HW, int C, int Cp, int group, enh_h16* out, int dtype, void* stream);
int enh_minibatch_stddev_nhwc_backward(const enh_h16* x, const enh_h16* g, int B, int HW, int C, int Cp, int group, enh_h16* dx, int dtype, void* stream);
/* img [B,C,H,W] f32, C <= 8  ->  [B,H,W,8] bf16 (channels C..7 zero), and the adjoint (padding channels dropped) */
int enh_img_to_nhwc8(const float* img, int B, int C, int H, int W, enh_h16* out, int dtype, void* stream);
int enh_nhwc8_to_img(const enh_h16* src, int B, int C, int H, int W, float* img, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 "exact mode": the same contractions with fp32 operands and fixed ascending-k fp32 accumulation (no bf16 anywhere), for end-to-end
 * parity runs against the fp32 CPU oracle (SURVEY.md §8d metric 3).  Same argument meaning as the bf16 entries above; all tensors f32.
 * ------------------------------------------------------------------------------------------------ */
int enh_gemm_f32(const float* A, int64_t lda, int trans_a, const float* B, int64_t ldb, int trans_b, int64_t M, int64_t N, int64_t K,
                 const float* bias, int act, const float* aux, int64_t ldaux, const float* res, int64_t ldres, int64_t res_rows,
                 int accumulate, float* C, int64_t ldc, void* stream);
int enh_attention_forward_f32(const float* qkv, int B, int N, int H, float scale, float* out, float* lse, void* stream);
int enh_attention_backward_f32(const float* qkv, const float* out, const float* dout, const float* lse, int B, int N, int H, float scale,
                               float* dqkv, float* delta_ws, void* stream);
/* the same with dim_head = D in {32, 64, 96, 128} (else ENH_E_SHAPE): the layouts of enh_attention_forward_dh in f32; D = 64 is the kernel above */
int enh_attention_forward_f32_dh(const float* qkv, int B, int N, int H, int D, float scale, float* out, float* lse, void* stream);
int enh_attention_backward_f32_dh(const float* qkv, const float* out, const float* dout, const float* lse, int B, int N, int H, int D, float scale,
                                  float* dqkv, float* delta_ws, void* stream);
int enh_colsum_f32(const float* x, int64_t M, int64_t N, int64_t ldx, float* out, int accumulate, void* stream);
/* to_patches = 1: img [B,C,H,W] -> patches [M, C*p*p] ; 0: the inverse scatter */
int enh_patch_perm_f32(const float* src, float* dst, int B, int C, int H, int W, int p, int to_patches, void* stream);
int enh_unpatchify_loss_f32(const float* pix, const float* target, int B, int C, int H, int W, int p, float w_l1, float w_l2, float* xrec,
                            double* sums, float* dpix, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS perceptual term (lpips 0.1.4, net = "vgg": pinned third-party dependency of the reference, requirements.txt:2; call sites
 * enhancing/losses/vqperceptual.py:29,43,74,115).  Activations are channels-last bf16 [B,H,W,C].
 * ------------------------------------------------------------------------------------------------ */
/* 3x3 convolution, stride 1, zero padding 1, as an implicit GEMM (no im2col tensor).  x [B,H,W,Cin], wt [Cout][9*Cin] tap-major
 * (wt[co][(kh*3+kw)*Cin + ci] = weight[co][ci][kh][kw]), out [B,H,W,Cout]; Cin, Cout multiples of 8.
 *   mode 0: out = relu(acc + bias[co])                            (torchvision vgg16.features conv + ReLU)
 *   mode 1: out = (acc + add[m,co]) * (aux[m,co] > 0)             (input gradient: wt = flipped / transposed weights, aux = the saved post-ReLU
 *                                                                  activation this gradient is for, add = optional extra gradient at that activation)
 *   mode 2: out = acc                                             (input gradient in front of a max-pool) */
int enh_conv3x3_nhwc_h16(const enh_h16* x, const enh_h16* wt, int B, int H, int W, int Cin, int Cout, const float* bias, int mode,
                         const enh_h16* aux, const enh_h16* add, enh_h16* out, int dtype, void* stream);
/* ScalingLayer + first convolution: img [B,3,H,W] f32 -> relu(conv3x3(((a img + b) - shift) / scale, w [64,3,3,3]) + bias) as [B,H,W,64] bf16, with
 * (a, b) = (2, -1) if normalize (images in [0,1]: lpips' normalize=True, = the inputs*2-1 of vqperceptual.py:43) else (1, 0); lpips ScalingLayer: shift
 * (-.030,-.088,-.188), scale (.458,.448,.450) ; and its gradient w.r.t. img given the gradient at the convolution output before the ReLU */
int enh_vgg_conv1(const float* img, const float* w, const float* bias, const float* shift, const float* scale, int normalize, int B, int H, int W, enh_h16* out, int dtype, void* stream);
int enh_vgg_conv1_backward(const enh_h16* gpre, const float* w, const float* scale, int normalize, int B, int H, int W, float* dimg, int dtype, void* stream);
/* 2x2 / stride-2 max-pool ; backward gx = (x > 0) * (gy routed to the first maximum of each window + add)  (add optional) */
int enh_maxpool2_nhwc_h16(const enh_h16* x, int B, int H, int W, int C, enh_h16* y, int dtype, void* stream);
int enh_maxpool2_nhwc_h16_backward(const enh_h16* x, const enh_h16* gy, const enh_h16* add, int B, int H, int W, int C, enh_h16* gx, int dtype, void* stream);
/* LPIPS head of one slice: feat [2B,h,w,C] (images 0..B-1 = references, B..2B-1 = reconstructions), lin [C] = the slice's 1x1 "lin" weights;
 * out[b] (+)= mean over pixels of sum_c lin[c] (f0/(|f0|+1e-10) - f1/(|f1|+1e-10))_c^2 ; val_ws [B*h*w] f32 scratch (deterministic two-stage sum).
 * Backward: gradient w.r.t. the reconstruction features only, dfeat1 [B,h,w,C] bf16, given gout[B] */
int enh_lpips_head(const enh_h16* feat, const float* lin, int B, int64_t HW, int C, float* val_ws, float* out, int accumulate, int dtype, void* stream);
int enh_lpips_head_backward(const enh_h16* feat, const float* lin, const float* gout, int B, int64_t HW, int C, enh_h16* dfeat1, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling: the decode-shaped kernels behind GPT.sample / sample_step with one condition token
 * (enhancing/modules/stage2/layers.py:57-97,213-303).  Every step is one token per batch row: M = batch <= 64 rows.
 * No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* y[M,N] = act(x[M,K] W[N,K]^T + bias[N]) (+ res[M,N]): W in nn.Linear layout, streamed exactly once; 1 <= M <= 64 (else ENH_E_SHAPE),
 * K % 8 == 0, N % 8 == 0; act 0 = none, 1 = square(relu(.)) (FFN.forward, layers.py:108); bias / res optional f32; the result goes to out_f32
 * and / or out_h16.  Rows of the padded MFMA tile beyond M or N are never read from memory.  Work is split over N (16 rows of W per
 * workgroup) and, where that leaves the chip idle, over K: slabs in `workspace`, added in ascending order by a second pass. */
size_t enh_skinny_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int enh_skinny_gemm_h16(const enh_h16* x, const enh_h16* W, int64_t M, int64_t N, int64_t K, const float* bias, int act, const float* res,
                        float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* One new token per (batch, head).  qkv [B, 3C] = the step's q | k | v (C = H hs), k_cache / v_cache [B, H, Tmax, hs], all in the format of
 * dtype: ENH_DT_BF16 / ENH_DT_F16, or ENH_DT_F32 (the exact mode).  Writes k and v into slot t and
 * out[B, C] = softmax(q K[0..t]^T / sqrt(hs)) V[0..t] (layers.py:64-89, the (B nh, T, hs) views).  Slots > t are neither read nor written.
 * hs: a multiple of 64 up to 384; Tmax <= 8192; 0 <= t < Tmax.  The cache length is cut into pieces of <= 256 slots across workgroups; their
 * partial results meet in `workspace` and are merged in ascending order. */
size_t enh_decode_attention_workspace_bytes(int B, int H, int hs, int Tmax);
int enh_decode_attention(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, int t, void* out, void* workspace,
                         size_t workspace_bytes, int dtype, void* stream);
/* What enh_ln_timeshift (below) computes at S = 1, for a decode step's M <= 64 rows, in a kernel of its own whose statistics may differ from that
 * one's by an ulp: LayerNorm (biased variance, f32 statistics), D % 8 == 0, D <= 8192, times colscale[D] when given (time_mix, layers.py:60 at
 * T == 1: no shifted term); out_f32 and / or out_h16.  csrc/gpt_rows.hip, as enh_gpt_embed. */
int enh_row_ln_scale(const float* x, const float* w, const float* b, const float* colscale, int M, int D, float eps, float* out_f32,
                     enh_h16* out_h16, int dtype, void* stream);
/* out[b] = table[ids[b * id_stride]] + pos_row, b < B; table [V, C] f32, pos_row [C] f32, C % 4 == 0 (layers.py:280-281,290-291) */
int enh_gpt_embed(const float* table, const int64_t* ids, int64_t id_stride, const float* pos_row, int B, int C, int V, float* out, void* stream);
/* The exact mode's form of enh_skinny_gemm_h16: f32 operands and result on the vector ALU, every dot product summed as 64 lane partials of K / 64
 * terms and a 6-level tree (enh_gemm_f32 adds the K terms in ascending order, which at K = 3072 is four times the fp32 reference's own error).
 * A parity instrument, not a fast path: W is re-read once per eight rows of x. */
int enh_skinny_gemm_f32(const float* x, const float* W, int64_t M, int64_t N, int64_t K, const float* bias, int act, const float* res, float* out,
                        void* stream);
/* GPT.sample lines 233-258 for B rows of V <= 16384 f32 logits, one workgroup per row: x = logits / temperature; top_k > 0: every x below the
 * k-th largest becomes -inf (ties with it stay); p = softmax(x); top_p >= 0: an entry is dropped when the probabilities strictly larger than
 * it sum to >= top_p (the largest always stays; entries of EQUAL probability stay or go together, where the reference's sort breaks such a
 * tie by position), then p is renormalised; the code is the first index whose running sum of p exceeds u * sum(p).  u = uniforms[row] when
 * given, else 23 bits of Philox4x32-10 (u = (x >> 9) 2^-23 + 2^-24, never 0 or 1) at key = seed, counter = (row0 + row, step, call): a pure function of those, the distribution of
 * torch.multinomial, not its bits.  top_k <= 0 / top_p < 0: off.
 * codes[row * code_stride] = the code; optional outputs: logits_out[row * logits_out_stride + v] = x after top-k (what the reference
 * returns), mask_out [B, V] (1 = kept), probs_out [B, V] (the renormalised p). */
int enh_sample_logits(const float* logits, int B, int V, float temperature, int top_k, float top_p, const float* uniforms, uint64_t seed,
                      uint32_t call, uint32_t step, int64_t row0, int64_t* codes, int64_t code_stride, float* logits_out,
                      int64_t logits_out_stride, uint8_t* mask_out, float* probs_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling with MXFP8 weights (csrc/gpt_decode_w8.hip): the weight-only 8-bit form of a decode step's products.
 * The operand format, fixed: a weight W [N, K] in nn.Linear layout, K % 32 == 0, is two row-major arrays,
 *   codes  [N, K]      uint8: OCP e4m3fn (bias 7, largest finite 448 = 0x7e, 0x7f / 0xff NaN; not the fnuz form),
 *   scales [N, K / 32] uint8: E8M0, byte s = 2^(s - 127), one per 32 consecutive k of a row,
 * and W[n, k] = e4m3(codes[n, k]) 2^(scales[n, k / 32] - 127).  Per block of 32 (OCP Microscaling Formats v1.0): amax = max |w|,
 * X = clamp(floor(log2 amax) - 8, -127, 127) (X = 0 when amax == 0), code = e4m3fn(RNE(w 2^-X)) saturated to +-448: values in (448, 512)
 * saturate and finite input never gives a NaN code.  Non-finite input: a block that holds an infinity or a NaN gets X = 120 (scale byte 247);
 * an infinity becomes +-448, a NaN the NaN code 0x7f with its sign, and the block's finite values are coded at that scale.
 * No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* Rows [0, N) of w (f32, K values each, w_row_stride elements apart; rows 16-byte aligned) become rows code_row0 .. code_row0 + N - 1 of `codes`
 * (row pitch K) and rows scale_row0 .. of `scales` (row pitch K / 32): q, k and v quantized one after another at row offsets 0, C and 2C are
 * the fused [3C, C] operand.  One pass over w; nothing outside those rows is written. */
int enh_mxfp8_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                       int64_t scale_row0, void* stream);
/* enh_skinny_gemm_h16 with W given as (codes, scales): y[M,N] = act(x[M,K] W^T + bias[N]) (+ res[M,N]), x in the 16-bit format of dtype,
 * 1 <= M <= 64, N % 8 == 0, K % 32 == 0 (else ENH_E_SHAPE); the same epilogue, outputs, K slabs and workspace (enh_skinny_gemm_workspace_bytes).
 * The codes are widened to the operand format exactly, every 32-wide block is one MFMA step whose f32 result is multiplied by the block's power of
 * two as it is added to the f32 sum: the scale costs no accuracy.  The codes and scales are read exactly once. */
int enh_skinny_gemm_w8(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias, int act,
                       const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling with MXFP4 weights (csrc/gpt_decode_w4.hip): the weight-only 4-bit form of a decode step's products.
 * The operand format, fixed: a weight W [N, K] in nn.Linear layout, K % 32 == 0, is two row-major arrays,
 *   codes  [N, K / 2]  uint8: two OCP e2m1 codes per byte, k even in the low nibble and k odd in the high nibble.  A nibble is sign, 2 exponent
 *                             bits (bias 1), 1 mantissa bit: codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN and no infinity,
 *   scales [N, K / 32] uint8: E8M0 as for MXFP8, byte s = 2^(s - 127), one per 32 consecutive k of a row; 0xff is the format's NaN,
 * and W[n, k] = e2m1(code[n, k]) 2^(scales[n, k / 32] - 127).  Per block of 32 (OCP Microscaling Formats v1.0): amax = max |w|,
 * X = clamp(floor(log2 amax) - 2, -127, 127) (X = 0 when amax == 0), code = RNE(w 2^-X) on the eight-value grid, ties to the even code
 * (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturated to +-6: values in (6, 8) saturate; -0.0 keeps its sign.
 * Non-finite input: a block that holds an infinity or a NaN gets the scale byte 0xff and all-zero codes, so the whole block dequantizes to NaN,
 * and the product gives NaN for every row of W that holds such a block.
 * No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* enh_mxfp8_quantize for this format: rows [0, N) of w become rows code_row0 .. of `codes` (row pitch K / 2 bytes, 4-byte aligned) and rows
 * scale_row0 .. of `scales` (row pitch K / 32).  One pass over w; nothing outside those rows is written. */
int enh_mxfp4_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                       int64_t scale_row0, void* stream);
/* enh_skinny_gemm_w8's contract with W in this format: 1 <= M <= 64, N % 8 == 0, K % 32 == 0 (else ENH_E_SHAPE), the same epilogue and outputs,
 * exact widening, one MFMA step per 32-wide block scaled in f32, codes and scales read exactly once.  Its slabs hold at least two K chunks per
 * wave, so its slab plan and workspace are its own: enh_skinny_gemm_w4_workspace_bytes (0 when no workspace is needed). */
size_t enh_skinny_gemm_w4_workspace_bytes(int64_t M, int64_t N, int64_t K);
int enh_skinny_gemm_w4(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias, int act,
                       const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling with MXFP6 weights (csrc/gpt_decode_w6.hip): the weight-only 6-bit form of a decode step's products.
 * The operand format, fixed: a weight W [N, K] in nn.Linear layout, K % 32 == 0, is two row-major arrays,
 *   codes  [N, 96 ceil(K / 128)] uint8: OCP FP6 E2M3 codes, six bits each: sign, 2 exponent bits (bias 1), 3 mantissa bits, code s << 5 | e << 3 | m,
 *                             magnitude m / 8 for e = 0 and 2^(e - 1) (1 + m / 8) for e = 1 .. 3; the largest value is 7.5; no NaN and no infinity.
 *                             A row is a sequence of 128-k chunks of 96 bytes; a last chunk that is only partly inside K is stored whole and the
 *                             codes of k >= K are 0.  Within chunk c, piece q = 0 .. 3 is a 192-bit little-endian integer whose bits 0 .. 127 are
 *                             the chunk's bytes [16 q, 16 q + 16) and whose bits 128 .. 191 are its bytes [64 + 8 q, 64 + 8 q + 8).  Position
 *                             j = 8 i + e of a piece (i = 0 .. 3, e = 0 .. 7) is bits [6 j, 6 j + 6) and holds the code of k = 128 c + 32 i + 8 q + e:
 *                             position order is the element order of v_cvt_scalef32_pk32_{f16,bf16}_fp6, element 0 in the lowest bits, so a lane's
 *                             two loads and one conversion are the four MFMA operands of a chunk as they stand,
 *   scales [N, K / 32] uint8: E8M0 as for MXFP8, byte s = 2^(s - 127), one per 32 consecutive k of a row in natural order; 0xff is the format's NaN,
 * and W[n, k] = e2m3(code[n, k]) 2^(scales[n, k / 32] - 127).  Per block of 32 (OCP Microscaling Formats v1.0): amax = max |w|,
 * X = clamp(floor(log2 amax) - 2, -127, 127) (X = 0 when amax == 0), code = RNE(w 2^-X) on the 32-value grid, ties to the even code, saturated
 * to +-7.5: values in (7.5, 8) saturate, the tie 7.75 too; -0.0 keeps its sign.
 * Non-finite input: a block that holds an infinity or a NaN gets the scale byte 0xff and all-zero codes, so the whole block dequantizes to NaN,
 * and the product gives NaN for every row of W that holds such a block.
 * No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* enh_mxfp4_quantize for this format: rows [0, N) of w become rows code_row0 .. of `codes` (row pitch 96 ceil(K / 128) bytes, 16-byte aligned) and
 * rows scale_row0 .. of `scales` (row pitch K / 32).  One pass over w; a partial last chunk is written whole, zero past K; nothing outside those
 * rows is written. */
int enh_mxfp6_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                       int64_t scale_row0, void* stream);
/* enh_skinny_gemm_w4's contract with W in this format: 1 <= M <= 64, N % 8 == 0, K % 32 == 0 (else ENH_E_SHAPE), the same epilogue and outputs,
 * exact widening (one conversion per lane and chunk, no lane swaps), one MFMA step per 32-wide block scaled in f32, codes and scales read exactly
 * once.  Its slab plan and workspace are its own: enh_skinny_gemm_w6_workspace_bytes (0 when no workspace is needed). */
size_t enh_skinny_gemm_w6_workspace_bytes(int64_t M, int64_t N, int64_t K);
int enh_skinny_gemm_w6(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias, int act,
                       const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling with an MXFP8 k / v cache (csrc/gpt_decode_kv8.hip): enh_decode_attention over caches held in the operand format above, with
 * the blocks of 32 running along the head dimension.  The cache layout, fixed: per layer four row-major uint8 tensors,
 *   k_codes, v_codes   [B, H, Tmax, hs]       e4m3fn codes,
 *   k_scales, v_scales [B, H, Tmax, hs / 32]  E8M0, one per 32 consecutive elements of a head row,
 * 1 + 1/32 bytes per element instead of 2, and K[b, h, j, d] = e4m3(k_codes[b, h, j, d]) 2^(k_scales[b, h, j, d / 32] - 127).
 * The step's k and v rows (the 16-bit values of qkv, widened to f32) are quantized with enh_mxfp8_quantize's rounding and appended at slot t, and the
 * step's own attention reads slot t through those quantized values: out = softmax(q K[0..t]^T / sqrt(hs)) V[0..t] over the dequantized cache as
 * stored, so a slot contributes the same k / v to every step that reads it (enh_decode_attention takes slot t unquantized from qkv).  q stays
 * 16-bit; scores, softmax and P V accumulate in f32; dequantization is exact.  Slots > t are neither read nor written.
 * No float atomics; the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* qkv [B, 3C] and out [B, C] in the 16-bit format of dtype (ENH_DT_BF16 | ENH_DT_F16 only); hs a multiple of 64 up to 384, Tmax <= 8192,
 * 0 <= t < Tmax; qkv and the code tensors 16-byte aligned.  The pieces, the workspace (enh_decode_attention_workspace_bytes) and the ascending merge
 * are enh_decode_attention's. */
int enh_decode_attention_kv8(const void* qkv, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, int B, int H, int hs, int Tmax,
                             int t, void* out, void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* the cursor form (see enh_decode_attention_at below): t = *cursor + t_offset read on the device, the same bits at the same t; the workspace is
 * always required; t outside [0, Tmax): nothing is read or written. */
int enh_decode_attention_kv8_at(const void* qkv, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, int B, int H, int hs,
                                int Tmax, const int* cursor, int t_offset, void* out, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling, the prefill of given codes (csrc/gpt_prefill_cache.hip; sample(prefix_codes=)): the k / v rows of whole sequences put into
 * the caches of the decode attentions above in one launch.  qkv is the packed [B S, 3 H hs] output of the fused q | k | v product, the layout
 * enh_causal_attention_forward reads; row (b, s) goes to slot slot0 + s of batch element b.  hs a multiple of 64 up to 384, slot0 >= 0,
 * slot0 + S <= Tmax (else ENH_E_SHAPE); qkv and the caches 16-byte aligned; offsets are 64-bit.  Slots outside [slot0, slot0 + S) are not touched.
 * 16-byte loads and stores, no atomics, no workspace.
 * ------------------------------------------------------------------------------------------------ */
/* k_cache / v_cache [B, H, Tmax, hs] and qkv in the format of dtype (ENH_DT_BF16 | ENH_DT_F16 | ENH_DT_F32: the exact mode): a bit-for-bit copy of
 * the k and v columns, what S successive enh_decode_attention calls at t = slot0 .. slot0 + S - 1 append. */
int enh_kv_cache_fill(const void* qkv, int B, int S, int H, int hs, int Tmax, int slot0, void* k_cache, void* v_cache, int dtype, void* stream);
/* The MXFP8 cache of enh_decode_attention_kv8 (codes [B, H, Tmax, hs], scales [B, H, Tmax, hs / 32]); qkv in the 16-bit format of dtype
 * (ENH_DT_BF16 | ENH_DT_F16).  Every head row is quantized as that entry's append quantizes it (blocks of 32 along hs, the rounding of
 * enh_mxfp8_quantize), with one difference: a block that holds an infinity or a NaN gets the scale byte 0xff, E8M0's NaN (the append gives 247);
 * its codes are those of X = 120.  The DEQUANTIZED values e4m3(code) 2^(scale - 127) are written back over the k and v columns of qkv in the
 * operand format (the q columns are not touched), so that an attention over qkv reads what every later step reads from the slot.  The write-back
 * is exact in bf16.  In fp16 it is exact whenever the block's amax is >= 2^-7: below that the smallest codes (2^-9 2^X) fall under fp16's
 * subnormal step 2^-24 and are rounded to it (to nearest even); the cache itself, which is what later steps read, is not affected. */
int enh_kv_cache_fill_kv8(void* qkv, int B, int S, int H, int hs, int Tmax, int slot0, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes,
                          uint8_t* v_scales, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 GPT, teacher-forced forward (csrc/gpt_prefill.hip: the attention, csrc/gpt_rows.hip: the row kernels; reference enhancing/modules/stage2/layers.py:57-97,132-136,193-211 with
 * cond_num_tokens == 1).  M = B S token rows at once: the wide products are enh_gemm_h16's (exact mode: enh_skinny_gemm_f32 in 64-row pieces),
 * these are the kernels between them.  No float atomics: the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* Causal softmax attention, out[b, n, h] = softmax_{j <= n}(q_n . k_j * scale) V: qkv packed [B, N, 3 H D] (enh_attention_forward_dh's layout),
 * out [B, N, H D], lse [B, H, N] f32 or NULL.  D a multiple of 64 up to 384 (else ENH_E_SHAPE), any N >= 1.  Key tiles above the diagonal are
 * neither loaded nor computed; above D = 128 two workgroups share a query block, each owning half of V's width. */
int enh_causal_attention_forward(const enh_h16* qkv, int B, int N, int H, int D, float scale, enh_h16* out, float* lse, int dtype, void* stream);
/* the exact mode's form (f32 tensors, vector ALU, N <= 8192): a parity instrument */
int enh_causal_attention_forward_f32(const float* qkv, int B, int N, int H, int D, float scale, float* out, float* lse, void* stream);
/* LayerNorm (biased variance, f32 statistics) of M rows of width D (D % 8 == 0, D <= 8192), M a multiple of the sequence length S.  With
 * colscale = time_mix [D]: y[b, s] = ln(x[b, s]) tm + ln(x[b, s - 1]) (1 - tm), and y[b, 0] = ln(x[b, 0]) tm (layers.py:60,77: the shifted term of a
 * batch element's first row is zero).  colscale = NULL: the plain LayerNorm (ln2, the final norm).  out_f32 and / or out_h16. */
int enh_ln_timeshift(const float* x, const float* w, const float* b, const float* colscale, int64_t M, int S, int D, float eps, float* out_f32,
                     enh_h16* out_h16, int dtype, void* stream);
/* out [B, S, C] f32: row (b, 0) = tok_cond[conds[b]] + pos_cond, row (b, s) = tok_code[codes[b * code_stride + s - 1]] + pos_code[s - 1]
 * (layers.py:195-203 without the last code, whose row the causal mask keeps from every logit).  C % 4 == 0; ids outside a table are clamped. */
int enh_gpt_embed_seq(const int64_t* conds, const int64_t* codes, int64_t code_stride, const float* tok_cond, const float* pos_cond,
                      const float* tok_code, const float* pos_code, int B, int S, int C, int Vc, int V, float* out, void* stream);
/* y = square(relu(.)) over n % 8 == 0 elements (FFN, layers.py:134).  x != NULL: reads f32 x and writes y in `dtype` (one rounding: what
 * GPT.forward uses); x == NULL: in place on y.  dtype ENH_DT_BF16 | ENH_DT_F16 | ENH_DT_F32 (the exact mode: y is f32). */
int enh_relu_sq_h16(const float* x, void* y, int64_t n, int dtype, void* stream);
/* nll[m] = logsumexp(logits[m]) - logits[m][target[m]] for M rows of V <= 16384 f32 logits, one workgroup per row; mean != NULL: a second,
 * fixed-order pass writes mean[0] = sum(nll) / M.  enh_mean_f32 is that pass alone (the mean over several calls' rows). */
int enh_cross_entropy_rows(const float* logits, const int64_t* target, int64_t M, int V, float* nll, float* mean, void* stream);
int enh_mean_f32(const float* v, int64_t M, float* mean, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 RQTransformer, teacher-forced forward (csrc/rq_prefill.hip): what it needs beyond the GPT's kernels above.  No float atomics.
 * ------------------------------------------------------------------------------------------------ */
/* The embedding stage of B images of T positions with Dp codes each (2 <= Dp <= 8; codes [B, T, Dp] contiguous), one launch.
 * spatial [B, T, C] f32: row (b, 0) = tok_cond[conds[b]] + pos_cond, row (b, s) = sum_j tok_code[codes[b, s - 1, j]] + pos_code[s - 1] (S = T rows:
 * position T - 1 has none).  depth [B T, Dp, C] f32: slot d >= 1 of sequence b T + t = sum_{j < d} tok_code[codes[b, t, j]] + pos_depth[d - 1]; slot 0
 * is left alone (enh_ln_rows_strided writes it).  Sums in ascending depth, one rounding per addition.  C % 4 == 0; ids outside a table are clamped. */
int enh_rq_embed_seq(const int64_t* conds, const int64_t* codes, const float* tok_cond, const float* pos_cond, const float* tok_code,
                     const float* pos_code, const float* pos_depth, int B, int T, int Dp, int C, int Vc, int V, float* spatial, float* depth,
                     void* stream);
/* LayerNorm (biased variance, f32 statistics) of M contiguous rows of width D (D % 8 == 0, D <= 8192); row m of the f32 output starts at
 * out + m out_stride (out_stride >= D, a multiple of 4): ln_spatial written into slot 0 of every depth sequence. */
int enh_ln_rows_strided(const float* x, const float* w, const float* b, int64_t M, int D, float eps, float* out, int64_t out_stride, void* stream);
/* Causal softmax attention of NSEQ sequences of L tokens, 1 <= L <= 8: qkv packed [NSEQ, L, 3 H D], out [NSEQ, L, H D], lse [NSEQ, H, L] f32 or NULL;
 * D a multiple of 64 up to 384 (anything else: ENH_E_SHAPE).  The arithmetic contract of enh_causal_attention_forward (f32 scores, exp(s - max)
 * rounded to the format before P V, one rounding of out); eight lanes own a (sequence, head) pair and a workgroup 32 pairs, nothing staged in LDS. */
int enh_short_causal_attention_forward(const enh_h16* qkv, int NSEQ, int L, int H, int D, float scale, enh_h16* out, float* lse, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 RQTransformer, sampling (csrc/rq_decode.hip; layers.py:397-547 with one condition token): what the spatial / depth decode loop needs
 * beyond the GPT's decode kernels above.  No float atomics.
 * ------------------------------------------------------------------------------------------------ */
/* out[b] = (((e_0 + e_1) + ...) + e_{n-1}) + pos_row with e_j = table[ids[b * id_stride + j]], b < B, 1 <= n <= 8 (else ENH_E_SHAPE); table [V, C]
 * f32, pos_row [C] f32, C % 4 == 0.  ids: int64 on the device (a strided view of the sampler's [B, T, D] codes: id_stride >= n).  Sums in ascending
 * depth, one rounding per addition: the bits of enh_rq_embed_seq's row for the same codes (layers.py:502,535).  Ids outside the table are clamped. */
int enh_rq_embed_step(const float* table, const int64_t* ids, int64_t id_stride, int n, const float* pos_row, int B, int C, int V, float* out,
                      void* stream);
/* enh_decode_attention (its arguments, its arithmetic contract: f32 scores, f32 softmax numerators, slot t taken from qkv and appended, slots > t
 * neither read nor written) for a cache of Tmax <= 8 slots (else ENH_E_SHAPE): eight lanes own a (row, head) pair and a workgroup 32 pairs,
 * nothing staged in LDS, no workspace.  dtype ENH_DT_BF16 | ENH_DT_F16 | ENH_DT_F32; hs a multiple of 64 up to 384. */
int enh_short_decode_attention(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, int t, void* out, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 sampling, the cursor forms (csrc/gpt_decode.hip; the input row's body: csrc/embed_row.h).  The position t of the sampling loop is one int32 in device memory,
 * the cursor, and no argument of these entries depends on t: the launches of one position, captured once into a HIP graph, are replayed for every
 * later position.  Each entry runs the body of its by-value sibling above and gives its bits at the same t.  The cursor is read, never checked on
 * the host: a position outside an entry's range makes every workgroup return without reading or writing anything.
 * ------------------------------------------------------------------------------------------------ */
/* *cursor += 1 (one thread) */
int enh_cursor_advance(int* cursor, void* stream);
/* enh_decode_attention at t = *cursor + t_offset.  The split plan is worked out on the device from t + 1 by the host's function, the grid covers the
 * (Tmax + 63) / 64 pieces the longest plan can have (workgroups past the plan return), and the merge kernel is always launched (it returns under a
 * plan of one piece).  workspace: at least enh_decode_attention_workspace_bytes(B, H, hs, Tmax), always required.  t outside [0, Tmax): nothing is
 * read or written. */
int enh_decode_attention_at(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, const int* cursor, int t_offset, void* out,
                            void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* The input row of a step at t = *cursor: out[b] = (((e_0 + e_1) + ...) + e_{n-1}) + pos_base[t pos_t_stride + pos_offset .. + C) with
 * e_j = table[ids_base[b id_row_stride + t id_t_stride + id_offset + j]], b < B, 1 <= n <= 8: enh_rq_embed_step's bits, and at n == 1 enh_gpt_embed's.
 * Strides and offsets count elements; offsets may be negative (the codes of position t - 1) as long as positions t_lo and t_hi - 1 stay at or
 * behind the bases; pos_t_stride and pos_offset are multiples of 4.  t outside [t_lo, t_hi): nothing is read or written.  Ids outside the table
 * are clamped. */
int enh_embed_step_at(const float* table, const int64_t* ids_base, int64_t id_row_stride, int64_t id_t_stride, int64_t id_offset, int n,
                      const float* pos_base, int64_t pos_t_stride, int64_t pos_offset, const int* cursor, int t_lo, int t_hi, int B, int C, int V,
                      float* out, void* stream);
/* enh_sample_logits at step = *cursor * step_mul + step_add, with the Philox uniform of (seed, call, step, row0 + row): the code of row b goes to
 * codes_base[b code_row_stride + step] and, when logits_base is given, the filtered logits to logits_base[b logits_row_stride + step V .. + V).
 * step outside [0, n_steps): nothing is read or written (code_row_stride >= n_steps, logits_row_stride >= n_steps V). */
int enh_sample_logits_at(const float* logits, int B, int V, float temperature, int top_k, float top_p, uint64_t seed, uint32_t call, const int* cursor,
                         int step_mul, int step_add, int n_steps, int64_t row0, int64_t* codes_base, int64_t code_row_stride, float* logits_base,
                         int64_t logits_row_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 GPT, backward of the teacher-forced forward (csrc/gpt_attn_bwd.hip: the attention, csrc/gpt_rows.hip: the row kernels).  The gradient
 * products are enh_gemm_h16's (trans_a / trans_b / accumulate); these are the kernels between them.  No float atomics: the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
/* dqkv [B, N, 3 H D] (16-bit) of enh_causal_attention_forward from qkv, the out and lse it stored, and dout [B, N, H D].  D a multiple of 64 up to
 * 384, any N >= 1.  Flash-style: P is recomputed from lse, delta = rowsum(dout o out) goes through ws (enh_causal_attention_backward_workspace_bytes:
 * B H N floats).  Two kernels (dQ; dK and dV); tiles on the masked side of the diagonal are neither loaded nor computed; above D = 128 a workgroup
 * owns at most 128 output columns (dK / dV: 64 from D = 256).  Query 0 of every sequence sees one key: its dQ row and its dS are exact zeros. */
size_t enh_causal_attention_backward_workspace_bytes(int B, int N, int H);
int enh_causal_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N, int H, int D, float scale,
                                  enh_h16* dqkv, void* ws, size_t ws_bytes, int dtype, void* stream);
/* nll as enh_cross_entropy_rows (the same bits) and dlogits[m][v] = (softmax(logits[m])[v] - (v == target[m])) * gscale in the operand format,
 * from one read of the f32 logits.  V a multiple of 8 up to 16384.  gscale_dev (optional device float) multiplies gscale: the loss scale of an fp16
 * backward, kept on the device (enh_loss_scale_update); with NULL the kernel is the one without it, bit for bit. */
int enh_cross_entropy_backward(const float* logits, const int64_t* target, int64_t M, int V, float gscale, float* nll, enh_h16* dlogits, int dtype,
                               const float* gscale_dev, void* stream);
/* dx = dy * 2 relu(h) over n % 8 == 0 elements, with relu(h) = sqrt(y) taken from y = square(relu(h)) in the operand format (what enh_relu_sq_h16
 * wrote and the p1 product consumed: the hidden activation is kept once). */
int enh_relu_sq_backward(const float* dy, const enh_h16* y, enh_h16* dx, int64_t n, int dtype, void* stream);
/* Backward of enh_ln_timeshift: dy [M, D] f32, x the forward's input (row statistics are recomputed from it), w, b (needed with colscale), colscale or
 * NULL.  dx f32 = the gradient of x (+ dres when given), dx16 an optional copy in the operand format; dw, db and (with colscale) dcolscale [D] are
 * set, or added to under `accumulate`.  With colscale = tm the gradient reaching ln(x[b, s]) is dy[b, s] tm + dy[b, s + 1] (1 - tm), the second term
 * only for s + 1 < S.  The column sums go through row-block partials in ws (enh_ln_timeshift_backward_workspace_bytes) and a fixed-order pass. */
size_t enh_ln_timeshift_backward_workspace_bytes(int64_t M, int D);
int enh_ln_timeshift_backward(const float* dy, const float* x, const float* w, const float* b, const float* colscale, const float* dres, int64_t M, int S,
                              int D, float eps, float* dx, enh_h16* dx16, float* dw, float* db, float* dcolscale, int accumulate, void* ws, size_t ws_bytes,
                              int dtype, void* stream);
/* Backward of enh_gpt_embed_seq from g [B, S, C] f32: dtok_code [V, C] and dtok_cond [Vc, C] (row v = the sum, in ascending (b, s) order, of the rows
 * whose fed id is v; rows that do not occur are zero), dpos_code [P, C] (row p = sum_b g[b, p + 1] for p < S - 1, zero beyond) and dpos_cond [C].
 * Only codes 0 .. S - 2 of a sequence are fed.  accumulate != 0 adds to the four tables instead of setting them.  C % 4 == 0, C <= 8192. */
int enh_gpt_embed_seq_backward(const float* g, const int64_t* conds, const int64_t* codes, int64_t code_stride, int B, int S, int C, int Vc, int V, int P,
                               float* dtok_cond, float* dpos_cond, float* dtok_code, float* dpos_code, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage-2 RQTransformer, backward of the teacher-forced forward (csrc/rq_backward.hip; the strided LayerNorm backward shares its body with
 * enh_ln_timeshift_backward in csrc/gpt_rows.hip).  The Blocks of both stacks run the GPT's backward kernels above.  No float atomics.
 * ------------------------------------------------------------------------------------------------ */
/* dqkv [NSEQ, L, 3 H D] (16-bit) of enh_short_causal_attention_forward from qkv, the out and lse [NSEQ, H, L] it stored, and dout [NSEQ, L, H D];
 * 1 <= L <= 8, D a multiple of 64 up to 384.  The arithmetic contract of enh_causal_attention_backward (P from lse, delta on the stored out, P and
 * P o (dP - delta) rounded to the format before their products, one rounding of dq, dk, dv; row 0 of dQ exact zeros).  Eight lanes own a
 * (sequence, head) pair and write all of its dq, dk and dv: no workspace, nothing staged in LDS. */
int enh_short_causal_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int NSEQ, int L, int H, int D,
                                        float scale, enh_h16* dqkv, int dtype, void* stream);
/* Backward of enh_ln_rows_strided: row m of dy starts at dy + m dy_stride (dy_stride >= D, a multiple of 4; nothing between the rows is read), x [M, D]
 * contiguous.  dx f32 [M, D], dx16 an optional copy in the operand format; dw, db [D] set, or added to under `accumulate`.  The workspace is
 * enh_ln_timeshift_backward_workspace_bytes(M, D); the bits are those of enh_ln_timeshift_backward(colscale = NULL, dres = NULL, S = 1) on a
 * compacted copy of dy. */
int enh_ln_rows_strided_backward(const float* dy, int64_t dy_stride, const float* x, const float* w, int64_t M, int D, float eps, float* dx, enh_h16* dx16,
                                 float* dw, float* db, int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream);
/* Backward of enh_rq_embed_seq from gs [B, T, C] f32 (the gradient of the spatial stream) and gd [B T, Dp, C] f32 (of the depth stream; slot 0 is
 * never read).  Every fed occurrence (b, t, j) of a code adds [t <= T - 2] gs[b, t + 1] + sum_{d = j + 1}^{Dp - 1} gd[(b, t), d] to its row of
 * dtok_code [V, C], in ascending (b, t, j) order, the spatial term first, then d ascending; code (b, T - 1, Dp - 1) is never fed.  dpos_code [P, C]
 * (row t = sum_b gs[b, t + 1] for t <= T - 2, zero beyond), dpos_depth [Dp - 1, C] (row d - 1 = sum_{b, t} gd[(b, t), d]), dtok_cond [Vc, C]
 * (row conds[b] += gs[b, 0]) and dpos_cond [C].  Rows that do not occur are zero; accumulate != 0 adds to the five tables and leaves those rows
 * alone.  2 <= Dp <= 8, C % 4 == 0, C <= 8192; ids outside a table are clamped. */
int enh_rq_embed_seq_backward(const float* gs, const float* gd, const int64_t* conds, const int64_t* codes, int B, int T, int Dp, int C, int Vc, int V, int P,
                              float* dtok_cond, float* dpos_cond, float* dtok_code, float* dpos_code, float* dpos_depth, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENH_HIP_H */
