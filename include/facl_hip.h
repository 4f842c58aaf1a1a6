/*
 * facl_hip.h -- C ABI of libfacl_hip.so, the MI355X (gfx950) implementation of FACL's
 * contrastive-step hot path.
 *
 * The reference (tangent-T/FACL) is 100 % Python on stock PyTorch ops and has no FFI of its own;
 * each entry point below replaces a composition of torch ops at the cited reference file:line
 * (paths relative to the reference's training_code/).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to call them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch's allocator in
 *     our host code); the library never allocates, frees or copies persistent memory;
 *   - every launch goes to `stream` (a hipStream_t passed as void*), nothing synchronises;
 *   - return value: 0 on success, a positive hipError_t if a launch failed, a negative
 *     FACL_E_* code if the arguments are unsupported (nothing is launched in that case);
 *   - re-entrant, no global state, no host threads.
 *   - fp32 tensors unless said otherwise; "rows" of activations are positions (cloud-major,
 *     then centroid, then neighbour), channels are the fastest axis.
 */
#ifndef FACL_HIP_H
#define FACL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FACL_E_SHAPE  (-1)   /* unsupported shape (see each function)            */
#define FACL_E_NULL   (-2)   /* a required pointer is NULL                       */
#define FACL_E_ALIGN  (-3)   /* a pointer is not aligned as the kernel requires  */
#define FACL_E_CONFIG (-4)   /* the fused variant does not cover this size: use the unfused entry points */

/* Library / ABI version: (major << 16) | minor. */
int facl_version(void);

/* ---- farthest point sampling ------------------------------------------------------------
 * cn3d_data_load.py:301-320 (= cn3D_data_set.py:675-694): iterative FPS with the start index
 * given explicitly (the reference draws it with np.random.randint).  argmax takes the lowest
 * index among equal maxima (np.argmax).  dist^2 = (dx*dx+dy*dy)+dz*dz in the input dtype.
 *   xyz       (M, N, ld) rows; the first 3 columns of each row are x,y,z   [f32 | f64]
 *   start     (M) int32, each in [0,N)
 *   out_idx   (M, m) int32
 * Supported: 1 <= N <= 4096, 1 <= m, ld >= 3. */
int facl_fps_f32(const float* xyz, int M, int N, int ld, int m, const int32_t* start,
                 int32_t* out_idx, void* stream);
int facl_fps_f64(const double* xyz, int M, int N, int ld, int m, const int32_t* start,
                 int32_t* out_idx, void* stream);

/* cn3D_data_set.py:665-672: reorder each cloud so that rows picks[0..m) come first and the
 * remaining rows follow in ascending order (np.setdiff1d), truncated to N rows.
 *   points (M,N,D) f32 -> out (M,N,D) f32 (must not alias);  picks (M,m) int32. */
int facl_fps_reorder(const float* points, int M, int N, int D, const int32_t* picks, int m,
                     float* out, void* stream);

/* ---- kNN-then-radius grouping -----------------------------------------------------------
 * utils_my.py:255-291 (group_points_3DV) / :7-42 (group_points_3DV_2048): centroids are rows
 * 0..S-1; fp32 dist^2 = (dx*dx+dy*dy)+dz*dz; the K nearest are kept; a kept neighbour with
 * dist^2 > r2 (strict) is replaced by the centroid's own row; all D channels are gathered and
 * xyz is centred on the centroid.
 *   points (M,N,D) f32, FACL_SA_D_MIN <= D <= FACL_SA_D_MAX (xyz + up to five feature channels); D == 4 needs 16-byte
 *          aligned points / xt, no other D has an alignment rule
 *   idx    (M,S,K) int32, ascending along K before the radius replacement   (may be NULL)
 *   xt     (M,S,K,D) f32 -- the memory behind the reference's (M,D,S,K) view (may be NULL)
 *   yt     (M,S,3)   f32 -- the memory behind the reference's (M,3,S,1) view (may be NULL)
 * Supported: S <= N <= 4096, 1 <= K <= N. */
int facl_group(const float* points, int M, int N, int D, int S, int K, float r2,
               int32_t* idx, float* xt, float* yt, void* stream);
/* The same on the loader's clip-major batch: clips (B,G,N,D) contiguous; outputs are view-major, cloud m = g*B + b
 * (the permute(1,0,2,3).reshape(-1,N,D) copy of cn3d_train_motion_GL.py:226 is folded into the kernel's addressing). */
int facl_group_clips(const float* clips, int B, int G, int N, int D, int S, int K, float r2, int32_t* idx,
                     float* xt, float* yt, void* stream);

/* ---- train-mode BatchNorm plumbing (fp64) -------------------------------------------------
 * BN semantics: cn3d_model_conbag.py:46,50,54,64,68,72,84 (nn.BatchNorm2d/1d defaults).
 * `sums` is (C,2) double = per-channel (sum, sum of squares) over `count` positions; under DDP the
 * host all-reduces `sums` (and adds the counts) between the producing pass and facl_bn_finalize.
 * `bnc` is (5,C) float: mean, invstd, scale = gamma*invstd, shift = beta - mean*scale, sign(gamma).
 * running_mean / running_var (may both be NULL) are updated in place with `momentum` and the
 * unbiased variance, like F.batch_norm(training=True). */
/* size of the scratch buffer `ws` the reducing calls need.  Nothing in it has to survive between calls and nothing has to be
 * initialised: every partial row a call reads, the same call has written. */
int64_t facl_ws_bytes(void);
/* aamax (or NULL): FACL_AMAX_WORDS uint32 that receive (in every slot) the bits of a rigorous BOUND of the layer's activation
 * max|gamma (y - mean) invstd + beta| over the batch: |gamma| sqrt(count - 1) sigma invstd + |beta| (Samuelson's inequality).
 * It is the fp16x3 operand scale of that activation (see "fp16x3 operand scales" below). */
/* zamax (or NULL): another FACL_AMAX_WORDS buffer that the call ZEROES (the next kernel raises it with atomics: spares a fill launch) */
int facl_bn_finalize(const double* sums, int C, double count, const float* gamma, const float* beta,
                     float eps, float momentum, float* running_mean, float* running_var, float* bnc,
                     uint32_t* aamax, uint32_t* zamax, void* stream);
int facl_bn_eval_consts(int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* bnc, void* stream);
/* The same two calls for a layer BEHIND another one, `prev` = `nprev` floats (or NULL: exactly the calls above) that the layer's
 * input was computed with.  The heavy passes apply the previous layer's ReLU as max(v, 0), which turns a NaN into a clean 0, so a
 * NaN / inf in the previous layer's constants never shows in this layer's sums, where nn.ReLU keeps it and the next convolution
 * spreads it over every channel.  With a non-finite value anywhere in `prev`, every output of the call (bnc, the running buffers)
 * is NaN, as the reference's statistics are; with a finite `prev` every output is bit-identical to the call without it.
 * Training: prev = rows 2..3 (scale, shift) of the previous layer's bnc, so the flag travels bnc1 -> bnc2 -> bnc3 and facl_sa_pool
 * puts it into the features.  Eval (no statistics): prev = the FACL_AMAX_WORDS words of the buffer facl_absmax measured x into. */
int facl_bn_finalize_after(const double* sums, int C, double count, const float* gamma, const float* beta,
                           float eps, float momentum, float* running_mean, float* running_var, float* bnc,
                           uint32_t* aamax, uint32_t* zamax, const float* prev, int nprev, void* stream);
int facl_bn_eval_consts_after(int C, const float* gamma, const float* beta, const float* running_mean,
                              const float* running_var, float eps, float* bnc, const float* prev, int nprev, void* stream);

/* ---- set-abstraction point-MLP forward (net3DV_1, cn3d_model_conbag.py:43-58 / :162-177) ----
 * x is the grouped input, (P,D) rows = the memory behind the reference's (M,D,S,K) view, P = M*S*K,
 * K = 64 ("unit" = 64 consecutive rows = one group), 3 <= D <= 8 (FACL_SA_D_MIN..FACL_SA_D_MAX).  Weights are the reference's
 * tensors as stored in the checkpoint: W1 (64,D), W2 (64,64), W3 (256,64), row-major (Cout,Cin).
 *   facl_sa_x_moments           x -> mom = [sum_p x (D) | sum_p x x^T (D*D)]  (double)
 *   facl_bn1_sums_from_moments  mom -> sums of y1 = W1 x + b1 (exact: y1 is affine in x)
 *   facl_sa_l1tab               fold BN1 into layer 1: l1tab (64,FACL_SA_L1_COLS(D)) = [scale*W1 | 0 | scale*b1+shift | 0]
 *   facl_sa_fwd2                x -> y2 = relu(bn1(y1)) W2^T + b2, stored in "fragment layout"
 *                               (nunits*4096 floats, see csrc/common.h); sums2 (64,2) or NULL
 *   facl_sa_fwd3                y2 -> per (group,channel) max_k sgn3*y3 and its argmax k (uint8),
 *                               y3 = relu(bn2(y2)) W3^T + b3; sums3 (256,2) = (sum, sumsq) of y3 or NULL
 *   facl_sa_pool                pooled = relu(|scale3| * ymax + shift3)   (rows,C)
 *
 * The D-dependent layer-1 layouts.  FACL_SA_L1_COLS(D) is 8 for D <= 4 and 12 for D > 4:
 *   l1tab  (64, FACL_SA_L1_COLS(D)) floats per row: the folded weights in columns 0..FACL_SA_L1_COLS(D)-5 (zero for i >= D),
 *          the folded bias in column FACL_SA_L1_COLS(D) - 4, zeros after it (D <= 4: [w0 w1 w2 w3 | b 0 0 0]);
 *   R1     the tail of facl_sa_bwd2's output, (FACL_SA_L1_COLS(D), 64) doubles: rows sum_p x_d*dz1 (d < D), then sum_p dz1
 *          (row D), then zeros; the whole output is FACL_SA_BWD2_OUT(D) doubles (4608 for D <= 4, 4864 for D > 4).
 */
#define FACL_SA_D_MIN 3
#define FACL_SA_D_MAX 8
#define FACL_SA_L1_COLS(D) ((D) <= 4 ? 8 : 12)
#define FACL_SA_BWD2_OUT(D) (64 * 64 + 64 * FACL_SA_L1_COLS(D))
int facl_sa_x_moments(const float* x, int64_t P, int D, double* mom, void* ws, void* stream);
int facl_bn1_sums_from_moments(const double* mom, double count, int D, const float* W1, const float* b1,
                               double* sums, void* stream);
/* training, the 64-channel first layer: facl_bn1_sums_from_moments + facl_bn_finalize + facl_sa_l1tab in ONE launch (sums (64,2),
 * bnc (5,64), running statistics, the activation bound in aamax, l1tab (64,FACL_SA_L1_COLS(D))); every output bit-identical to
 * the three calls */
int facl_sa_bn1_chain(const double* mom, double count, int D, const float* W1, const float* b1, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                      double* sums, float* bnc, uint32_t* aamax, float* l1tab, void* stream);
/* xamax -> a1amax (both or neither; FACL_AMAX_WORDS uint32 each): the bound of max|a1| from max|x| (eval-mode constants give
 * no bound of their own; in training facl_bn_finalize's aamax of BN1 serves) */
int facl_sa_l1tab(const float* W1, const float* b1, int D, const float* scale, const float* shift,
                  float* l1tab, const uint32_t* xamax, uint32_t* a1amax, void* stream);
/* a1amax: bits of a bound of max|a1| (FACL_AMAX_WORDS uint32): the fp16x3 scale of the layer-1 activation */
int facl_sa_fwd2(const float* x, int64_t nunits, int D, const float* l1tab, const float* W2,
                 const float* b2, float* y2f, double* sums2, void* ws, const uint32_t* a1amax, void* stream);
int facl_sa_fwd3(const float* y2f, int64_t nunits, const float* scale2, const float* shift2,
                 const float* W3, const float* b3, const float* sgn3, float* ymax, uint8_t* arg,
                 double* sums3, void* ws, void* stream);
/* (sgn3 / sgn arguments of facl_sa_fwd3 and facl_gemm_fwd_segmax: only the SIGN of each entry is used, sign(0) = +1, so the
 * BatchNorm weight itself can be passed.) */
/* fp16-input twin of facl_sa_fwd3 (dense configuration): a2 and W3 rounded to fp16, one v_mfma_f32_32x32x16_f16 product
 * per multiply-add, fp32 accumulation; same outputs. */
int facl_sa_fwd3_f16(const float* y2f, int64_t nunits, const float* scale2, const float* shift2, const float* W3,
                     const float* b3, const float* sgn3, float* ymax, uint8_t* arg, double* sums3, void* ws,
                     void* stream);
/* fp16x3 twin of facl_sa_fwd3 (csrc/common.h: a2 and W3 as two fp16 planes each of the operand times a power of two
 * taken from its own maximum / bound, three products per multiply-add, fp32 accumulation): fp32-GEMM accuracy at half the
 * MFMA work; same outputs.  The model's default.  a2amax: bits of a bound of max|relu(bn2(y2))| (FACL_AMAX_WORDS uint32). */
int facl_sa_fwd3_h3(const float* y2f, int64_t nunits, const float* scale2, const float* shift2, const float* W3,
                    const float* b3, const float* sgn3, float* ymax, uint8_t* arg, double* sums3, void* ws,
                    const uint32_t* a2amax, void* stream);
/* amax (or NULL): FACL_AMAX_WORDS uint32 (zeroed, or holding the maximum of a tensor that shares the scale) raised to the
 * bits of max(pooled) */
int facl_sa_pool(const float* ymax, int64_t rows, int C, const float* scale, const float* shift,
                 float* pooled, uint32_t* amax, void* stream);
/* net3DV_1 in EVAL mode as ONE kernel (csrc/sa_eval.hip; SURVEY 8 f-1: extract_motion_feature.py:143-221 runs the encoder under
 * eval(), every BatchNorm a constant affine): x (nunits*64, D) grouped rows -> pooled (nunits, 256); nothing else is stored (no y2
 * tile, no statistics, no argmax).  l1tab from facl_sa_l1tab with BN1's eval constants (and xamax -> a1amax); scale2 / shift2 (64),
 * scale3 / shift3 (256): rows 2 and 3 of facl_bn_eval_consts. */
int facl_sa_eval(const float* x, int64_t nunits, int D, const float* l1tab, const float* W2, const float* b2,
                 const float* scale2, const float* shift2, const float* W3, const float* b3, const float* scale3,
                 const float* shift3, float* pooled, const uint32_t* a1amax, void* stream);
/* ---- fp16x3 operand scales: measured maxima for operands no BatchNorm bounds ----
 *   facl_absmax          raises the slots of `amax` (FACL_AMAX_WORDS uint32, zeroed by the caller or pre-seeded) to max|x| over
 *                        the FINITE elements of x; a NaN / inf element raises word 1 of the buffer (no slot) to NaN bits instead
 *   facl_rows_act_amax   the same for max relu(scale[c] y[r][c] + shift[c]) of a (R,C) array (eval-mode layers: running
 *                        statistics say nothing about the data) */
int facl_absmax(const float* x, int64_t n, uint32_t* amax, void* stream);
int facl_rows_act_amax(const float* y, int64_t R, int C, const float* scale, const float* shift, uint32_t* amax, void* stream);

/* ---- set-abstraction point-MLP backward (autograd of net3DV_1) ---------------------------
 * See csrc/sa_bwd.hip for the algebra ("BN-affine folding": the dense part of BN3's backward is
 * affine in y3, so layer 3's backward is 64x64 work per position and y3 is never re-materialised).
 *   facl_sa_bwd0    dpooled (rows,256), ymax, bnc3 (5,256) -> coef = scale3*dz3 (rows,256),
 *                   sums (256,2) = (dbeta3, dgamma3)
 *   facl_sa_bwd1    y2f, bnc2 (5,64), G3 (64,64), h3 (64), W3, coef, arg -> dz2f (fragment layout),
 *                   sums (64,2) = (dbeta2, dgamma2)
 *   facl_sa_bwd_w3  y2f, bnc2, coef, arg -> out (20544 doubles) =
 *                   [ sum_g coef*a2[arg] (256,64) | sum_p a2^T a2 (64,64) | sum_p a2 (64) ]
 *   facl_sa_bwd2    dz2f, y2f, x, bw2 (4,64) = [scale2 | A | B | mean2] with dy2 = scale2*dz2 + A + B*(y2-mean2),
 *                   W2, l1tab -> out (FACL_SA_BWD2_OUT(D) doubles) = [ dW2 (64,64) | R1 (FACL_SA_L1_COLS(D),64) ],
 *                   R1 rows = sum_p x_d*dz1 (d < D), then sum_p dz1, then zeros.
 */
int facl_sa_bwd0(const float* dpooled, const float* ymax, int64_t rows, const float* bnc3, float* coef,
                 double* sums, void* ws, void* stream);
int facl_sa_bwd1(const float* y2f, int64_t nunits, const float* bnc2, const float* G3, const float* h3,
                 const float* W3, const float* coef, const uint8_t* arg, float* dz2f, double* sums,
                 void* ws, const uint32_t* a2amax, void* stream);
int facl_sa_bwd_w3(const float* y2f, int64_t nunits, const float* bnc2, const float* coef,
                   const uint8_t* arg, double* out, void* ws, const uint32_t* a2amax, void* stream);
/* a1amax / a2amax: the activation bounds the forward passes were given (facl_sa_fwd2 / facl_sa_fwd3_h3).  facl_sa_bwd2 returns
 * FACL_E_CONFIG for D > 4 when the exact-fp32 A/B kernel is selected (FACL_BWD2_F32=1): it does not fit a CU's LDS there */
int facl_sa_bwd2(const float* dz2f, const float* y2f, const float* x, int64_t nunits, int D,
                 const float* bw2, const float* W2, const float* l1tab, double* out, void* ws,
                 const uint32_t* a1amax, void* stream);
/* fp64 closed-form assembly between those passes (csrc/finalize.hip).  "_g" = after the SyncBN all-reduce,
 * "_l" = this rank's sums (parameter gradients stay local; the data-parallel wrapper averages them).
 *   facl_sa_bwd_consts3  sums0 (dbeta3,dgamma3) -> G3 (64,64), h3 (64) for facl_sa_bwd1
 *   facl_sa_bwd_consts2  sums1 (dbeta2,dgamma2) -> bw2 (4,64) for facl_sa_bwd2
 *   facl_sa_bwd_final    all partial sums -> dW3,dgamma3,dbeta3, dW2,dgamma2,dbeta2, dW1,dgamma1,dbeta1
 *                        (R1_g (FACL_SA_L1_COLS(D),64) = all-reduced tail of facl_sa_bwd2's output, mom_l = local x moments) */
/* BN backward constants of a row layer (tail): sums (C,2) = (dbeta, dgamma) of THIS rank / after the SyncBN
 * all-reduce -> dbeta (C), dgamma (C) fp32 parameter gradients (local) and kk (2,C) = reduced sums / P */
int facl_bn_bwd_consts(const double* sums_local, const double* sums_global, int C, double P, float* dbeta,
                       float* dgamma, float* kk, void* stream);
int facl_sa_bwd_consts3(const double* sums0, const float* bnc3, const float* W3, const float* b3, double P,
                        float* G3, float* h3, void* stream);
int facl_sa_bwd_consts2(const double* sums1, const float* bnc2, double P, float* bw2, void* stream);
int facl_sa_bwd_final(const double* out3, const double* sums0_g, const double* sums0_l, const float* bnc3,
                      const float* W3, const float* b3, const double* out2, const double* sums1_l,
                      const double* R1_g, const double* mom_l, const float* bnc1, const float* W1,
                      const float* b1, int D, double P, float* dW3, float* dg3, float* dbe3, float* dW2,
                      float* dg2, float* dbe2, float* dW1, float* dg1, float* dbe1, void* stream);
/* Frozen (eval-mode) BatchNorm backward: bnc = the (5,C) constants of facl_bn_eval_consts (running statistics), so
 * z = scale*y + shift is a constant affine and dy = scale*dz.  The (C,2) sums of the SAME statistics passes
 * (facl_rows_bwd_stats, facl_segmax_bwd_stats[_ymax], facl_gemm_rs_dgrad_bnstats; facl_sa_bwd0 / facl_sa_bwd1) are then
 * (dbeta, dgamma) themselves; nothing is all-reduced.
 *   facl_bn_bwd_consts_frozen   sums (C,2), bnc -> dbeta (C), dgamma (C), dbias (C) = scale*dbeta (the gradient of the bias
 *                               of the conv / Linear in front, identically zero in train mode) and kk (2,C) = 0, with which
 *                               facl_rows_bwd_apply[_amax] / facl_segmax_bwd_apply[_amax] give dy = scale*dz
 *   facl_sa_bwd_consts3_frozen  G3 (64,64) = 0, h3 (64) = 0 for facl_sa_bwd1: da2 keeps its sparse rows only
 *   facl_sa_bwd_consts2_frozen  bnc2 -> bw2 (4,64) = [scale2 | 0 | 0 | mean2] for facl_sa_bwd2: dy2 = scale2*dz2
 *   facl_sa_bwd_final_frozen    out3 (facl_sa_bwd_w3; its sparse part), sums0 (facl_sa_bwd0), out2 (facl_sa_bwd2), sums1
 *                               (facl_sa_bwd1), bnc3 / bnc2 / bnc1 -> the twelve gradients of net3DV_1:
 *                               dW3 = sparse part, dW2 = out2's, dW1 = scale1*R1[x rows]; (dbeta, dgamma) = the sums
 *                               (layer 1: from R1 in closed form); db = scale*dbeta.  No x moments (an eval forward has none). */
int facl_bn_bwd_consts_frozen(const double* sums, const float* bnc, int C, float* dbeta, float* dgamma, float* dbias,
                              float* kk, void* stream);
int facl_sa_bwd_consts3_frozen(float* G3, float* h3, void* stream);
int facl_sa_bwd_consts2_frozen(const float* bnc2, float* bw2, void* stream);
int facl_sa_bwd_final_frozen(const double* out3, const double* sums0, const float* bnc3, const double* out2,
                             const double* sums1, const float* bnc2, const float* bnc1, const float* W1, const float* b1,
                             int D, float* dW3, float* dg3, float* dbe3, float* db3, float* dW2, float* dg2, float* dbe2,
                             float* db2, float* dW1, float* dg1, float* dbe1, float* db1, void* stream);

/* ---- encoder tail: row-major (R,C) BatchNorm / ReLU / max-over-S kernels ----------------------
 * net3DV_3 + my_max_pool + netR_FC (cn3d_model_conbag.py:61-88, :199-207).  The dense contractions
 * between them are the facl_gemm_* entries below (hand-written MFMA GEMMs); these kernels are everything else.
 * bnc = (5,C) constants of facl_bn_finalize / facl_bn_eval_consts; kk = (2,C) = (dbeta/P, dgamma/P).
 *   facl_rows_stats        y (R,C) -> sums (C,2)
 *   facl_rows_bn_relu      out = relu(scale*y + shift)                         (may run in place)
 *   facl_rows_segmax       x_pre[m,c] = max_s relu(bn(y[m,s,c])), arg = first maximising s
 *   facl_rows_bwd_stats    sums (C,2) = (sum dz, sum dz*yhat), dz = dout*[bn(y) > 0]
 *   facl_rows_bwd_apply    dy = scale*(dz - k1 - yhat*k2)
 *   facl_segmax_bwd_stats / _apply : the same two steps for the gradient arriving through the max over S
 */
int facl_rows_stats(const float* y, int64_t R, int C, double* sums, void* ws, void* stream);
int facl_rows_bn_relu(const float* y, int64_t R, int C, const float* scale, const float* shift, float* out,
                      void* stream);
int facl_rows_segmax(const float* y, int64_t M, int S, int C, const float* bnc, float* out, int32_t* arg,
                     void* stream);
int facl_rows_bwd_stats(const float* dout, const float* y, int64_t R, int C, const float* bnc, double* sums,
                        void* ws, void* stream);
/* gobaol_max_pool (cn3d_model_conbag.py:225-226) on the per-view maxima: x (G*B,C) view-major (row g*B+b) ->
 * out (B,C) = max over the G views, arg (B,C) = first view that attains it; backward routes dout to that view's row
 * of dx (G*B,C) and writes zeros elsewhere. */
int facl_viewmax_fwd(const float* x, int G, int B, int C, float* out, int32_t* arg, void* stream);
int facl_viewmax_bwd(const float* dout, const int32_t* arg, int G, int B, int C, float* dx, void* stream);
/* the same routing ADDED into dx (G*B,C), whose rows already hold the other gradient path of x_pre (each (clip, channel)
 * touches exactly one element: no atomics) */
int facl_viewmax_bwd_add(const float* dout, const int32_t* arg, int G, int B, int C, float* dx, void* stream);
/* gobaol_max_pool straight into netR_FC's stacked input (cn3d_model_conbag.py:225-229): h (G*B + B, C) = [x ; max over the G views
 * of x], arg (B,C) = the first view that attains the maximum -- facl_viewmax_fwd plus the copy of the rows it reads anyway. */
int facl_viewmax_stack(const float* x, int G, int B, int C, float* h, int32_t* arg, void* stream);

/* ---- netR_FC's BatchNorm1d + ReLU over the STACKED rows (cn3d_model_conbag.py:203-204 called at :228 on the G*B view rows and
 * at :229 on the B clip rows): y (R,C), segment a = rows [0,M), segment b = rows [M,R); two batch statistics, the running
 * buffers updated twice (a first), one set of kernels (csrc/fchead.hip).  M % 32 == 0 (else FACL_E_CONFIG: use the
 * single-segment entries).  Statistics are kept as 32-row SLICE sums that the consumer adds itself (no reduction launch):
 *   facl_fc_bn_stats      slice (sum, sumsq) of y into `ws`; with sums2 (2,C,2) also the segment totals (SyncBN all-reduce).
 *   facl_fc_bn_apply      bnc2 (2,5,C) = (mean, invstd, scale, shift, sign) per segment from `sums2` (totals) or from `part`
 *                         (nslices_a + nslices_b slice rows of (C,2) doubles: `ws` after facl_fc_bn_stats);
 *                         running statistics (momentum, unbiased variance) for a then b; a_out = relu(bn(y)).
 *   facl_fc_bn_bwd_stats  slice sums of dz = dact*[z>0] and dz*yhat into `ws` (+ totals into sums2).
 *   facl_fc_bn_bwd_apply  kk2 (2,2,C), dy = scale (dz - k1 - yhat k2) with k = (all-reduced sums2_g, or the local slice sums
 *                         in `ws`) / count; dgamma / dbeta (C) = this rank's sums of both segments (fp32 add of the two). */
int facl_fc_bn_stats(const float* y, int64_t M, int64_t R, int C, double* sums2, void* ws, void* stream);
int facl_fc_bn_apply(const float* y, int64_t M, int64_t R, int C, const double* sums2, const double* part, int nslices_a,
                     int nslices_b, double count_a, double count_b, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, float* bnc2, float* a_out, void* stream);
int facl_fc_bn_bwd_stats(const float* dact, const float* y, int64_t M, int64_t R, int C, const float* bnc2, double* sums2,
                         void* ws, void* stream);
int facl_fc_bn_bwd_apply(const float* dact, const float* y, int64_t M, int64_t R, int C, const float* bnc2,
                         const double* sums2_g, const void* ws, double count_a, double count_b, float* dgamma, float* dbeta,
                         float* kk2, float* dy, void* stream);
/* out (C) = column sums of x (R,C), fp64 accumulation: the bias gradient of netR_FC's last Linear (dout.sum(0)). */
int facl_col_sums(const float* x, int64_t R, int C, float* out, void* stream);
/* dWc (C,3) fp64 = dy^T centers: the centroid-xyz columns of the first per-centroid layer's weight gradient
 * (the input of net3DV_3 is torch.cat((yt, xt), 1), cn3d_model_conbag.py:219) in one streaming pass over dy */
int facl_rows_center_wgrad(const float* dy, const float* centers, int64_t R, int C, double* dWc, void* ws,
                           void* stream);
int facl_rows_bwd_apply(const float* dout, const float* y, int64_t R, int C, const float* bnc,
                        const float* kk, float* dy, void* stream);
int facl_segmax_bwd_stats(const float* dxpre, const float* xpre, const float* y, const int32_t* arg,
                          int64_t M, int S, int C, const float* bnc, double* sums, void* ws, void* stream);
/* the same sums from ymax (M,C) = max over the S rows of sign(gamma)*y, as facl_gemm_rs_fwd / facl_gemm_fwd_segmax return it: the
 * value at the argmax is sign(gamma)*ymax exactly (bnc row 4 holds the sign), so y is not gathered (one cache line per element) */
int facl_segmax_bwd_stats_ymax(const float* dxpre, const float* xpre, const float* ymax, int64_t M, int C,
                               const float* bnc, double* sums, void* ws, uint32_t* zamax, int zwords, void* stream);
/* (zamax, zwords: amax words -- or NULL, 0 -- that the call zeroes for the *_amax kernels behind it: spares a fill launch) */
int facl_segmax_bwd_apply(const float* dxpre, const float* xpre, const float* y, const int32_t* arg,
                          int64_t M, int S, int C, const float* bnc, const float* kk, float* dy, void* stream);
/* the two dy producers of the BatchNorm backward, also maintaining max|dy| in `amax`: a buffer of FACL_AMAX_WORDS uint32 the
 * caller zeroed, in which the kernels raise one of 64 slots (one 128-byte line each: atomics on a single address serialise)
 * to the bit pattern of the largest |dy| they wrote (non-negative floats order like unsigned integers; a NaN lands above
 * everything); max|dy| = the maximum over the buffer.  The fp16x3 GEMMs that consume dy take its power-of-two operand scale
 * from there, on the device, with no host round trip.  amax = null: the plain functions.  With amax the 4-channel kernels
 * are required (C % 4 == 0, 16-byte aligned tensors), else FACL_E_ALIGN. */
#define FACL_AMAX_WORDS 2048
int facl_rows_bwd_apply_amax(const float* dout, const float* y, int64_t R, int C, const float* bnc, const float* kk,
                             float* dy, uint32_t* amax, void* stream);
int facl_segmax_bwd_apply_amax(const float* dxpre, const float* xpre, const float* y, const int32_t* arg, int64_t M, int S,
                               int C, const float* bnc, const float* kk, float* dy, uint32_t* amax, void* stream);

/* ---- fp32 MFMA GEMMs of the tail's dense 1x1 channel contractions (csrc/gemm.hip) ------------------
 * Weights are the checkpoint tensors, row-major (Cout,Cin) with leading dimension ldw (multiple of 4).
 *   facl_gemm_fwd    y (M,N) = a' W^T + bias [+ centers (M,3) Wc (N,ldwc)^T], a' = a or relu(pscale*a+pshift);
 *                    sums (N,2) = column (sum, sumsq) of y for the BN that follows (or NULL)
 *   facl_gemm_dgrad  da (M,K) = dy (M,N) W (N,K)
 *   facl_gemm_wgrad  dW (N,K) = dy^T a, contraction over the M rows split into nz slices
 *                    (`slices` = scratch of nz*N*K floats), summed in slice order (deterministic) */
int facl_gemm_fwd(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                  const float* pscale, const float* pshift, const float* centers, const float* Wc,
                  int ldwc, float* y, double* sums, void* ws, void* stream);
/* facl_gemm_fwd with my_max_pool over blocks of S = 64 consecutive rows fused into its epilogue
 * (cn3d_model_conbag.py:71-73 + :80/:199): ymax (M/64,N) = max over the block of sgn[j]*y, arg (M/64,N) = first row of
 * the block that attains it.  FACL_E_CONFIG when the problem is too small for the 128x128-tile kernel (callers then use
 * facl_gemm_fwd + facl_rows_segmax). */
int facl_gemm_fwd_segmax(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                         const float* sgn, float* y, double* sums, float* ymax, int32_t* arg, void* ws,
                         void* stream);
int facl_gemm_dgrad(const float* dy, int64_t M, int N, const float* W, int ldw, int K, float* da,
                    void* stream);
int facl_gemm_wgrad(const float* dy, const float* a, int64_t M, int N, int K, int lda, float* dW,
                    float* slices, int nz, void* stream);
/* facl_gemm_wgrad_acc: dW (N,K) += dy^T a -- the weight-gradient GEMM accumulating INTO its output (the second gradient path of
 *   the loss's keys, d x += dsim^T @ [x ; x_global], without an add launch).  prec: 0 = fp32-grade (bf16x6), 1 = fp16 inputs,
 *   2 = bf16x3 (the twins below).  Few rows only (M <= 8192, one wave of 64x64 workgroups): FACL_E_CONFIG otherwise. */
int facl_gemm_wgrad_acc(const float* dy, const float* a, int64_t M, int N, int K, int lda, float* dW, int prec, void* stream);
/* fp16-input twins (dense configuration, BASELINE configs[4] "fp16 MFMA point-MLP"): same arguments and fp32 storage;
 * the operands are rounded to fp16 while their tiles are staged and every multiply-add is ONE
 * v_mfma_f32_32x32x16_f16 product with fp32 accumulation (instead of the six bf16 products of the fp32-grade path). */
int facl_gemm_fwd_f16(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                      const float* pscale, const float* pshift, const float* centers, const float* Wc, int ldwc,
                      float* y, double* sums, void* ws, void* stream);
int facl_gemm_fwd_segmax_f16(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                             const float* sgn, float* y, double* sums, float* ymax, int32_t* arg, void* ws,
                             void* stream);
int facl_gemm_dgrad_f16(const float* dy, int64_t M, int N, const float* W, int ldw, int K, float* da,
                        void* stream);
int facl_gemm_wgrad_f16(const float* dy, const float* a, int64_t M, int N, int K, int lda, float* dW,
                        float* slices, int nz, void* stream);
/* ---- row-streamed forward / dgrad for the 49,152-row layers (csrc/gemm_rs.hip) -------------------------------------------
 * Replaces the same torch chain as facl_gemm_fwd / facl_gemm_dgrad (Conv2d 1x1 of net3DV_3, cn3d_model_conbag.py:61-77,
 * and its autograd) with the weight operand pre-split ONCE per step into fragment-ordered bf16 planes
 * (facl_gemm_rs_planes; caller-allocated buffer of facl_gemm_rs_planes_bytes) and the activation rows streamed through
 * per-wave LDS slots.  Same arithmetic as facl_gemm_fwd (six bf16 products per multiply-add): bit-identical results.
 *   facl_gemm_rs_supported   1 when (rows M, contraction K, output columns N) is served: M >= 2048, 64 <= K <= 1024,
 *                            K % 32 == 0, N % 256 == 0; else 0 (callers then use facl_gemm_fwd / facl_gemm_dgrad)
 *   facl_gemm_rs_planes      transposed = 0: planes for y = a W^T (W (N,K), leading dimension ldw; Wc (N,3) optional:
 *                            the centroid-xyz columns of torch.cat((yt, xt), 1), :219); transposed = 1: planes for da = dy W
 *   facl_gemm_rs_fwd         y = f(a) W^T + bias [+ centers Wc^T], f = relu(pscale*a + pshift) when pscale is given (the
 *                            previous layer's BatchNorm2d + ReLU, :62-63: the activation is never materialised); sums (N,2)
 *                            as facl_gemm_fwd; sgn / ymax / arg (all or none) as facl_gemm_fwd_segmax (M % 64 == 0)
 *   `half` (planes and forward): 0 = three bf16 planes, six products per multiply-add (bf16x6); 1 = two fp16 planes of the
 *                            operands times a power of two, THREE products (fp16x3, csrc/common.h): the same fp32-GEMM
 *                            accuracy (22-bit operands, fp32 accumulation) at half the MFMA work.  No operand has a fixed
 *                            scale: the weights carry one power of two per 32-column tile (max|w| of the tile, taken by
 *                            facl_gemm_rs_planes and stored behind the planes), the row operand takes its scale from
 *                            `amax_a` (forward: FACL_AMAX_WORDS uint32 with the bits of a bound of max|f(a)| -- and of
 *                            max|centers| when centres are given -- from facl_bn_finalize / facl_sa_pool / facl_absmax /
 *                            facl_rows_act_amax); the planes must have been built with the same `half`
 *   facl_gemm_rs_dgrad       da (M,K) = dy (M,N) W.  half = 1: fp16x3 with dy's scale chosen per launch from `amax` (the
 *                            FACL_AMAX_WORDS buffer of facl_rows_bwd_apply_amax / facl_segmax_bwd_apply_amax): the
 *                            power of two that puts the maximum in [2^13, 2^14); elements down to 2^-16 of the maximum keep
 *                            22 bits, smaller ones lose at most 2^-38 of the maximum
 *   facl_gemm_rs_wgrad       amax non-null: the same arithmetic (dy by its scale, f(y) by the scale of `amax_b`, the bound the
 *                            forward GEMM that consumed f(y) was given)
 *   facl_gemm_wgrad_pro      dW (N,K) = dy^T relu(pscale*y + pshift): facl_gemm_wgrad whose `a` operand is recomputed from
 *                            the previous layer's raw output y (M,K) while it is staged (the companion of the forward
 *                            prologue: the activation tensor never exists); `_x3`: the opt-in three-product arithmetic.
 *                            FACL_E_CONFIG when the shape is not served by the 128x128-tile kernel (callers materialise a). */
int facl_gemm_wgrad_pro(const float* dy, const float* y, int64_t M, int N, int K, int ldy, const float* pscale,
                        const float* pshift, float* dW, float* slices, int nz, void* stream);
int facl_gemm_wgrad_pro_x3(const float* dy, const float* y, int64_t M, int N, int K, int ldy, const float* pscale,
                           const float* pshift, float* dW, float* slices, int nz, void* stream);
/* the same weight gradient in fp16x3 (see `half` above): dy by the scale read from `amax` (the FACL_AMAX_WORDS buffer of
 * facl_rows_bwd_apply_amax), the activation operand by the one read from `amax_b` (its bound, same format); pscale / pshift
 * null: `y` IS the activation.  FACL_E_CONFIG when the shape is not served by the 128x128-tile kernel (callers use the
 * bf16x6 entries). */
int facl_gemm_wgrad_h3(const float* dy, const float* y, int64_t M, int N, int K, int ldy, const float* pscale,
                       const float* pshift, const uint32_t* amax, const uint32_t* amax_b, float* dW, float* slices, int nz,
                       void* stream);
/* Weight gradient of the widest layer on the register-streamed kernel (csrc/gemm_rs.hip: k_wgrad_rs): dW (N,K) =
 * dy^T f(y), f = relu(pscale*y + pshift) when pscale is given (else identity).  facl_gemm_rs_wgrad_slices returns the number
 * of row slices the call will use (scratch = that many x N x K floats), or 0 when the shape is not served (N % 512, K % 128,
 * M >= 4096 and at least 8 output blocks): facl_gemm_rs_wgrad then returns FACL_E_CONFIG and callers use facl_gemm_wgrad[_pro]. */
int facl_gemm_rs_wgrad_slices(int64_t M, int N, int K);
int facl_gemm_rs_wgrad(const float* dy, const float* y, int64_t M, int N, int K, const float* pscale, const float* pshift,
                       const uint32_t* amax, const uint32_t* amax_b, float* dW, float* slices, void* stream);
int64_t facl_gemm_rs_planes_bytes(int N, int K, int with_centers);
int facl_gemm_rs_planes(const float* W, int ldw, int N, int K, int transposed, const float* Wc, int ldwc, int half,
                        void* planes, void* stream);
/* n <= 8 matrices in one launch: arrays (length n) of the per-matrix arguments of facl_gemm_rs_planes */
/* absmax_x / absmax_n / absmax_amax (all or none): the launch also raises `absmax_amax` (FACL_AMAX_WORDS uint32) to
 * max|absmax_x[0 .. absmax_n)| -- the centroid coordinates share the fp16x3 scale of the first layer's row operand */
int facl_gemm_rs_planes_multi(int n, const float* const* W, const int* ldw, const int* N, const int* K,
                              const int* transposed, const float* const* Wc, const int* ldwc, const int* half,
                              void* const* planes, const float* absmax_x, int64_t absmax_n, uint32_t* absmax_amax,
                              void* stream);
int facl_gemm_rs_supported(int64_t M, int K, int N);
int facl_gemm_rs_fwd(const float* a, int64_t M, int K, const void* planes, int half, const uint32_t* amax_a, int N,
                     const float* bias, const float* pscale, const float* pshift, const float* centers, float* y, double* sums,
                     const float* sgn, float* ymax, int32_t* arg, void* ws, void* stream);
int facl_gemm_rs_dgrad(const float* dy, int64_t M, int N, const void* planes, int half, const uint32_t* amax, int K,
                       float* da, void* stream);
/* facl_gemm_rs_dgrad + facl_rows_bwd_stats(da, y, bnc) in one pass: sums (K,2) = the BatchNorm-backward column sums of the
 * layer whose activation relu(bn(y)) was this GEMM's forward input, taken from the accumulator tile before it is stored */
int facl_gemm_rs_dgrad_bnstats(const float* dy, int64_t M, int N, const void* planes, int half, const uint32_t* amax, int K,
                               float* da, const float* y, const float* bnc, double* sums, void* ws, void* stream);
/* "bf16x3" twins (opt-in precision "x3"; never the default): each operand keeps its two leading bf16 pieces and a
 * multiply-add is three products (hi*mid, mid*hi, hi*hi) instead of six -- relative error of a product <= 3 * 2^-16
 * (results ~1e-5 of an fp64 GEMM; the north_star's tolerance for features / loss is 1e-4), half the MFMA work. */
int facl_gemm_fwd_x3(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                     const float* pscale, const float* pshift, const float* centers, const float* Wc, int ldwc,
                     float* y, double* sums, void* ws, void* stream);
int facl_gemm_fwd_segmax_x3(const float* a, int64_t M, int K, const float* W, int ldw, int N, const float* bias,
                            const float* sgn, float* y, double* sums, float* ymax, int32_t* arg, void* ws,
                            void* stream);
int facl_gemm_dgrad_x3(const float* dy, int64_t M, int N, const float* W, int ldw, int K, float* da,
                       void* stream);
int facl_gemm_wgrad_x3(const float* dy, const float* a, int64_t M, int N, int K, int lda, float* dW,
                       float* slices, int nz, void* stream);
int facl_sa_fwd3_x3(const float* y2f, int64_t nunits, const float* scale2, const float* shift2, const float* W3,
                    const float* b3, const float* sgn3, float* ymax, uint8_t* arg, double* sums3, void* ws,
                    void* stream);

/* ---- second-level grouping on channel-first features (utils_my.py:332-381 group_points_2 / group_points_2_3DV) ----
 * The kNN + radius rule of a second level runs on the level-1 centroid coordinates through facl_group (idx + centred xyz).
 * facl_gather_rows moves the features: out[r][col_off + c] = feat[m][idx[r]][c] for the rows r = (m, s2, k) of cloud m
 * (feat (M,S1,C) rows of stride ldf; out rows of stride ldo); with xyz (rows,3) also out[r][0..2] = xyz[r] (col_off = 3:
 * the reference's concatenated (3+C)-channel rows).  facl_scatter_rows is its transpose (gradient of the gather):
 * dfeat[m][s][c] = sum_{r: idx[r] = s} drows[r][col_off + c], rows added in index order (deterministic, no atomics). */
int facl_gather_rows(const float* feat, int ldf, int M, int S1, int C, const int32_t* idx, int rows_per_cloud,
                     const float* xyz, float* out, int ldo, int col_off, void* stream);
int facl_scatter_rows(const float* drows, int ldd, int col_off, int M, int S1, int C, const int32_t* idx,
                      int rows_per_cloud, float* dfeat, void* stream);

/* ---- contrastive losses on a similarity matrix (utils_my.py:53-116) ----------------------------
 * sim = anchors @ keys^T with J = G*Bk columns (column j belongs to clip j % Bk).  Same-clip columns count as exp(0) (the
 * reference multiplies them by 0); the anchor rows of a clip (one for the global loss, G-1 for the circle loss) form ONE
 * shared negative set; the clip's positive slots (G resp. G-1) are same-clip columns read before masking; CE = mean over B,
 * summed over the slots.  clip_offset = rank*B under data parallelism.
 *
 * Both losses of a training step (cn3d_train_motion_GL.py:265-316) in one launch on ONE similarity matrix
 * sim ((G+1)*B, J) = [x ; x_global] @ keys^T (row block g < G: view g of the local clips, block G: x_global; J = G*Bk).
 * order (G) int64 = the circle loss's view permutation (utils_my.py:96-97).  losses = [loss_c, loss_circle];
 * dsim ((G+1)*B, J) = d(loss_c + loss_circle)/d sim, every row written (the block of view order[G-1], which is no
 * anchor, is zero). */
int facl_contrast_pair(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                       float* dsim, double* losses, void* ws, void* stream);
/* facl_contrast_pair that also writes the fp32 values of the loop body: losses32 = [loss_c, loss_circle, loss_circle + loss_c]
 * (the fp32 sum of the two fp32 losses: `loss = loss_circle + loss_c`, cn3d_train_motion_GL.py:329), one finishing launch
 * instead of a reduction, a cast and an add. */
int facl_contrast_pair_sum(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                           float* dsim, double* losses, float* losses32, void* ws, void* stream);
/* facl_contrast_pair_sum with the treatment of the same-clip key columns as an argument.  mask_mode 0 (zero) = the reference's
 * rule above: the column is multiplied by 0 and stays in the log-sum-exp as exp(0); facl_contrast_pair_sum is this entry with
 * mode 0.  mask_mode 1 (exclude): same-clip columns are no members of the log-sum-exp (negatives only); their dsim is 0 and the
 * positives are still read before masking; needs Bk >= 2 (a negative must exist).  Any other mode: FACL_E_SHAPE. */
int facl_contrast_pair_sum_mask(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                                int mask_mode, float* dsim, double* losses, float* losses32, void* ws, void* stream);
/* Row pass in front of the similarity GEMM (cosine similarity and temperature of the contrastive losses): x (R,C) ->
 * n_r = x_r * s / max(||x_r||_2, 1e-12) (normalize = 1: F.normalize's clamp) or n_r = x_r * s (normalize = 0), with s =
 * 1/sqrt(temperature), so that n @ n^T = cos / temperature resp. <.,.> / temperature.  inv_norm (R) = 1 / max(||x_r||, 1e-12)
 * (1 with normalize = 0).  Backward: dx_r = s * inv_norm_r * (dn_r - xh_r <dn_r, xh_r>), xh_r = n_r / s, resp. dx_r = s * dn_r;
 * every row of dx is written.  Sum of squares and dot product in fp64 in a fixed order, one rounding per element, no atomics.
 * C % 4 == 0, 0 < s < inf, 16-byte aligned matrices. */
int facl_loss_rows_fwd(const float* x, int64_t R, int C, int normalize, float s, float* n, float* inv_norm, void* stream);
int facl_loss_rows_bwd(const float* dn, const float* n, const float* inv_norm, int64_t R, int C, int normalize, float s,
                       float* dx, void* stream);
/* facl_contrast_pair_sum_mask with a queue of negative keys from earlier steps.  sim_q ((G+1)*B, L) = [x ; x_global] @
 * queue^T; qstate = {head, valid} (two int32 ON THE DEVICE, read by the kernels: a captured step replays correctly while the
 * queue fills).  The first `valid` columns of sim_q are extra negative columns of every clip in both losses; they carry no clip
 * identity, so neither mask mode touches them.  Columns >= valid are never used (they may hold anything, NaN included; with
 * valid % 4 != 0 the 16-byte load that straddles `valid` fetches up to three of them and drops them) and their dsim_q is
 * written as exactly 0; a valid outside [0, L] is clamped.  dsim_q ((G+1)*B, L) = d(loss_c + loss_circle)/d sim_q, every
 * element written; dsim, losses, losses32 as above.  Same bits every run (no atomics).  L >= 1 and the domain of
 * facl_contrast_pair_sum_mask, else FACL_E_SHAPE; also when (G+1)*B*(ceil(J/2048) + ceil(L/2048)) chunk partials (12 bytes
 * each) do not fit the workspace. */
int facl_contrast_pair_queue(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L, const int64_t* order,
                             int clip_offset, int mask_mode, const int32_t* qstate, float* dsim, float* dsim_q, double* losses,
                             float* losses32, void* ws, void* stream);
/* Ring buffer of the queue: copies rows (P,C) into the slots [head, head+P) of queue (L,C) and then, in a second launch in
 * stream order, sets head = (head + P) % L and valid = min(valid + P, L) in qstate (device int32[2]).  L % P == 0, so a push
 * never wraps inside itself; head is clamped to a multiple of P below L and valid to [0, L] before use.  C % 4 == 0, L % P == 0,
 * else FACL_E_SHAPE (checked first); a NULL pointer: FACL_E_NULL; rows / queue 16-byte aligned, else FACL_E_ALIGN. */
int facl_queue_push(const float* rows, int P, int C, float* queue, int L, int32_t* qstate, void* stream);
/* The class-aware negative mask (mask mode `class`): facl_contrast_pair_sum_mask's mode 1 (exclude) that also takes the keys of
 * clips KNOWN to share the anchor's class out of the log-sum-exp.  cls (Bk int32): one class id per key clip, >= 0 a class, < 0
 * unknown (the ids are compared, never used as an index).  For anchor clip n, myclip = n + clip_offset, column j of sim is masked
 * iff j % Bk == myclip || (cls[myclip] >= 0 && cls[j % Bk] == cls[myclip]): no member of the log-sum-exp, dsim exactly 0.  The
 * positives (same-clip columns) are read before masking and keep their gradient.  A clip may be left without any negative (a
 * batch of one class): then lse = -inf, every term of the clip and its rows of dsim, positives included, are exactly 0, nothing
 * is NaN.  With every id < 0, or all ids distinct, the outputs equal mode 1's bit for bit.  A NULL cls: FACL_E_NULL; shapes as
 * mode 1 (Bk >= 2), else FACL_E_SHAPE. */
int facl_contrast_pair_sum_cls(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                               const int32_t* cls, float* dsim, double* losses, float* losses32, void* ws, void* stream);
/* facl_contrast_pair_queue under the class-aware mask.  qcls (L int32): the class id of the clip that pushed queue row k
 * (facl_queue_push_ids); column k < valid of sim_q is masked iff cls[myclip] >= 0 && qcls[k] == cls[myclip] (dsim_q exactly 0).
 * Columns >= valid are ignored as in facl_contrast_pair_queue, whatever qcls holds there.  With an empty queue the outputs equal
 * facl_contrast_pair_sum_cls's bit for bit; with every id of cls < 0 they equal facl_contrast_pair_queue(mode 1)'s.  A NULL cls
 * or qcls: FACL_E_NULL; otherwise the domain of facl_contrast_pair_queue with mode 1.  The 16-byte kernels also need qcls
 * 16-byte aligned (else the scalar ones run). */
int facl_contrast_pair_queue_cls(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L, const int64_t* order,
                                 int clip_offset, const int32_t* cls, const int32_t* qcls, const int32_t* qstate, float* dsim,
                                 float* dsim_q, double* losses, float* losses32, void* ws, void* stream);
/* Class-mates as extra positives: facl_contrast_pair_sum_cls, and the cells it masks for a reason other than "own clip" -- the
 * clip's class cells C: (r, j) with r an anchor row of the clip, j % Bk != myclip, cls[myclip] >= 0 and cls[j % Bk] ==
 * cls[myclip] -- are positive slots against the same lse as well.  With term(p) = logaddexp(p, lse) - p and nS the clip's own
 * slots (G global, G-1 circle):  loss_n = sum_s term(pos_s) + w sum_{c in C} term(sim_c),  w = pos_weight * nS / |C| (nothing
 * added when |C| = 0).  dsim of a class cell is w * dterm/dp / B; the cells' dlse shares, times w, join the own slots' in the
 * coefficient of the negatives; |C| is not differentiated.  Own-clip columns that are no positive keep exactly 0.  Without a
 * class cell anywhere (every id < 0, or all distinct) all outputs equal mode 1's bit for bit; a clip without a negative has
 * exact zeros, class cells included.  A NULL cls: FACL_E_NULL; the shapes of facl_contrast_pair_sum_cls and a pos_weight that
 * is finite and > 0, else FACL_E_SHAPE; every refusal before any launch. */
int facl_contrast_pair_sum_sup(const float* sim, int G, int B, int Bk, int J, const int64_t* order, int clip_offset,
                               const int32_t* cls, float pos_weight, float* dsim, double* losses, float* losses32, void* ws,
                               void* stream);
/* The same on facl_contrast_pair_queue_cls: column k < valid of sim_q with cls[myclip] >= 0 && qcls[k] == cls[myclip] is a class
 * cell too (dsim_q = w * dterm/dp / B there; queue rows carry no gradient, so it moves the anchor only); columns >= valid are
 * ignored whatever qcls holds.  Three launches on one grid (chunk partials and cell counts; the cells' terms against lse; the
 * write), combined in a fixed order: same bits every run, no atomics.  With an empty queue the register-kernel shapes give
 * facl_contrast_pair_sum_sup's bits; with every id < 0 the outputs are facl_contrast_pair_queue(mode 1)'s.  Domain of
 * facl_contrast_pair_queue_cls, with 32 bytes per chunk partial instead of 12 in the workspace check; pos_weight finite and
 * > 0, else FACL_E_SHAPE. */
int facl_contrast_pair_queue_sup(const float* sim, const float* sim_q, int G, int B, int Bk, int J, int L, const int64_t* order,
                                 int clip_offset, const int32_t* cls, const int32_t* qcls, const int32_t* qstate,
                                 float pos_weight, float* dsim, float* dsim_q, double* losses, float* losses32, void* ws,
                                 void* stream);
/* Writes ids (P int32) into the slots [head, head + P) of qcls (L int32), head clamped as in facl_queue_push.  The state is
 * only read: the caller launches this BEFORE facl_queue_push in stream order, so that both see the same head.  L % P == 0, else
 * FACL_E_SHAPE (checked first); a NULL pointer: FACL_E_NULL. */
int facl_queue_push_ids(const int32_t* ids, int P, int32_t* qcls, int L, const int32_t* qstate, void* stream);
/* dst (R,J) = src scaled by *g1 in rows [0,R1) and by *g2 in rows [R1,R): the two upstream gradients (device scalars)
 * of loss_circle / loss_c applied to the shared d/dsim matrix. */
int facl_scale_rows2(const float* src, float* dst, int64_t R1, int64_t R, int J, const float* g1, const float* g2,
                     void* stream);

/* ---- F.normalize + mapping (cn3d_model_conbag.py:231-232) --------------------------------------
 * x (M,C) -> x_nor = x / max(||x||_2, 1e-12) row-wise, code (M,K) = x_nor @ Wm^T (Wm (K,C), no bias).
 * C % 4 == 0, C <= 4096, K <= 256. */
int facl_normalize_map(const float* x, int64_t M, int C, const float* Wm, int K, float* x_nor, float* code,
                       void* stream);

/* ---- OPT-IN one-shot all-reduce of a small fp64 buffer through peer-mapped mailboxes (csrc/mailbox.hip; FACL_ONESHOT_SYNCBN=1):
 * the 14 SyncBN reductions of the data-parallel step (0.1-16 KB each: the statistics the reference's single-process BatchNorm
 * layers take over the whole batch, cn3d_model_conbag.py:46-84) as ONE capturable kernel launch per rank and call instead of a
 * latency-bound RCCL collective.  Every rank allocates a mailbox (facl_mailbox_alloc: device memory + its 64-byte IPC handle),
 * opens every peer's (facl_mailbox_open), and calls facl_mailbox_allreduce in the same order: out = sum over the R ranks of
 * their `in`, added in rank order (bit-identical on every rank).  boxes: DEVICE array of R mailbox pointers, own at [rank]; seq: a
 * device uint64 that starts at 0 (the kernel advances it: a replayed graph posts fresh sequence numbers); err: device word
 * raised -- and the output poisoned with NaN -- when a peer does not post within 2 s (the wait never hangs the GPU).
 * Rehearsed with 2 / 4 processes on one GPU; cross-device visibility over xGMI is untested: never the default. */
int64_t facl_mailbox_bytes(int R, int n_max);
int facl_mailbox_alloc(int64_t bytes, void** ptr, void* handle64);
int facl_mailbox_open(const void* handle64, void** ptr);
int facl_mailbox_close(void* ptr);
int facl_mailbox_free(void* ptr);
int facl_mailbox_allreduce(const double* in, double* out, int n, int n_max, void* const* boxes, int rank, int R, uint64_t* seq,
                           uint32_t* err, void* stream);

/* ---- optimizer step (cn3d_train_motion_GL.py:180,:332: Adam, betas (0.5, 0.999), eps 1e-6, no weight decay) ------------
 * facl_adam_prep: step[0] += 1 (device float), consts = (lr[0] / (1 - b1^t), 1 / sqrt(1 - b2^t)) -- lr and the step
 * counter live on the device so that a captured HIP graph advances them by itself.
 * facl_adam_apply: ALL parameter tensors in one launch.  p / g / m / v are HOST arrays of nt <= 64 device pointers
 * (parameter, gradient, exp_avg, exp_avg_sq), n their element counts.
 * The chunk table, shared by facl_adam_apply, facl_ema_apply, facl_grad_sqnorm, facl_adamw_apply and the SGD entries below
 * (facl_tensor_sqnorms, facl_sgd_apply): the entry copies its nt <=
 * FACL_ADAM_MAX_TENSORS pointers and counts into the kernel arguments, where they travel by value (a captured graph bakes
 * them), and cuts every tensor into chunks of FACL_ADAM_CHUNK elements, one 256-thread workgroup each, the chunks of tensor 0
 * first: sum_i ceil(n[i] / FACL_ADAM_CHUNK) workgroups.  A chunk is walked 16 bytes per lane where n[i] % 4 == 0 and every
 * pointer of tensor i is 16-byte aligned, else element by element; nothing outside [0, n[i]) is touched.  A NULL array or
 * entry: FACL_E_NULL; nt outside 1..FACL_ADAM_MAX_TENSORS or an n[i] < 1: FACL_E_SHAPE; every refusal comes before the launch. */
#define FACL_ADAM_MAX_TENSORS 64
#define FACL_ADAM_CHUNK 2048
int facl_adam_prep(const float* lr, float* step, float b1, float b2, float* consts, void* stream);
int facl_adam_apply(int nt, float* const* p, const float* const* g, float* const* m, float* const* v, const int* n,
                    const float* consts, float b1, float b2, float eps, void* stream);
/* Momentum average of the key encoder (facl_amd/key_encoder.py; MoCo's param_k = param_k * m + param_q * (1 - m)):
 * pk[i][j] = m * pk[i][j] + (1 - m) * p[i][j] in fp32 (three roundings and the one of 1 - m) for ALL tensors in one launch.
 * pk / p are HOST arrays of nt <= 64 device pointers (the averaged copy, the trained parameter), n their element counts: the
 * chunk table above, with its walk and its refusals; p is only read.  m is a launch constant.  On finite data m == 0 copies p
 * and m == 1 leaves pk as it is, through the formula.  m outside [0, 1] (NaN included): FACL_E_SHAPE, before the launch. */
int facl_ema_apply(int nt, float* const* pk, const float* const* p, const int* n, float m, void* stream);

/* ---- optimizer recipe: global-norm clipping, decoupled weight decay, warm-up / cosine learning rate ---------
 * Off by default: facl_adam_prep + facl_adam_apply above stay the whole step.  With any of it on the step is
 *   [facl_grad_sqnorm, only when clipping] -> facl_adam_prep_ex -> facl_adamw_apply.
 * facl_grad_sqnorm: partial[chunk] = sum of g^2 over the chunk, in the chunk table's order (see facl_adam_apply).  g is a HOST
 *   array of nt <= 64 device pointers, n their element counts, partial a DEVICE array of sum_i ceil(n[i] / FACL_ADAM_CHUNK)
 *   doubles, every one of them written.  Each element is widened to fp64 before it is squared (the square is exact), the
 *   additions run in one fixed order (thread, wave shuffle, LDS) and no atomic takes part: the same bits from run to run,
 *   launched eagerly or replayed.  g is only read.
 * facl_adam_prep_ex: one workgroup.  step[0] += 1 (t, 1-based); norm = sqrt(partial[0] + ... + partial[npartial - 1]) in fp64,
 *   fixed order; c = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient (an infinite norm gives
 *   c = 0, a NaN norm c = NaN, as there); npartial == 0: no clipping, c = 1 exactly, norm = 0, max_norm is not read.  The learning
 *   rate of step t, in fp64: warm = min(1, t / warmup_steps) (1 when warmup_steps == 0);
 *     FACL_LR_STEP:   lr_t = warm * lr[0]                       (the host's schedule, as facl_adam_prep reads it)
 *     FACL_LR_COSINE: lr_t = warm * (lr_min + (lr[0] - lr_min) * 0.5 * (1 + cos(pi * min(t', T') / T'))),
 *                     t' = max(t - warmup_steps, 0), T' = decay_steps - warmup_steps: lr_min from step decay_steps on.
 *   consts (5 floats) = (lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t), lr_t, c, norm); the host may read the last three after a
 *   synchronisation.
 * facl_adamw_apply: facl_adam_apply on g' = c * g (consts[3]; the stored gradient is only read), and on the tensors whose
 *   decay[i] (HOST array of nt ints) is non-zero p *= 1 - lr_t * wd first (consts[2]; torch.optim.AdamW's order).  With c == 1 and
 *   wd == 0 the outputs are facl_adam_apply's bit for bit.
 * Refusals, all before the launch: a NULL array or entry (partial only when npartial > 0): FACL_E_NULL; nt outside 1..64, an
 * n[i] < 1, npartial < 0, max_norm not positive when npartial > 0, wd negative, warmup_steps < 0, lr_min negative (NaN included
 * in each), a schedule other than the two, decay_steps <= warmup_steps under FACL_LR_COSINE: FACL_E_SHAPE. */
#define FACL_LR_STEP   0
#define FACL_LR_COSINE 1
int facl_grad_sqnorm(int nt, const float* const* g, const int* n, double* partial, void* stream);
int facl_adam_prep_ex(const float* lr, float* step, float b1, float b2, const double* partial, int npartial, double max_norm,
                      int schedule, int warmup_steps, int decay_steps, double lr_min, float* consts, void* stream);
int facl_adamw_apply(int nt, float* const* p, const float* const* g, float* const* m, float* const* v, const int* n,
                     const int* decay, const float* consts, float b1, float b2, float eps, float wd, void* stream);

/* ---- SGD with momentum and LARS on the optimizer's chunk table (facl_amd/optim.py: FusedSGD) -------------------
 * The step is [facl_grad_sqnorm when clipping | facl_tensor_sqnorms under LARS] -> facl_sgd_prep -> facl_sgd_apply; plain SGD
 * is the last two.  The table, its walk and its refusals are facl_adam_apply's.
 * facl_tensor_sqnorms: partial_p[chunk] = sum of p^2 and partial_g[chunk] = sum of g^2 over the chunk, in ONE pass over both
 *   columns, in the chunk table's order; DEVICE arrays of sum_i ceil(n[i] / FACL_ADAM_CHUNK) doubles each, every entry written.
 *   The arithmetic is facl_grad_sqnorm's (widened to fp64 before the square, one fixed order, no atomic): partial_g holds the
 *   bits facl_grad_sqnorm writes for the same gradients.  p and g are only read.
 * facl_sgd_prep: one workgroup.  step[0] += 1; lr_t, c and norm by facl_adam_prep_ex's own operations (clip_on != 0: norm =
 *   sqrt(partial_g[0] + ... + partial_g[npartial - 1]), c = min(1, max_norm / (norm + 1e-6)); clip_on == 0: c = 1 exactly,
 *   norm = 0, max_norm is not read); consts (5 floats) = (lr_t, 0, lr_t, c, norm): slots 2, 3, 4 as facl_adam_prep_ex's.
 *   partial_p != NULL (LARS): n and mask are HOST arrays of nt <= 64 element counts and flags, copied into the kernel
 *   arguments as a prefix table of chunks (a captured graph bakes it); npartial must be their chunk count.  For tensor i, over
 *   its own chunks in one fixed order and in fp64, wn = sqrt(sum partial_p), gn = c * sqrt(sum partial_g), with c the fp32 value
 *   of consts[3] that facl_sgd_apply multiplies by, and
 *     trust[i] = (mask[i] && wn > 0 && gn > 0) ? eta * wn / (gn + wd * wn) : 1      rounded once to fp32
 *   (a NaN norm fails the comparisons and gives 1: the NaN reaches the parameters through the gradient itself).
 *   partial_p == NULL (plain SGD): nt, n, mask, eta, wd and trust are not read and trust is not written.
 * facl_sgd_apply: p / g / buf are HOST arrays of nt <= 64 device pointers (parameter, gradient, momentum buffer), n their
 *   element counts, mask HOST flags, trust facl_sgd_prep's ratios or NULL (q = 1).  Per element in fp32, one rounding per
 *   operation, in this order:
 *     gc = g * c;  d = mask[t] ? gc + wd * p : gc;  d = d * q;  buf = mu * buf + d;  p = p - lr_t * (nesterov ? d + mu * buf : buf)
 *   torch.optim.SGD(momentum = mu, dampening = 0, nesterov) with L2 decay on the flagged tensors; with c == 1 and q == 1 the two
 *   products are exact, and mu = 0, wd = 0 gives p - lr_t * g to the bit.  g is only read.
 * Refusals, all before the launch: a NULL array or entry: FACL_E_NULL (trust of facl_sgd_apply may be NULL; partial_p may be
 * NULL, and then n, mask and trust of facl_sgd_prep too; partial_g only when clip_on == 0 and partial_p == NULL); nt outside
 * 1..64, an n[i] < 1, mu outside [0, 1), wd, eta or lr_min negative, max_norm not positive when clipping (NaN included in
 * each), npartial < 0 or, under LARS, not the chunk count of n, warmup_steps < 0, a schedule other than the two, decay_steps <=
 * warmup_steps under FACL_LR_COSINE: FACL_E_SHAPE. */
int facl_tensor_sqnorms(int nt, const float* const* p, const float* const* g, const int* n, double* partial_p,
                        double* partial_g, void* stream);
int facl_sgd_prep(const float* lr, float* step, const double* partial_g, const double* partial_p, int npartial, int nt,
                  const int* n, const int* mask, double max_norm, int clip_on, int schedule, int warmup_steps, int decay_steps,
                  double lr_min, double eta, double wd, float* consts, float* trust, void* stream);
int facl_sgd_apply(int nt, float* const* p, const float* const* g, float* const* buf, const int* n, const int* mask,
                   const float* consts, const float* trust, float mu, float wd, int nesterov, void* stream);

/* ---- optional loss terms of the training loop (switched off in the shipped loop) ----------------------
 * facl_sinkhorn: distributed_sinkhorn + shoot_infs (cn3d_model_conbag.py:391-425).  Q (R,C) = exp(scores)^T, R prototypes
 * x C samples; `iters` row/column scalings; out (C,R).  scratch: R*C + R floats.
 * facl_kmeans: KMeans (cn3d_train_motion_GL.py:54-70): `iters` Lloyd iterations from the first K rows of x (N,D);
 * labels (N) = final assignment (first minimum on ties), cent (K,D) = final means, counts (K) (an empty cluster: 1). */
int facl_sinkhorn(const float* Q, int R, int C, int iters, float* scratch, float* out, void* stream);
int facl_kmeans(const float* x, int N, int D, int K, int iters, int32_t* labels, float* cent, int32_t* counts,
                void* stream);

/* ---- view construction of a batch of clips (replaces the NumPy pipeline of
 * training_code/cn3D_data_set.py:285-350 get_data_train + :654-663 + :708-713 + :734-749 + :767-778 and the
 * float64->float32 / permute head of cn3d_train_motion_GL.py:225-228) ----------------------------
 * src (rows,C>=8): the batch's source clouds packed row-wise (xyz, channels 3..7); idx (B,10,512): row of src for
 * every output point (views: raw, reversed, key, key-reversed, rotated x2, temporal ch4, temporal ch7, low-res x2);
 * noise (B,7,512,3): the standard-normal jitter draws in the reference's order; cossin (B,2,2): cos, sin of the two
 * rotation angles.  The host draws all of them (NumPy order) -- facl_amd/views.py.
 * out (10*B,512,4) float32, view-major (row g*B+b).  _f32/_f64 = dtype of the source arrays. */
int facl_build_views_f32(const float* src, int64_t rows, int C, const int32_t* idx, const double* noise,
                         const double* cossin, int B, float* out, void* stream);
int facl_build_views_f64(const double* src, int64_t rows, int C, const int32_t* idx, const double* noise,
                         const double* cossin, int B, float* out, void* stream);

/* ---- the same views with counter-based draws (--view_rng philox; csrc/views_philox.hip, recipe in its header and in
 * facl_amd/philox.py): Philox4x32-10 keyed by `seed`, counter (point, draw slot, clip id, epoch) -- a clip's views depend on
 * (seed, epoch, clip id) only.  Two launches per batch, no host draws:
 * meta (B,9) int32 per clip: row offsets in src of points, key points, res1, res2; their row counts (>= 1); clip id.
 * facl_views_temporal_rows_*: list (2,rows) int32 = the rows of each clip's point cloud whose channel 4 (list[0]) /
 * channel 7 (list[1]) is non-zero, at [base0 + k]; counts (B,2); *err = 1 when a count is zero (err is only raised).
 * facl_build_views_philox_*: out (10*B,512,4) float32 view-major as facl_build_views_*; a temporal view of a clip with a
 * zero count is written as zeros (void: the caller must not use the batch when *err != 0).  idx_out (B,10,512) int32 or
 * NULL: the source row of every point.  rows < 2^30. */
int facl_views_temporal_rows_f32(const float* src, int64_t rows, int C, const int32_t* meta, int B, int32_t* list,
                                 int32_t* counts, int32_t* err, void* stream);
int facl_views_temporal_rows_f64(const double* src, int64_t rows, int C, const int32_t* meta, int B, int32_t* list,
                                 int32_t* counts, int32_t* err, void* stream);
int facl_build_views_philox_f32(const float* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                const int32_t* counts, int64_t seed, int epoch, int B, float* out, int32_t* idx_out,
                                void* stream);
int facl_build_views_philox_f64(const double* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                const int32_t* counts, int64_t seed, int epoch, int B, float* out, int32_t* idx_out,
                                void* stream);
/* facl_build_views_philox_gp_*: G views of P points per clip (the reference has no recipe beyond 10 x 512; an extension of
 * this stream only).  View v is of kind k = v % 10 (the ten views above) in round r = v / 10 and draws exactly as kind k
 * does with every counter slot moved by 32*r (a round uses slots 0..25: rows 0..2, jitter 3..23, angles 24, 25); its row
 * word is word k & 3 of slot (k >> 2) + 32*r; the point index n runs over 0..P-1 in counter word 0.  A view's values do
 * not depend on G and its first P' points do not depend on P: the block [v < 10, n < 512] of any (G, P) is
 * facl_build_views_philox_*'s output bit for bit, and that entry IS this one at G = 10, P = 512 (one kernel).
 * Domain: 1 <= G <= 64; 64 <= P <= 4096 with P % 64 == 0 (the grouping limit); otherwise FACL_E_SHAPE and no launch.
 * out (G*B,P,4) float32 view-major (row v*B+b), 16-byte aligned; idx_out (B,G,P) int32 or NULL; void views (zeros,
 * idx_out -1) for the temporal kinds of EVERY round of a clip with a zero count. */
int facl_build_views_philox_gp_f32(const float* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                   const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                                   int32_t* idx_out, void* stream);
int facl_build_views_philox_gp_f64(const double* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                   const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                                   int32_t* idx_out, void* stream);

/* ---- the philox views of clips RESIDENT in device memory (--resident 1; csrc/views_resident.hip, facl_amd/resident.py):
 * the training split is loaded once into a pool and a batch is B table positions.  The views equal
 * facl_build_views_philox_*'s bit for bit (one shared implementation of the draws and the arithmetic).
 *   src    (rows_total,8) in the dataset's dtype: the clips back to back, each as points, key points, res1, res2
 *   table  int64 (n_clips,FACL_RESIDENT_REC): [0..3] row offsets in src of the four clouds, [4..7] their row counts (>= 1, a
 *          clip's rows together < 2^31), [8] clip id, [9] L = point-cloud rows of all clips before it, [10],[11] number of
 *          point-cloud rows with a non-zero channel 4 / 7 (written by facl_resident_temporal_rows_*)
 *   lists  int32 (2 * point-cloud rows of all clips): for a clip with P point-cloud rows, [2L, 2L+n4) = its rows with a
 *          non-zero channel 4 and [2L+P, 2L+P+n7) = those with a non-zero channel 7, in row order, relative to table[.][0]
 *   err    int32 (2): [0] flags, only ever raised: 1 a clip without temporal rows, 2 a selection outside [0,n_clips);
 *          [1] the smallest table position that raised flag 1 (initialise to INT32_MAX)
 * facl_resident_temporal_rows_*: the ingest pass over table records [first, first+count), once per clip, not per batch.
 * facl_build_views_resident_*: sel (B) int32 table positions, any order, repeats allowed; out (10*B,512,4) float32
 * view-major, 16-byte aligned; idx_out int64 (B,10,512) or NULL: the row of src of every point.  A selection outside the
 * table raises err, reads nothing of the pool and writes zeros (idx_out: -1) for that clip's ten views; so do the temporal
 * views of a clip whose count is zero.  All row addressing is 64-bit: rows_total has no 2^31 limit. */
#define FACL_RESIDENT_REC 12
int facl_resident_temporal_rows_f32(const float* src, int64_t* table, int32_t* lists, int first, int count, int32_t* err,
                                    void* stream);
int facl_resident_temporal_rows_f64(const double* src, int64_t* table, int32_t* lists, int first, int count, int32_t* err,
                                    void* stream);
int facl_build_views_resident_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                  const int32_t* sel, int B, int64_t seed, int epoch, float* out, int64_t* idx_out,
                                  int32_t* err, void* stream);
int facl_build_views_resident_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                  const int32_t* sel, int B, int64_t seed, int epoch, float* out, int64_t* idx_out,
                                  int32_t* err, void* stream);
/* facl_build_views_resident_gp_*: G views of P points per clip out of the pool, by facl_build_views_philox_gp_*'s recipe
 * (kind v % 10, round v / 10, slots + 32*round, n in 0..P-1) and equal to its output bit for bit.  Same domain: 1 <= G <= 64;
 * 64 <= P <= 4096 with P % 64 == 0; otherwise FACL_E_SHAPE and no launch.  out (G*B,P,4) float32 view-major, 16-byte
 * aligned; idx_out int64 (B,G,P) or NULL.  A selection outside the table voids all G views of that clip, a zero temporal
 * count the temporal kinds of every round.  facl_build_views_resident_* is this entry at G = 10, P = 512 (one kernel). */
int facl_build_views_resident_gp_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                     const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                     int64_t* idx_out, int32_t* err, void* stream);
int facl_build_views_resident_gp_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                     const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                     int64_t* idx_out, int32_t* err, void* stream);

/* ---- the philox views by a RECIPE: which kinds a round holds and how strongly they are augmented (csrc/views_point.inc;
 * restated by facl_amd/philox.py's Recipe).  A recipe is a list of 1..FACL_VIEW_POS_MAX kind codes, the positions of a round,
 * and FACL_VIEW_NSTRENGTH strengths.  View v is of the kind at position v % n_kinds in round v / n_kinds.
 *   kinds      RAW, MIRROR, KEY, KEY_MIRROR, ROT, T4, T7, RES30, RES10: the reference's views (the default list is RAW, MIRROR,
 *              KEY, KEY_MIRROR, ROT, ROT, T4, T7, RES30, RES10).  JITTER: the jittered point cloud.  SCALE: jitter, then xyz * s,
 *              s = scale_lo + (scale_hi - scale_lo) * u.  TILT_NEG / TILT_POS: jitter, then a rotation about y by -/+ pi *
 *              tilt_angle
 *   strengths  [0] jitter_sigma 0.01, [1] jitter_clip 0.05, [2] rot_range 0.8 (the angle of ROT is (u - 0.5) * pi * rot_range),
 *              [3] scale_lo 0.5, [4] scale_hi 1.5, [5] tilt_angle 0.25; each applies to every position of the recipe
 *   slots      row word of position i: word i & 3 of slot i >> 2.  Jitter draws are numbered j = 0, 1, ... in position order
 *              (MIRROR and KEY_MIRROR take two; KEY, ROT, JITTER, SCALE, TILT_* one) and draw j uses slots 3 + 3 j + d.  The
 *              scalar draws of ROT and SCALE are numbered in position order from 3 + 3 max(7, J), J = jitter draws of the round.
 *              A round takes `stride` = 32 ceil((3 + 3 max(7, J) + A) / 32) slots, A = its scalar draws.  So a view's draws
 *              depend on the kinds BEFORE it in the list; the default list gives the layout of the _gp entries above.
 * facl_build_views_philox_recipe_* / facl_build_views_resident_recipe_*: the _gp entries with a recipe; every entry above IS
 * this one at the default recipe (one kernel), bit for bit.  The recipe travels in the kernel's arguments.  Same domain of
 * (G, P): 1 <= G <= 64; 64 <= P <= 4096 with P % 64 == 0; otherwise FACL_E_SHAPE and no launch.
 * `kinds` AND `strengths` ARE HOST POINTERS, READ BEFORE THE LAUNCH; EVERY OTHER POINTER OF THIS ABI IS A DEVICE POINTER.
 * Refused without a launch: NULL kinds / strengths: FACL_E_NULL; n_kinds outside 1..12, an unknown kind code, a strength
 * that is not finite, jitter_sigma < 0, jitter_clip <= 0, rot_range outside [0, 2], scale_lo <= 0 or scale_lo > scale_hi:
 * FACL_E_SHAPE.  A temporal kind at any position keeps the void-view behaviour (zeros, idx_out -1, err raised).
 * facl_view_recipe_table: HOST ONLY, no HIP call.  table (n_kinds, FACL_VIEW_TABLE_COLS) int32 per position: source (0..3 the
 * four clouds, 4 / 5 the rows with a non-zero channel 4 / 7), channel copied to output channel 3, operation (0 gather, 1 jitter,
 * 2 mirror, 3 rot, 4 scale, 5 tilt_neg, 6 tilt_pos), row slot, row word, first and second jitter draw j (-1: none), scalar
 * slot (-1: none); *stride = the slots of a round.  All three pointers are host pointers. */
#define FACL_VIEW_RAW        0
#define FACL_VIEW_MIRROR     1
#define FACL_VIEW_KEY        2
#define FACL_VIEW_KEY_MIRROR 3
#define FACL_VIEW_ROT        4
#define FACL_VIEW_T4         5
#define FACL_VIEW_T7         6
#define FACL_VIEW_RES30      7
#define FACL_VIEW_RES10      8
#define FACL_VIEW_JITTER     9
#define FACL_VIEW_SCALE      10
#define FACL_VIEW_TILT_NEG   11
#define FACL_VIEW_TILT_POS   12
#define FACL_VIEW_NKINDS     13
#define FACL_VIEW_POS_MAX    12
#define FACL_VIEW_NSTRENGTH  6
#define FACL_VIEW_TABLE_COLS 8
int facl_build_views_philox_recipe_f32(const float* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                       const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                                       int32_t* idx_out, const int32_t* kinds, int n_kinds, const double* strengths,
                                       void* stream);
int facl_build_views_philox_recipe_f64(const double* src, int64_t rows, int C, const int32_t* meta, const int32_t* list,
                                       const int32_t* counts, int64_t seed, int epoch, int B, int G, int P, float* out,
                                       int32_t* idx_out, const int32_t* kinds, int n_kinds, const double* strengths,
                                       void* stream);
int facl_build_views_resident_recipe_f32(const float* src, const int64_t* table, const int32_t* lists, int n_clips,
                                         const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                         int64_t* idx_out, int32_t* err, const int32_t* kinds, int n_kinds,
                                         const double* strengths, void* stream);
int facl_build_views_resident_recipe_f64(const double* src, const int64_t* table, const int32_t* lists, int n_clips,
                                         const int32_t* sel, int B, int G, int P, int64_t seed, int epoch, float* out,
                                         int64_t* idx_out, int32_t* err, const int32_t* kinds, int n_kinds,
                                         const double* strengths, void* stream);
int facl_view_recipe_table(const int32_t* kinds, int n_kinds, int32_t* table, int32_t* stride);

/* ---- 3DV generation: depth frames -> motion, key and appearance clouds (generate_data/generate_NTU.py; csrc/gen3dv.hip,
 * whose header describes the stages and the layouts) for a batch of B clips.  int32 unless said otherwise:
 *   frames uint16 (NF,H,W): per clip the first file of its folder, then its chosen frames (at most FACL_GEN3DV_MAX_FRAMES)
 *   fmeta  (NF,4): clip; index among the clip's chosen frames, -1 for the first file; the frame before it in the motion
 *          chain (:140-150); offset of its pixel list in pix (exclusive scan of fcount over the chosen frames)
 *   fbox   (NF,4): rows [60,rhi) and columns [clo,chi) survive load_depth_from_img (:339-351); [3] = frame has a pixel
 *   fcount (NF): pixels kept;  fext float64 (NF,6): min xyz, max xyz of their back-projection (+-inf when none)
 *   cmin   float64 (B,3), cgrid (B,4) = nx, ny, nz, voxel offset: the clip's grid (:165-181), voxel (x*ny+y)*nz+z
 *   occ, mocc uint64 (NV), ZEROED by the caller: bit i = chosen frame i has a point / a motion point in the voxel
 *   pix    (NP): the kept pixels of every chosen frame, row-major;  wtab (B,5,64): weight of frame i in channel m (:409-438)
 *   vol    (5,NV) channel planes, key (NV); vol0f, keyf (NV): disca_voxel (:277-296) of channel 0 / of key
 *   lists  (12*NV): per clip at 12*offset the (m,x,y,z)-ordered hits (5V), the sorted unique voxels (V), and the same two
 *          under the key mask (:196-201, :212-219), as voxel numbers;  counts (B,4) in that order
 *   idx    (B,2,2048) rows of the list the reference samples from (hits > 2048: the unique list), or NULL: Philox4x32-10
 *          keyed by seed, counter (row, slot, crc[b], resolution) -- recipe in csrc/gen3dv.hip; crc uint32 (B)
 *   out_raw, out_key float64 (B,2048,8); norm float64 (B,14): centres, y_len, c_min[5], c_len[5] (:232-240)
 *   ameta  (NA,3): frame, clip, slot of an appearance frame; idx (NA,2048) ranks among the frame's kept pixels or NULL;
 *          out float64 (NA,2048,4) (:61-73, :249-260)
 *   err    a word of flags, only ever raised: 1 a point outside its grid, 2 pixel list overrun, 4 bad fmeta / ameta row,
 *          8 an empty list or frame, 16 a drawn index out of range.  Nothing is written out of bounds in any of these cases.
 * maxF = the largest number of chosen frames of a clip, maxvox = the largest nx*ny*nz.  FACL_E_SHAPE beyond the limits
 * below (never truncated). */
#define FACL_GEN3DV_MAX_FRAMES        64           /* chosen frames per clip: one bit each            */
#define FACL_GEN3DV_MAX_FRAMES_TOTAL  (1 << 16)    /* frames (NF) / appearance frames (NA) per batch  */
#define FACL_GEN3DV_MAX_PIXELS        (1 << 22)    /* H * W                                           */
#define FACL_GEN3DV_MAX_CLIPS         4096         /* B                                               */
#define FACL_GEN3DV_MAX_VOXELS        (1 << 24)    /* nx * ny * nz of one clip                        */
#define FACL_GEN3DV_MAX_VOXELS_TOTAL  (1 << 27)    /* NV                                              */
int facl_gen3dv_frames(const uint16_t* frames, int NF, int H, int W, int32_t* fbox, int32_t* fcount, double* fext,
                       void* stream);
int facl_gen3dv_voxelise(const uint16_t* frames, int NF, int H, int W, const int32_t* fbox, const int32_t* fmeta,
                         const double* cmin, const int32_t* cgrid, int B, int maxF, int maxvox, int64_t NV, int64_t NP,
                         double voxel, uint64_t* occ, uint64_t* mocc, int32_t* pix, int32_t* err, void* stream);
int facl_gen3dv_volumes(const uint64_t* occ, const uint64_t* mocc, const int32_t* wtab, const int32_t* cgrid, int B,
                        int maxvox, int64_t NV, int32_t* vol, int32_t* key, void* stream);
int facl_gen3dv_filter(const int32_t* vol, const int32_t* key, const int32_t* cgrid, int B, int maxvox, int64_t NV,
                       int th_all, int th_key, int32_t* vol0f, int32_t* keyf, void* stream);
int facl_gen3dv_compact(const int32_t* vol, const int32_t* vol0f, const int32_t* keyf, const int32_t* cgrid, int B,
                        int maxvox, int64_t NV, int32_t* lists, int32_t* counts, void* stream);
int facl_gen3dv_sample(const int32_t* vol, const int32_t* vol0f, const int32_t* lists, const int32_t* counts,
                       const int32_t* cgrid, int B, int maxvox, int64_t NV, const int32_t* idx, int64_t seed,
                       int resolution, const uint32_t* crc, double* out_raw, double* out_key, double* norm, int32_t* err,
                       void* stream);
int facl_gen3dv_app(const uint16_t* frames, int NF, int H, int W, const int32_t* fmeta, const int32_t* fcount,
                    const int32_t* pix, int64_t NP, const int32_t* ameta, int NA, const int32_t* idx, int64_t seed,
                    int resolution, const uint32_t* crc, const double* cmin, const int32_t* cgrid, int B, int maxvox,
                    int64_t NV, double voxel, const int32_t* vol0f, const double* norm, double* out, int32_t* err,
                    void* stream);

/* ---- weighted k-nearest-neighbour evaluation of frozen features (csrc/knn.hip) -----------------------------
 * The reference has no counterpart: this is the standard cheap complement of its linear probe (linear_classify/linercls.py),
 * cosine similarity between L2-normalised feature rows and an exp(s / T)-weighted vote of the k nearest bank rows.
 *
 * facl_knn_topk: for every query row the k bank rows of largest cosine similarity.
 *   q (nq, C) fp32 rows ldq floats apart; x (nb, C) fp32 rows ldx floats apart (the bank)
 *   self_idx  int32 (nq) or NULL: the bank row that query must not return (-1: none) -- leave-one-out of a split against itself
 *   top_val   (nq, k) fp32 cosine similarities, non-increasing along a row;  top_idx (nq, k) int32 bank rows
 *   ws        facl_knn_ws_bytes(nq, nb, k) bytes, 16-byte aligned; contents are scratch
 * Rows are normalised as F.normalize does (x / max(||x||, 1e-12), the norm taken in fp64) by a row pre-pass whose factors the
 * GEMM epilogue applies: no normalised copy of either operand is made.  The similarities are an fp16x3 exact-split GEMM
 * (each row scaled by its own power of two) with fp32 accumulation: fp32-GEMM accuracy.  Equal similarities are ordered by
 * the lower bank index, and the result is the same bits from run to run: the order (similarity descending, index ascending)
 * is total, every partial list is the k best under it, and no atomic takes part.  A similarity that is NaN is never
 * returned; should fewer than k rows remain, the tail of the row is (-inf, -1).
 * Domain: nq, nb >= 1; 1 <= k <= 64; C a positive multiple of 64; ldq, ldx >= C and multiples of 4; nb - (self_idx ? 1 : 0)
 * >= k (a non-NULL self_idx counts as set); else FACL_E_SHAPE.  NULL q / x / outputs / ws: FACL_E_NULL.  q, x, ws not
 * 16-byte aligned: FACL_E_ALIGN.
 * facl_knn_ws_bytes: 8 (nq + nb) bytes of row factors + 8 nq k splits bytes of partial lists, where splits (1 when the query
 * tiles alone fill the device, up to nb / 128 for a handful of queries) is fixed by (nq, nb); never O(nq nb).  FACL_E_SHAPE
 * outside the domain of (nq, nb, k). */
int64_t facl_knn_ws_bytes(int nq, int nb, int k);
int facl_knn_topk(const float* q, int nq, int ldq, const float* x, int nb, int ldx, int C, int k, const int32_t* self_idx,
                  float* top_val, int32_t* top_idx, void* ws, void* stream);

/* facl_knn_vote: scores[i][c] = sum over the neighbours j of query i with labels[top_idx[i][j]] == c of
 * exp(top_val[i][j] * inv_T), added in the order j = 0..k-1 (no atomics); pred[i] = argmax_c, the lower class on equal scores.
 *   labels int32 (nb), each in [0, num_class); pred int32 (nq); scores (nq, num_class) fp32 or NULL
 * A neighbour whose index is outside [0, nb) or whose label is outside [0, num_class) adds nothing.  One launch.
 * Domain: nq, nb >= 1; 1 <= k <= 64; 1 <= num_class <= 1024; else FACL_E_SHAPE. */
int facl_knn_vote(const float* top_val, const int32_t* top_idx, const int32_t* labels, int nq, int nb, int k, int num_class,
                  float inv_T, int32_t* pred, float* scores, void* stream);

/* ---- classifier head of supervised fine-tuning (csrc/cls.hip) ------------------------------------------------
 * The probe head of the reference (linear_classify/fc_model.py:12-25, Final_FC: F.normalize(x, dim=1) then Linear) on the
 * model's own output layout, and the softmax cross-entropy of its logits.  The Linear layer is facl_gemm_fwd / dgrad / wgrad.
 * No entry synchronises, allocates or uses an atomic: each can be captured in a graph and returns the same bits every run.
 *
 * facl_cls_gather_norm_fwd: `stacked` (G*B + B, C) is the FC head's stacked, view-major output: row g*B + b = view g of clip
 * b, row G*B + b = the clip's global feature.  out (B, (G+1)*C) = the clip-major vector [x_view0 .. x_view(G-1), x_global] of
 * every clip times inv_norm[b] = 1 / max(||vector||, 1e-12) (F.normalize's clamp; the sum of squares is taken in fp64 in a fixed
 * order).  The G + 1 rows of a clip are read in place: no permute / cat copy exists.  One workgroup per clip.
 * facl_cls_gather_norm_bwd: dstacked[g*B + b] = inv_norm[b] * (dout[b][g] - out[b][g] * <dout[b], out[b]>), the dot product in
 * fp64 in a fixed order; EVERY row of dstacked (G*B + B, C) is written.  dout, out (B, (G+1)*C).
 * Domain: C a multiple of 64 in 64..1024; 1 <= G <= 64; B >= 1; else FACL_E_SHAPE.  A NULL pointer: FACL_E_NULL.  stacked, out,
 * dout, dstacked not 16-byte aligned: FACL_E_ALIGN. */
int facl_cls_gather_norm_fwd(const float* stacked, int G, int B, int C, float* out, float* inv_norm, void* stream);
int facl_cls_gather_norm_bwd(const float* dout, const float* out, const float* inv_norm, int G, int B, int C, float* dstacked,
                             void* stream);

/* facl_softmax_ce: mean cross-entropy of R rows of logits (rows ld floats apart, ncls classes) against int32 labels, the row
 * maximum subtracted and the exponentials summed in fp64.
 *   loss     (1) fp32: (sum of the row losses) / R
 *   dlogits  (R, ncls) fp32 contiguous, or NULL: (softmax - onehot) / R
 *   stats    int32 (2): [0] rows whose argmax equals the label (the lowest class on equal logits), [1] rows whose label lies
 *            outside [0, ncls): such a row adds no loss, no gradient (its dlogits row is zero) and no hit, and still counts in R
 *   ws       the partial-sum workspace (facl_ws_bytes(), 8-byte aligned): 12 R bytes of row losses and flags; scratch
 * One wave per row writes the row's loss and flags to the workspace; a second launch of ONE wave sums them in a fixed order
 * in fp64, so the mean does not depend on scheduling.
 * Domain: 2 <= ncls <= 1024; R >= 1 with 12 R bytes inside the workspace; ld >= ncls; else FACL_E_SHAPE.  NULL logits /
 * labels / loss / stats / ws: FACL_E_NULL. */
int facl_softmax_ce(const float* logits, int ld, const int32_t* labels, int R, int ncls, float* loss, float* dlogits,
                    int32_t* stats, void* ws, void* stream);

/* ---- prediction with a trained head (csrc/predict.hip) ----------------------------------------------------------
 * Class probabilities of a head's logits, accumulated over test-time draws of the views in fp64, and the k most probable
 * classes of every row with the rank of its label.  One wave per row, lanes striding over the classes.  No entry synchronises,
 * allocates or uses an atomic; each returns the same bits every run.
 *
 * facl_cls_probs_acc: p[i][c] = exp(x[i][c] - max_i) / sum_c exp(x[i][c] - max_i) of R rows of logits (rows ld floats apart,
 * ncls classes); the differences, the exponentials, their sum (lane partial sums, then the xor tree) and the quotient in fp64.
 *   acc   (R, ncls) fp64 contiguous: first != 0 stores acc[i][c] = p (whatever acc held, NaN included); first == 0 stores
 *         acc[i][c] + p.  The sum over the draws is then the caller's: draw 0 with first = 1, every later draw with first = 0.
 * A logit of -inf gives p = 0.  A row whose maximum is not finite -- a NaN logit anywhere in it, a +inf logit, or nothing but
 * -inf -- makes the whole acc row NaN, and it stays NaN through the later draws.
 * Domain: 2 <= ncls <= 1024; R >= 1; ld >= ncls; else FACL_E_SHAPE.  NULL logits / acc: FACL_E_NULL.  acc not 8-byte aligned:
 * FACL_E_ALIGN. */
int facl_cls_probs_acc(const float* logits, int ld, int R, int ncls, double* acc, int first, void* stream);

/* facl_cls_topk: for every row of acc the k classes of largest acc under the total order (value descending, class ascending).
 *   top_p   (R, k) fp32: (float)(acc / ndraws), the fp64 quotient rounded once; non-increasing along a row
 *   top_c   (R, k) int32 classes
 *   labels  int32 (R) or NULL;  rank int32 (R), required with labels and ignored without them: rank[i] = the number of classes
 *           that precede labels[i] in that order over ALL ncls classes, so 0 is a top-1 hit and rank < j a top-j hit for any j
 *           (k plays no part in it); -2 for a label outside [0, ncls)
 * A row of acc that holds a NaN gives top_c = -1 and top_p = NaN in all its k entries and rank = -1 (whatever its label is).
 * Lane e of the row's wave ends up with list entry e: k rounds of a wave argmax over the lanes' <= 16 classes each.
 * Domain: 2 <= ncls <= 1024; R >= 1; 1 <= k <= min(ncls, 64); ndraws >= 1; else FACL_E_SHAPE.  NULL acc / top_p / top_c, or
 * labels without rank: FACL_E_NULL.  acc not 8-byte aligned: FACL_E_ALIGN. */
int facl_cls_topk(const double* acc, int R, int ncls, int ndraws, int k, const int32_t* labels, float* top_p, int32_t* top_c,
                  int32_t* rank, void* stream);

/* ---- spherical k-means over frozen features: the centroid update (csrc/cluster.hip) ----------------------------
 * The reference has no counterpart: clustering accuracy / NMI / ARI are the standard label-free complement of its linear probe,
 * and cluster ids stand in for action labels in the class-aware loss modes.  The ASSIGNMENT step of a Lloyd iteration is
 * facl_knn_topk with q = x, the centroids as the bank, k = 1 and self_idx = NULL; these entries are the UPDATE step.
 *   x (n, C) fp32 rows ldx floats apart (a column slice of a wider matrix is read in place)
 *
 * facl_cluster_row_inv: inv[i] = fp32(1 / max(||x_i||, 1e-12)), the sum of squares in fp64 in a fixed order (one wave per row).
 * Run once per clustering.  Domain: n >= 1; C a positive multiple of 64; ldx >= C and a multiple of 4; else FACL_E_SHAPE.  NULL x /
 * inv: FACL_E_NULL.  x not 16-byte aligned: FACL_E_ALIGN.
 *
 * facl_cluster_sums: for every cluster c with offs[c+1] > offs[c]
 *     cent[c][j] = fp32( sum over r = offs[c] .. offs[c+1]-1, in that order, of double(x[order[r]][j]) * double(inv[order[r]]) ),
 * the UN-normalised sum (facl_knn_topk normalises bank rows itself).  A cluster without rows leaves its row of cent untouched.
 *   order  int32 (n): the row indices sorted by label, ascending row index inside a label
 *   offs   int32 (K+1): the label boundaries, 0 = offs[0] <= offs[1] <= ... <= offs[K] = n
 *   cent   (K, C) fp32 contiguous
 *   err    one int32 of flags, only ever raised: 1 an entry of order outside [0, n) -- that row is skipped and never
 *          dereferenced; 2 boundaries that are not as above -- then no row is read and cent is left as it is
 *   ws     facl_cluster_ws_bytes(n, K, C) bytes, 16-byte aligned; contents are scratch
 * A cluster is cut into segments of 128 rows of order; a first launch writes each segment's fp64 partial sums to ws, a second
 * adds a cluster's segments in segment order and rounds once.  No floating-point atomic takes part and the order of every sum
 * is fixed by (n, order, offs): the same bits every run.
 * Domain: n >= 1; 1 <= K <= 1024 (facl_knn_vote's class limit); C, ldx as above; else FACL_E_SHAPE.  A NULL pointer:
 * FACL_E_NULL.  x, cent or ws not 16-byte aligned: FACL_E_ALIGN.  Every refusal comes before any launch.
 * facl_cluster_ws_bytes: 4 (K + 1) bytes of segment offsets, rounded up to 256, + 8 C (n / 128 + K) bytes of partial sums.
 * FACL_E_SHAPE outside the domain of (n, K, C). */
int64_t facl_cluster_ws_bytes(int n, int K, int C);
int facl_cluster_row_inv(const float* x, int n, int ldx, int C, float* inv, void* stream);
int facl_cluster_sums(const float* x, int n, int ldx, int C, const float* inv, const int32_t* order, const int32_t* offs, int K,
                      float* cent, int32_t* err, void* ws, void* stream);

/* ---- prototype contrastive term on the k-means centroids (csrc/proto.hip) ------------------------------------------
 * The reference has no counterpart: ProtoNCE (Li et al. 2021, "Prototypical Contrastive Learning") on the centroids that
 * --class_ids cluster computes anyway.  With z_r = x_r / max(||x_r||, 1e-12), p_k = c_k proto_inv_k, l_rk = scale_k <z_r, p_k> and
 * s_r = classes[r % B]:
 *   loss     = (1/M) sum over the rows with 0 <= s_r < K of [logsumexp_k l_rk - l_{r,s_r}]      (the division is by M: a row of
 *              unknown class adds nothing and still counts, facl_softmax_ce's convention)
 *   dstacked = d loss / d stacked: row r = inv_r (dz_r - z_r <dz_r, z_r>) with dz_r = sum_k (softmax_k(l_r.) - [k = s_r]) / M scale_k p_k,
 *              exact zeros in the other rows.  The prototypes are constants: they get no gradient.
 *   stacked   (M, C) float32, row stride ld; row r belongs to clip r % B (view-major rows, the clips' global rows last)
 *   classes   (B) int32; < 0: unknown.  An id >= K raises bit 0 of err[0] (an integer OR: the caller zeroes err once and may
 *             read it whenever it likes); the row is treated as unknown and the id indexes nothing
 *   protos    (K, C) float32 contiguous, un-normalised;  proto_inv (K) = 1 / max(||c_k||, 1e-12);  scale (K) = 1 / phi_k > 0
 *   loss      (1) float32;  dstacked (M, C) float32 contiguous;  ws facl_proto_nce_ws_bytes(M) bytes, contents are scratch
 * One launch does everything per tile of 16 rows on the exact f32-input MFMA (sums of squares, sum of exp and the projection
 * in fp64), a second one (one wave) adds the tiles' loss sums in a fixed order.  No floating-point atomic: equal inputs give
 * equal bits.  With every class unknown the loss is +0.0 and dstacked all zero bits.
 * Domain: M >= 1, B >= 1, M % B == 0; 1 <= K <= 1024; C a multiple of 64 in 64..512; ld >= C and a multiple of 4; else
 * FACL_E_SHAPE.  A NULL pointer: FACL_E_NULL.  stacked, protos, proto_inv, scale, dstacked or ws not 16-byte aligned:
 * FACL_E_ALIGN.  Every refusal comes before any launch.
 * facl_proto_nce_ws_bytes: 8 ceil(M / 16) bytes, rounded up to 256; FACL_E_SHAPE for M < 1. */
int64_t facl_proto_nce_ws_bytes(int M);
int facl_proto_nce(const float* stacked, int M, int ld, int C, int B, const int32_t* classes, const float* protos,
                   const float* proto_inv, const float* scale, int K, float* loss, float* dstacked, int32_t* err, void* ws,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FACL_HIP_H */
