/* anncur_hip.h -- C ABI of libanncur_hip.so: the MI355X (gfx950) kernels behind the
 * CUR nearest-neighbour path of iesl/anncur.
 *
 * The reference is pure Python with no FFI of its own; the symbols below are what a
 * binding for this path binds (ctypes).  Each entry point cites
 * the reference interface (file:line, relative to the upstream repo) it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (ANNCUR_E_*); the message is
 *    available from anncur_last_error() (thread-local);
 *  - the caller owns every buffer; pointers are DEVICE pointers unless stated;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *    asynchronous on that stream; no hidden allocation, no host synchronisation:
 *    scratch comes from an explicit workspace sized by the *_workspace_bytes() query; every call can be captured into a HIP graph
 *    and replayed on other data in the same buffers (tests/test_gpu_graph_replay.py) -- with ONE EXCEPTION: the fused top-k at Kp > 512
 *    (the wide route of anncur_score_topk / _ex and anncur_eval_topk), whose replay on a workspace overwritten since the capture ended in
 *    a GPU memory fault; its cause is supposed, not established, so capture it only if nothing else writes the workspace;
 *    the calls documented to synchronise (_timed, _survivors, _ladder_state) cannot be captured at all;
 *  - matrices are row-major; `ld*` are leading dimensions in ELEMENTS;
 *  - dtype codes: ANNCUR_F32 (float) / ANNCUR_BF16 (bfloat16, 2 bytes);
 *  - top-k results are sorted by score descending, ties broken by the smaller index
 *    (torch.topk leaves tie order unspecified; this is one valid order);
 *  - NaN scores are never selected.
 */
#ifndef ANNCUR_HIP_H
#define ANNCUR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANNCUR_F32  0
#define ANNCUR_BF16 1
#define ANNCUR_F64  2            /* only the fp64 helpers of the on-device pseudo-inverse take it */

#define ANNCUR_OK            0
#define ANNCUR_E_INVALID    -1   /* bad argument (shape, dtype, alignment, k range) */
#define ANNCUR_E_WORKSPACE  -2   /* workspace missing or too small */
#define ANNCUR_E_HIP        -3   /* a HIP runtime call / kernel launch failed */
#define ANNCUR_E_UNSUPPORTED -4  /* valid request outside what this build implements */

#define ANNCUR_MAX_TOPK 2048     /* largest k accepted by the top-k entry points */

/* library / diagnostics ------------------------------------------------------------ */
int         anncur_version(void);            /* 1000*major + minor */
const char *anncur_last_error(void);         /* thread-local, never NULL */
int         anncur_device_info(int *n_cu, int *wave_size, char *arch_name, int arch_name_len);

/* a2: anchor row / column gather ---------------------------------------------------
 * rows = A[row_idxs,:], cols = A[:,col_idxs]
 *   eval/run_retrieval_eval_wrt_exact_crossenc.py:73-74
 *   eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py:297,300
 * src and dst share `dtype` unless dst_dtype says otherwise (F32<->BF16 convert on the fly).
 * idx are int32 device arrays; out-of-range indices are an error reported lazily as
 * zeros (the Python layer validates indices on the host before calling). */
int anncur_gather_cols(const void *A, int dtype, int64_t n_rows, int64_t n_cols, int64_t lda,
                       const int32_t *col_idx, int32_t n_idx,
                       void *out, int dst_dtype, int64_t ldo, void *stream);
int anncur_gather_rows(const void *A, int dtype, int64_t n_rows, int64_t n_cols, int64_t lda,
                       const int32_t *row_idx, int32_t n_idx,
                       void *out, int dst_dtype, int64_t ldo, void *stream);

/* a4/a5/a6: strided GEMM with exact-fp32 accumulation ------------------------------
 * C(m,n) = sum_k A(m,k) * B(k,n), element (i,j) of an operand at base + i*s0 + j*s1
 * (strides in elements), so NN / NT / TN / transposed-output products are one call.
 * Inputs F32 or BF16 (up-converted exactly), products and sums in fp32 on the matrix
 * cores (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fmaf chain).  Subnormal numbers are numbers here: subnormal fp32 and bf16
 * operands are read as they are, every subnormal partial sum is kept and rounded to nearest even like any other, and a bf16 C is one
 * more such rounding, into bf16's subnormals (measured on gfx950, tests/test_gpu_subnormal_exact.py; no kernel of this library is built
 * with a flushing denormal mode, tests/test_cpu_denorm_mode.py).  Replaces
 *   latent_cols = U @ R                      eval/matrix_approx_zeshel.py:65
 *   latent_rows = C @ U                      eval/matrix_approx_zeshel.py:61
 *   get / get_rows / get_cols / get_complete_row / get_complete_col
 *                                             eval/matrix_approx_zeshel.py:74,79,85,97,118
 *   pinv(C) @ A @ pinv(R)                    eval/matrix_approx_zeshel.py:47 (the two products)
 *   mention_embeds @ label_embeds.T          ..._w_fixed_train_test_splits.py:283 */
int anncur_gemm(const void *A, int a_dtype, int64_t a_sm, int64_t a_sk,
                const void *B, int b_dtype, int64_t b_sk, int64_t b_sn,
                void *C, int c_dtype, int64_t c_sm, int64_t c_sn,
                int64_t M, int64_t N, int64_t K, void *stream);

/* Same product with scaling and accumulation: C = alpha * A.B + beta * Cin (Cin fp32 with its own strides, may be NULL; it may
 * alias C element for element); a subnormal accumulator, a subnormal Cin and a subnormal result are kept, none is flushed.
 * Building block of the on-device pseudo-inverse (Newton-Schulz X <- 2X - (X W) X), the
 * alternative to the host numpy.linalg.pinv of eval/matrix_approx_zeshel.py:47,49 for large anchor counts. */
int anncur_gemm_ex(const void *A, int a_dtype, int64_t a_sm, int64_t a_sk,
                   const void *B, int b_dtype, int64_t b_sk, int64_t b_sn,
                   void *C, int c_dtype, int64_t c_sm, int64_t c_sn,
                   int64_t M, int64_t N, int64_t K, float alpha, float beta,
                   const float *Cin, int64_t i_sm, int64_t i_sn, void *stream);
/* out[0] = sum of squares of an fp32 matrix (Frobenius norm squared); dst(i,j) = alpha / (divide_by ? divide_by[0] : 1) * src(i,j)
 * with arbitrary strides (scaled transpose).  Helpers of the on-device pseudo-inverse; no host synchronisation.
 * anncur_sumsq combines its waves' partial sums by atomic adds, in the order they finish: the last bits of out[0] differ from call to call.
 * anncur_sumsq_ordered adds in an order that depends on the shape alone (one partial per workgroup in `partials`, ANNCUR_SUMSQ_PARTIALS
 * floats of caller-owned workspace, nothing pre-filled, then one workgroup over them): equal inputs give equal bits.  pinv.py scales and
 * stops its fp32 iteration by this sum, so it takes the ordered one.  Subnormal squares and sums are kept by both; anncur_scale_copy's
 * factor is the IEEE quotient alpha / divide_by[0], a subnormal one included, and a subnormal product is stored as it is. */
#define ANNCUR_SUMSQ_PARTIALS 1024
int anncur_sumsq(const float *A, int64_t n_rows, int64_t n_cols, int64_t lda, float *out, void *stream);
int anncur_sumsq_ordered(const float *A, int64_t n_rows, int64_t n_cols, int64_t lda, float *partials, float *out, void *stream);
int anncur_scale_copy(const float *src, int64_t s0, int64_t s1, float *dst, int64_t d0, int64_t d1, int64_t M, int64_t N,
                      float alpha, const float *divide_by, void *stream);

/* fp64 building blocks of the PARITY-GRADE on-device pseudo-inverse (anncur_amd/pinv.py, Newton-Schulz X <- X (2 I - W X) in
 * double precision, rounded to fp32 once at the end): replaces the host call
 *   U = numpy.linalg.pinv(W)                 eval/matrix_approx_zeshel.py:47,49
 * when the caller asks for it (pinv_backend "device" / "auto").  Strided like anncur_gemm_ex; products and sums in fp64 on
 * v_mfma_f64_16x16x4_f64.  anncur_convert_f64: dst(i,j) = (alpha * src(i,j)) / divide_by[0] in fp64 -- one rounded product, then one rounded
 * division, in that order (pinv.py's results depend on it) -- or alpha * src(i,j) where divide_by is NULL, for the dtype pairs
 * F32->F64, BF16->F64 (widened exactly, denormals included), F64->F64 (scaled copy / transpose) and F64->F32 (one more rounding, to
 * nearest even); any other pair is ANNCUR_E_INVALID and writes nothing, M * N == 0 returns without a launch.  anncur_diff_sumsq_f64:
 * out2 = {sum (x - y)^2, sum x^2} over n contiguous doubles (y may be NULL), device doubles, no host synchronisation. */
int anncur_gemm_f64(const double *A, int64_t a_sm, int64_t a_sk, const double *B, int64_t b_sk, int64_t b_sn,
                    double *C, int64_t c_sm, int64_t c_sn, int64_t M, int64_t N, int64_t K,
                    double alpha, double beta, const double *Cin, int64_t i_sm, int64_t i_sn, void *stream);
int anncur_convert_f64(const void *src, int src_dtype, int64_t s0, int64_t s1, void *dst, int dst_dtype, int64_t d0, int64_t d1,
                       int64_t M, int64_t N, double alpha, const double *divide_by, void *stream);
int anncur_diff_sumsq_f64(const double *X, const double *Y, int64_t n, double *out2, void *stream);

/* a11: approximation error without materialising S_hat ------------------------------
 * err_sq[q] = sum_i (X[q,:].E[:,i] - A[q,i])^2 , norm_sq[q] = sum_i A[q,i]^2
 *   eval/run_retrieval_eval_wrt_exact_crossenc.py:146-147 (torch.norm over row subsets;
 *   the host sums the per-row terms over anchor / non-anchor / all rows in fp64).
 * X [Q x K] (x_dtype), Et [I x K] = E transposed (e_dtype), A [Q x I] (a_dtype).
 * err_sq / norm_sq: float[Q], overwritten.  A difference, a square or a sum inside the subnormal range is kept, here and in the two
 * packed forms below: rows whose every (S_hat - A)^2 is a subnormal still add up to their exact sum. */
int anncur_approx_error(const void *X, int x_dtype, int64_t ldx,
                        const void *Et, int e_dtype, int64_t lde,
                        const void *A, int a_dtype, int64_t lda,
                        int64_t Q, int64_t I, int64_t K,
                        float *err_sq, float *norm_sq, void *stream);

/* The same on the fused path's packed bf16 operands (layouts of anncur_score_topk: X [Q x Kp], Et [ceil32(I) x Kp], Kp in
 * {64,128,256,512}), on the bf16 MFMA loop of the sweep instead of the strided fp32 GEMM: ~25x faster at Q=10k, I=100k, Kp=256.
 * A: fp32 or bf16, 16-byte aligned, lda a multiple of 4 (ANNCUR_E_UNSUPPORTED otherwise: use anncur_approx_error). */
int anncur_approx_error_packed(const void *X, int64_t ldx, const void *Et, int64_t lde,
                               const void *A, int a_dtype, int64_t lda,
                               int64_t Q, int64_t I, int32_t Kp,
                               float *err_sq, float *norm_sq, void *stream);

/* a8 (retrieval half) + a11 of one grid cell of entry point A in ONE sweep (SURVEY 8b.6 `anncur_eval_fused`) ---------------------------
 *   approx = CURApprox(...).get(rows, cols); approx.topk(top_k_retvr); torch.norm((approx - A)[rows]) ; torch.norm(A[rows])
 *                                                                     eval/run_retrieval_eval_wrt_exact_crossenc.py:84,106,146-147
 * = anncur_score_topk(X, Et, k) + anncur_approx_error_packed(X, Et, A): out_val / out_idx = the exact top-k of S_hat = X . E (values
 * and index sets those of anncur_score_topk_ex with ANNCUR_TOPK_MFMA32: same MFMAs in the same order), err_sq[q] = sum_i (S_hat - A)^2,
 * norm_sq[q] = sum_i A^2 -- with ONE S_hat GEMM per sweep stage instead of two: the kernel that streams the exact tile through LDS
 * beside the MFMA chain also runs the threshold filter on the accumulator it holds (csrc/score_evalf.hpp).
 * X [Q x Kp], Et [ceil32(I) x Kp] packed bf16 in ITEM order (a tile of Et faces the same 32 columns of A), Kp in {64,128,256};
 * A [Q x I] bf16, 16-byte aligned, lda a multiple of 8 (ANNCUR_E_UNSUPPORTED otherwise: the two calls above).  Workspace:
 * anncur_eval_fused_workspace_bytes (0: shape outside the fused path).
 * Non-finite values: the top-k follows anncur_score_topk (NaN never selected, +-inf ordinary candidates, (-inf, -1) pads); err_sq[q] is
 * NaN if row q of S_hat - A holds a NaN (a NaN in either, or equal infinities in both), else +inf if it holds an infinity; norm_sq[q]
 * likewise from row q of A alone.  Rows without such a cell are not affected by the others' (anncur_approx_error(_packed): the same). */
size_t anncur_eval_fused_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k);
int anncur_eval_fused(const void *X, int64_t ldx, const void *Et, int64_t lde, const void *A, int a_dtype, int64_t lda,
                      int64_t Q, int64_t I, int32_t Kp, int32_t k, float *out_val, int32_t *out_idx, float *err_sq, float *norm_sq,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same with a HINT for the first threshold (round 5): Et_hint = a copy of Et's rows in any other order, same shape and pitch -- CURApprox
 * keeps one in descending-norm order for anncur_score_topk_ex (ANNCUR_TOPK_LEADING_SAMPLE) -- whose LEADING tiles the prepass samples instead of a
 * strided sample of Et: with the largest-norm items in the sample the first threshold is tighter and the sweep keeps fewer candidates.  The
 * sweep itself runs on Et (item order).  Same results bit for bit (any subset of the items yields a valid threshold); null = anncur_eval_fused. */
int anncur_eval_fused_ex(const void *X, int64_t ldx, const void *Et, int64_t lde, const void *Et_hint, const void *A, int a_dtype, int64_t lda,
                         int64_t Q, int64_t I, int32_t Kp, int32_t k, float *out_val, int32_t *out_idx, float *err_sq, float *norm_sq,
                         void *workspace, size_t workspace_bytes, void *stream);

/* a7/a8: exact row-wise top-k of a stored matrix (HBM-streaming scan) ---------------
 *   torch.topk(S, k, dim=1)                  eval/matrix_approx_zeshel.py:106,126
 *   curr_ment_scores.topk(top_k)             ...crossenc.py:103 ; ..._splits.py:86
 * A [Q x I] (dtype), out_val float[Q x k] (ldo = k), out_idx int32[Q x k].  1 <= k <= min(I, ANNCUR_MAX_TOPK).
 * Order: score descending, equal scores by ascending index (torch leaves ties unspecified).  -inf entries are ordinary
 * candidates; NaN is never selected (torch ranks NaN first): a row with fewer than k non-NaN entries is padded with (-inf, -1). */
int anncur_rowwise_topk(const void *A, int dtype, int64_t Q, int64_t I, int64_t lda, int32_t k,
                        float *out_val, int32_t *out_idx, void *stream);

/* The same scan over RAGGED rows (round 5; the batched IVF search's packed score rows): row q of A holds row_len[q] elements,
 * k <= row_len[q] <= I_max <= lda (a length outside 0..I_max is clamped; a row shorter than k is padded with (-inf, -1)).  k <= 128 (ANNCUR_E_UNSUPPORTED above). */
int anncur_rowwise_topk_ragged(const void *A, int dtype, int64_t Q, int64_t I_max, int64_t lda, const int32_t *row_len, int32_t k,
                               float *out_val, int32_t *out_idx, void *stream);

/* a2 folded into a8's pass over A (SURVEY a2 "fold into the first pass"; reference ..._splits.py:297,300 + 86): the scan of
 * anncur_rowwise_topk (k <= 128) also copies the anchor columns, cq[q, j] = A[q, col_idx[j]], as their 16-byte vectors stream past --
 * C_q costs no second read of the rows' sectors.  col_idx: n_idx (<= 65535) ascending, distinct columns in [0, I);
 * vec_tab uint32[ceil(I / V)] (V = 8 elements for bf16, 4 for fp32; per 16-byte vector: which elements are anchors, and how many
 * anchors lie before it) from anncur_gather_tables for the same (col_idx, I, dtype) -- built once per anchor set; cq [Q x ldo] has A's
 * element type.  A and its rows must be 16-byte aligned
 * (ANNCUR_E_UNSUPPORTED otherwise: use anncur_gather_cols + anncur_rowwise_topk).  Same top-k result as anncur_rowwise_topk.
 * Measured on MI355X (cfg2: 10 000 x 100 000 bf16, 256 anchors): 0.50 ms against 0.357 + 0.049 ms for the two separate kernels -- one HBM
 * pass less, but the per-vector extraction costs more than the sectors it saves; callers that are HBM-capacity- rather than
 * time-bound may still prefer it. */
int anncur_gather_tables(const int32_t *col_idx, int32_t n_idx, int64_t I, int dtype, uint32_t *vec_tab, void *stream);
int anncur_rowwise_topk_gather(const void *A, int dtype, int64_t Q, int64_t I, int64_t lda, int32_t k, float *out_val, int32_t *out_idx,
                               const int32_t *col_idx, int32_t n_idx, const uint32_t *vec_tab, void *cq, int64_t ldo, void *stream);

/* a6+a7 fused: S_hat = X . E never written; per-query top-k ---------------------------
 *   CURApprox.topk_in_row                    eval/matrix_approx_zeshel.py:121-126
 *   approx_curr_ment_scores.topk(top_k_retvr) ...crossenc.py:106 ; ..._splits.py:89
 *   faiss IndexFlatIP.add / .search          models/nearest_nbr.py:36-38 (+ utils/data_process.py:351,397)
 * X  [Q x Kp]  bf16 row-major (queries' anchor-item scores / query embeddings),
 * Et [Ip x Kp] bf16 row-major (item embeddings E^T), Kp in {64,128,256,512} with the
 * logical K zero-padded up to Kp, Ip = I rounded up to a multiple of 32 with zero rows.
 * Products are exact (bf16 x bf16 in fp32), sums fp32 on v_mfma_f32_32x32x16_bf16.
 * Launches on `stream`: (1) group-max pre-pass over a strided sample of item tiles ->
 * (2) per-query lower bound tau on the k-th best; (3) full sweep in 1-3 stages, survivors
 * >= tau appended to per-lane candidate segments, tau raised between stages; (4) per-query
 * select + sort (a query whose segments overflowed is repaired in the same call by
 * recomputing the affected item range: the result is always the exact top-k of S_hat).
 * Non-finite scores, on every body and under every flag: S_hat[q,i] is a NaN if a product has a NaN factor or is inf . 0, or if the sum
 * meets +inf and -inf (in any summation order), and a NaN is never selected; +inf and -inf scores are ordinary candidates (+inf first,
 * -inf last, ties by ascending row).  A query with fewer than k non-NaN scores gets all of them, then (-inf, -1) pads; a NaN in a row of
 * X makes that query's result k pads; a NaN row of Et is never returned and costs no other item or query its place (the prepass' group
 * maxima skip NaN; a query whose sample holds fewer than k non-NaN maxima, or whose k-th maximum is -inf, sweeps without a threshold and
 * its row is rescanned by the select).
 * Subnormal values, on every body and under every flag: a subnormal bf16 operand is read as it is and a subnormal product, partial sum or
 * score is kept (the bf16 MFMAs flush neither A/B nor C/D on gfx950), and the group maxima, tau, the ladder levels and every filter
 * compare it as the number it is: n 2^-149 never ties with 0.  The coarse threshold (a 16-bit key prefix) of a row of such scores is
 * +-0, about half of the row passes it and the select may repair: slower, and exact.  The same holds for anncur_eval_fused.
 * ldx: the pitch of X in elements, >= Kp and a multiple of 8.  On the wide route (Kp > 512) the kernel addresses the queries of a 256-row
 * block with 32-bit byte offsets: 255 x ldx x 2 + 64 < 2^32, i.e. ldx <= 8 421 504; a longer pitch is refused (ANNCUR_E_UNSUPPORTED, also by
 * anncur_score_topk_ex / _timed and anncur_eval_topk; anncur_score_topk_supported does not see the pitch): pass a compact copy of X.
 * out_val float[Q x k], out_idx int32[Q x k]. */
size_t anncur_score_topk_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k);
int anncur_score_topk_supported(int64_t Q, int64_t I, int32_t Kp, int32_t k);   /* 1 / 0 */
int anncur_score_topk(const void *X, int64_t ldx, const void *Et, int64_t lde,
                      int64_t Q, int64_t I, int32_t Kp, int32_t k,
                      float *out_val, int32_t *out_idx,
                      void *workspace, size_t workspace_bytes, void *stream);

/* The same with two hints an index builder can give (both leave the result the exact top-k of S_hat):
 *  ANNCUR_TOPK_LEADING_SAMPLE: the rows of Et are ordered so that the likeliest high scorers come first (e.g. by descending
 *    norm); the threshold sample then takes the leading item tiles instead of a strided sample (fewer survivors in the sweep);
 *  item_ids (int32[I], may be NULL): out_idx reports item_ids[row of Et] instead of the row (undoes such a reordering; score
 *    ties are then ordered by row, not by id).  Same workspace as anncur_score_topk. */
#define ANNCUR_TOPK_LEADING_SAMPLE 1
/*  The sweep has two bodies for Kp <= 256: v_mfma_f32_32x32x16_bf16 with per-lane candidate rings, and v_mfma_f32_16x16x32_bf16 with one
 *    candidate queue per wave (I < 2^26; the chip holds a higher clock on that shape).  Same products and fp32 sums: the result is the
 *    same bit for bit up to the order of exact score ties.  Default: the 16x16x32 body for k <= 1024, where its threshold ladder runs
 *    (k <= 384 in a plan without the ladder), the 32x32x16 body above.
 *  ANNCUR_TOPK_MFMA16 / ANNCUR_TOPK_MFMA32: force the 16x16x32 / the 32x32x16 body (A/B variants).  Kp = 512 has one MFMA shape and two
 *    candidate paths: one queue per wave with the dynamic tile schedule on 16x16x32 MFMAs (default, I < 2^26), per-lane rings with
 *    static shares on 32x32x16 MFMAs (ANNCUR_TOPK_MFMA32). */
#define ANNCUR_TOPK_MFMA16 2
/*  ANNCUR_TOPK_QT1 (Kp = 128 / 256): one 32-query sub-tile per wave and three workgroups per CU, with the cross-tile software
 *    pipeline of the Kp = 512 sweep, instead of two sub-tiles staggered inside a wave at two workgroups per CU (A/B variant). */
#define ANNCUR_TOPK_QT1 4
#define ANNCUR_TOPK_MFMA32 8
/*  ANNCUR_TOPK_RING: retired.  It selected a tile-ring sweep body (round 4: the 16x16x32 body in 8-wave workgroups of 512 queries whose
 *    item tiles stream through a ring of four LDS slots synchronised by per-wave counters instead of a workgroup barrier per tile),
 *    which measured 3-4 % slower than the default at every size tried.  The body is gone; a call that sets the flag fails with
 *    ANNCUR_E_UNSUPPORTED. */
#define ANNCUR_TOPK_RING 16
/*  ANNCUR_TOPK_STAGED: no threshold ladder -- the sweep in stages with a refinement launch between them, as rounds 1-4 ran it (A/B and
 *    parity reference; the default since round 5 is ONE sweep launch whose waves move their thresholds up a ladder of levels from
 *    device-wide counts of the candidates kept so far: csrc/score16.hpp).  Kp <= 256: for k <= 384 this is the default 16x16x32 body
 *    without its ladder; for k in 385..1024 the flag ALSO switches the body, to 32x32x16 with per-lane rings (the 16x16x32 body is the
 *    default there only because of the ladder), so an A/B in that range compares two kernels, not the ladder alone.  Same result. */
#define ANNCUR_TOPK_STAGED 32
int anncur_score_topk_ex(const void *X, int64_t ldx, const void *Et, int64_t lde,
                         int64_t Q, int64_t I, int32_t Kp, int32_t k,
                         float *out_val, int32_t *out_idx,
                         void *workspace, size_t workspace_bytes,
                         int32_t flags, const int32_t *item_ids, void *stream);

/* a6+a7 for a FEW queries (1 <= Q <= 64): the small-batch route (csrc/few.hip) ---------------------------------------
 * Same operands and the same result as anncur_score_topk -- the exact top-k of S_hat = X . E, score descending, ties by ascending row,
 * NaN never selected, +-inf ordinary candidates, (-inf, -1) pads -- in TWO launches: few_score_kernel streams Et once (item fragments
 * straight from global memory into v_mfma_f32_16x16x32_bf16, k ascending into one accumulator: at Kp <= 256 a score has the bits of
 * anncur_score_topk's) and writes S_hat [Q x ceil32(I)] fp32 plus one maximum per 64 consecutive items into the workspace;
 * few_select_kernel takes the k-th largest group maximum as threshold, reads only the groups that reach it, and selects.  A query with
 * more than cand_cap candidates at or above its threshold (heavy ties) is scanned in full by the same workgroup: always exact.
 * Et is in ITEM order (no leading-sample hint, no id map).  Rows >= Q of X are never read.  Subnormal operands, scores and group
 * maxima are kept as in anncur_score_topk, so the two routes agree on them bit for bit as well. */
#define ANNCUR_FEW_MAX_Q 64             /* queries per call */
#define ANNCUR_FEW_STAGE_BYTES 65536    /* LDS stage of the queries: 16 ceil(Q / 16) x Kp x 2 bytes must fit (Q <= 16: Kp <= 2048; Q > 48: Kp <= 512) */
#define ANNCUR_FEW_PLAN_WORDS 12
/*   CURApprox.topk_in_row, few queries          eval/matrix_approx_zeshel.py:121-126 ; models/nearest_nbr.py:36-38
 * 1 when 1 <= Q <= ANNCUR_FEW_MAX_Q, Kp in {64,128,256,512} or a multiple of 128 up to 4096, the queries fit the LDS stage,
 * 1 <= k <= min(I, ANNCUR_MAX_TOPK) and I < 2^31 - 1; 0 otherwise. */
int anncur_score_topk_few_supported(int64_t Q, int64_t I, int32_t Kp, int32_t k);
/*   eval/matrix_approx_zeshel.py:121-126 ; models/nearest_nbr.py:36-38
 * Header (1 KiB: per query {groups_read, n_cand, fallback, 0} as uint32), the group maxima and the score scratch; 0 = unsupported. */
size_t anncur_score_topk_few_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k);
/*   eval/matrix_approx_zeshel.py:121-126 ; models/nearest_nbr.py:36-38
 * X [Q x Kp] bf16 (pitch ldx >= Kp, a multiple of 8), Et [ceil32(I) x Kp] bf16 packed (lde == Kp), both 16-byte aligned; out_val float[Q x k],
 * out_idx int32[Q x k]; workspace 256-byte aligned, nothing in it pre-filled by the caller (the kernels write the header themselves).
 * A shape outside anncur_score_topk_few_supported is ANNCUR_E_UNSUPPORTED (k outside its range: ANNCUR_E_INVALID), a missing, short or
 * misaligned workspace ANNCUR_E_WORKSPACE; nothing is written then. */
int anncur_score_topk_few(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, int32_t k,
                          float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes, void *stream);
/*   CURApprox.get_complete_row, few queries     eval/matrix_approx_zeshel.py:118-126 ; models/nearest_nbr.py:36-38
 * Launch 1 alone, on the bf16 operands: S[q, i] = <X[q], Et[i]> for q < Q, i < I (pitch lds >= I, a multiple of 4, S 16-byte aligned) and
 * GM[q, g] = max of S[q, 64 g .. 64 g + 63] over the items < I (pitch ldg >= ceil(I / 64)); a NaN is skipped, an all-NaN group gives NaN.
 * Nothing else of S or GM is written. */
int anncur_score_rows_few(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, float *S, int64_t lds,
                          float *GM, int64_t ldg, void *stream);
/*   eval/matrix_approx_zeshel.py:121-126 ; models/nearest_nbr.py:36-38
 * The plan of a call (host only, no device): out[0..min(n_out, ANNCUR_FEW_PLAN_WORDS)) = {16-item tiles, workgroups, waves per workgroup,
 * fewest / most tiles of a wave that has any, 16-query sub-tiles, groups per query, cand_cap, scratch pitch / 32, groups per wave,
 * byte offsets / 256 of the group maxima and of the score scratch in the workspace}.  ANNCUR_E_UNSUPPORTED outside the route. */
int anncur_score_topk_few_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out, int32_t n_out);

/* a6+a7 on SPARSE operands: inner-product search through a term-major (inverted) index (csrc/sparse.hip) ------------------
 *   tfidf evaluation method           eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py:360-385
 *   TF-IDF hard-negative mining       utils/data_process.py:373-397 ; utils/compute_tfidf_hard_negs.py
 * Queries: CSR [Q x V], q_ptr int64[Q + 1], q_term int32 (strictly ascending inside a row), q_val fp32.  Items: the TRANSPOSE of a CSR
 * matrix [I x V], term_ptr int64[V + 1], post_item int32[nnz] (ascending inside a term), post_val fp32[nnz].  All on the device.
 * Score: S[q, i] = the fp32 chain over the terms t that q and i share, in ascending t, from +0.0f, each step two separately rounded
 * operations acc = fadd_rn(acc, fmul_rn(w_qt, v_it)); an item that shares no term with q scores +0.0 (bit pattern 0).  No atomics and no
 * split sums: a score does not depend on the launch shape, on Q or on the position of q in the call, and equals a float32 loop on the host
 * -- on a host that does not flush: subnormal weights, products and sums are kept by both steps.
 * One launch: a four-wave workgroup per (query, run of item windows); a wave owns a span of consecutive windows of ANNCUR_SPARSE_WINDOW
 * items with private accumulators in LDS and one cursor per query term into that term's posting list (found once per span by a lower
 * bound, carried from window to window).  LDS per workgroup: 8 bytes per staged query term (8 KB) + 4 waves x (8 KB accumulators + 8 bytes
 * per term of cursors) = 72 KB at ANNCUR_SPARSE_MAX_QNNZ = 1024, so two workgroups share a CU's 160 KB; 2048 terms would take 136 KB and
 * leave one.  A query with more stored terms than that is the CALLER's error (q_ptr lives on the device: ops checks it on the host); the
 * kernel reads its first ANNCUR_SPARSE_MAX_QNNZ terms.  Equally defensive: a term id outside [0, V) contributes nothing and term_ptr is
 * not read for it, a posting list is read for at most I entries, an item outside the window is skipped.
 * Top-k: anncur_rowwise_topk on the score rows -- score descending, equal scores to the smaller item id, NaN never, -inf ordinary,
 * (-inf, -1) pads; this route has no selector of its own.  On a row where thousands of items tie at +0.0 the scan's threshold is a composite
 * (score, id) key: once a compaction has left it at the k-th zero, every later zero has a larger id, a smaller key, and is dropped
 * without being buffered (the one-wave form for k <= 128 does the same in its wave's buffer): exact, and one read of the row as on any
 * other data.  (few_select_kernel on (S, GM) would find nearly every group maximum equal to the
 * threshold, overflow its candidate buffer and fall back to the same full scan, so GM buys nothing there; it is written for callers that
 * audit the scores.) */
#define ANNCUR_SPARSE_WINDOW 2048       /* items per window of LDS accumulators */
#define ANNCUR_SPARSE_MAX_QNNZ 1024     /* stored terms per query (a 128-token mention has at most 128, an entity description a few hundred) */
#define ANNCUR_SPARSE_PLAN_WORDS 10
/*   ..._splits.py:383 (mention x entity TF-IDF scores)
 * S[q, i] for q < Q, i < I at pitch lds >= I (16-byte stores when S is 16-byte aligned and lds a multiple of 4, scalar stores otherwise)
 * and, if GM is not NULL, GM[q, g] = max of S[q, 64 g .. 64 g + 63] over the items < I at pitch ldg >= ceil(I / 64), an fmaxf chain from
 * NaN as anncur_score_rows_few's.  Nothing else of S or GM is written.  Q >= 0 (Q == 0 returns OK), 1 <= I < 2^31 - 1, 0 <= V < 2^31;
 * Q x workgroups per query must stay below 2^31 (ANNCUR_E_UNSUPPORTED: call in chunks).  post_item / post_val may be NULL when nnz == 0. */
int anncur_sparse_score_rows(const int64_t *q_ptr, const int32_t *q_term, const float *q_val, int64_t Q, const int64_t *term_ptr,
                             const int32_t *post_item, const float *post_val, int64_t V, int64_t I, float *S, int64_t lds, float *GM,
                             int64_t ldg, void *stream);
/*   ..._splits.py:383-385 ; utils/data_process.py:397 (index.search(ment_embeds, k))
 * The scores into the workspace [Q x ceil32(I)] fp32 (256-byte aligned, nothing pre-filled), then anncur_rowwise_topk: out_val float[Q x k],
 * out_idx int32[Q x k], 1 <= k <= min(I, ANNCUR_MAX_TOPK).  A short or misaligned workspace is ANNCUR_E_WORKSPACE, nothing is written. */
int anncur_sparse_score_topk(const int64_t *q_ptr, const int32_t *q_term, const float *q_val, int64_t Q, const int64_t *term_ptr,
                             const int32_t *post_item, const float *post_val, int64_t V, int64_t I, int32_t k, float *out_val,
                             int32_t *out_idx, void *workspace, size_t workspace_bytes, void *stream);
/* Q x ceil32(I) x 4 bytes; 0 outside the limits. */
size_t anncur_sparse_score_topk_workspace_bytes(int64_t Q, int64_t I, int32_t k);
/* The plan of a call (host only, no device): out[0..min(n_out, ANNCUR_SPARSE_PLAN_WORDS)) = {windows per query, windows per wave, spans
 * (waves with work) per query, workgroups per query, workgroups, waves per workgroup, LDS bytes per workgroup, score pitch / 32, groups of
 * 64 items per query, ANNCUR_SPARSE_MAX_QNNZ}.  Windows per wave = ceil(Q x windows / 2048 waves), at most a query's windows: one query
 * spreads over its windows, many queries give each wave a long span and few searches. */
int anncur_sparse_plan(int64_t Q, int64_t I, int32_t *out, int32_t n_out);

/* a6+a7 at fp32 parity on the bf16 matrix cores: the split-bf16 ("bf16x3") route -------------------------------------------------
 *   CURApprox.get_complete_row + topk_in_row on FloatTensors      eval/matrix_approx_zeshel.py:118,126
 *   faiss IndexFlatIP.add / .search on float32 vectors            models/nearest_nbr.py:36-38
 * The fp32 route materialises S_hat with anncur_gemm and scans it; this one keeps S_hat unwritten.  An fp32 operand is split as
 * x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (round-to-nearest-even; x - hi is exact), and  x.e ~= lo_x hi_e + hi_x lo_e + hi_x hi_e
 * is ONE bf16 inner product of length 3K, so anncur_score_topk_ex sweeps the packed operands unchanged with Kp >= 3K; the dropped
 * lo.lo term and the roundings of lo leave |S_split - S| <= (2^-16 + 3K 2^-23) (|X|.|E|^T) elementwise.  The few candidates it
 * returns are then rescored in true fp32 (anncur_rescore_topk): the values the caller sees are those of anncur_gemm bit for bit.
 * NaN operands behave as on the fp32 route (the NaN scores are never candidates).  LIMIT: an operand entry that is +-inf (or rounds to
 * it in bf16) has hi = +-inf and lo = 0, and its term inside the sweep is lo_x hi_e + hi_x lo_e + hi_x hi_e with inf . 0 = NaN or two
 * infinities of opposite sign -- a NaN unless the other side's entry has a non-zero low part of its high part's sign.  So a score that
 * anncur_gemm reports as +-inf is a candidate only against those entries and a NaN, never retrieved, against all others (every entry that
 * is exact in bf16 among them): an item or a query with an infinite entry loses the results the fp32 route returns at +-inf, all of them
 * or an operand-dependent part.  Keep infinities off this route.
 *
 * anncur_pack_split_bf16: src [n_rows x K] (F32 or BF16, row pitch lds_) -> dst bf16 [n_rows_pad x ldd], ldd >= 3K a multiple of 8,
 *   dst 16-byte aligned.  role 0 (query rows) writes [ lo | hi | hi ], role 1 (item rows) [ hi | lo | hi ], each segment K wide at
 *   element offsets 0, K, 2K.  The kernel writes EVERY element of dst -- zeros in columns 3K..ldd and in rows n_rows..n_rows_pad --,
 *   the caller clears nothing.  Where hi is not finite (inf, NaN, a finite x that rounds to inf) lo = 0; BF16 input gives lo = 0. */
int anncur_pack_split_bf16(const void *src, int src_dtype, int64_t lds_, int64_t n_rows, int64_t K, int role,
                           void *dst, int64_t ldd, int64_t n_rows_pad, void *stream);
/* anncur_rescore_topk: for query q and each of its n_cand candidate ids i = cand_idx[q*ld_idx + j] (distinct per row; an id < 0 or
 *   >= I is a hole and is skipped), s = fmaf(X[q,K-1], Et[i,K-1], ... fmaf(X[q,0], Et[i,0], 0)) in fp32, k ascending -- the k-ordered
 *   fmaf chain anncur_gemm is bit for bit, subnormal operands and partial sums included -- and the k_out best: out_val float[Q x k_out], out_idx int32[Q x k_out] (item ids), score
 *   descending, ties by the smaller id, NaN never selected, (-inf, -1) where fewer than k_out valid candidates exist.
 *   X [Q x K] (x_dtype, pitch ldx), Et [I x K] (e_dtype, pitch lde; rows are read with 16-byte loads when Et and its pitch are 16-byte
 *   aligned).  k_out <= n_cand <= ANNCUR_MAX_TOPK.  An HBM gather of Q n_cand K elements; no matrix cores.
 *   Workspace: scratch = float[Q x n_cand] (4 Q n_cand bytes, caller-owned, contents undefined on entry and exit). */
int anncur_rescore_topk(const void *X, int x_dtype, int64_t ldx, const void *Et, int e_dtype, int64_t lde, int64_t K,
                        const int32_t *cand_idx, int64_t ld_idx, int32_t n_cand, int64_t Q, int64_t I, int32_t k_out,
                        float *out_val, int32_t *out_idx, float *scratch, void *stream);

/* filtered retrieval: the best k items OUTSIDE a given set, behind every top-k above ---------------------------------------------
 *   the anchor items every query has scored already               ..._w_fixed_train_test_splits.py:297-301
 *   the gold entity removed by hand after the search              utils/data_process.py:343-351,393-397
 * (FAISS, whose calling convention models/nearest_nbr.py follows, has an id selector for this.)  If query q excludes e_q distinct
 * items, the unfiltered top-(k + e_q) contains the filtered top-k: the caller asks its top-k for k + max_q e_q candidates and this call
 * compacts each row.  No other entry point, plan or workspace knows about it.
 *
 * anncur_filter_topk: row q of in_val / in_idx (both with row pitch ld_in) holds n_cand (score, id) entries in the producer's order
 *   -- descending --; an id < 0 is a hole.  excl_off != NULL: query q excludes excl_ids[excl_off[q] .. excl_off[q+1]) (excl_off
 *   int64[Q + 1], ascending); excl_off == NULL: every query excludes excl_ids[0 .. n_excl_shared) (n_excl_shared is ignored otherwise).
 *   The ids of a segment are STRICTLY ASCENDING (the kernel binary-searches them and trusts this; the Python layer sorts and
 *   de-duplicates); empty segments are fine, and excl_ids may be NULL when there is nothing to exclude.
 *   out_val float[Q x k_out], out_idx int32[Q x k_out], contiguous: the first k_out entries of row q that are neither holes nor
 *   excluded, IN INPUT ORDER (a stable compaction), then (-inf, -1).  The outputs must not alias the inputs.
 *   1 <= k_out <= n_cand <= ANNCUR_MAX_TOPK, Q >= 1.  One wave per query; latency-bound, the rows and segments come from L2. */
int anncur_filter_topk(const float *in_val, const int32_t *in_idx, int64_t ld_in, int64_t n_cand, int64_t Q,
                       const int64_t *excl_off, const int32_t *excl_ids, int64_t n_excl_shared, int32_t k_out,
                       float *out_val, int32_t *out_idx, void *stream);

/* a8 per-query evaluation loop: exact top-k of the stored scores AND the approximate retrieval, in one call ----------------------
 *   curr_ment_scores.topk(top_k) ; approx_curr_ment_scores.topk(top_k_retvr)          ...crossenc.py:97-106 ; ..._splits.py:80-89
 * = anncur_rowwise_topk(A, k_exact) + anncur_score_topk_ex(X, Et, k_retvr), same results, scheduled together: the retrieval is a chain
 * of MFMA-bound sweep launches with latency-bound launches between them (threshold, refinements, select); the HBM-bound exact scan is
 * cut into row chunks (whole rounds of the scan's rows in flight) and chunk i runs on `aux_stream` beside the i-th latency-bound
 * launch -- forked and joined with events, so the call is one unit of work on `stream` (and capturable into a graph).  aux_stream
 * NULL or equal to stream: the two parts run one after the other.  Workspace as anncur_score_topk.
 * On an error return the outputs are undefined (chunks of the scan already forked are joined back into `stream` first). */
int anncur_eval_topk(const void *A, int a_dtype, int64_t lda, int32_t k_exact, float *exact_val, int32_t *exact_idx,
                     const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, int32_t k_retvr,
                     float *approx_val, int32_t *approx_idx, void *workspace, size_t workspace_bytes,
                     int32_t flags, const int32_t *item_ids, void *stream, void *aux_stream);

/* Measurement only: same as anncur_score_topk but records HIP events on `stream` between the four
 * launches, synchronises, and returns their durations in stage_ms[9] (host floats, milliseconds):
 * {prepass (its workgroups also clear the workspace header: there is no memset launch in front of it), threshold,
 *  sweep stage (sweep launches + the threshold refinements between them), select,
 *  sum of the sweep-kernel launches alone, number of sweep launches, and the duration of each of the up to
 *  three sweep launches (0 where the plan has fewer stages; anncur_score_topk_plan_ex gives their tile ranges)}.
 *  bench.py's live roofline figure is (2*Q*Kp*I / launches) / (stage_ms[4] / launches). */
int anncur_score_topk_timed(const void *X, int64_t ldx, const void *Et, int64_t lde,
                            int64_t Q, int64_t I, int32_t Kp, int32_t k,
                            float *out_val, int32_t *out_idx,
                            void *workspace, size_t workspace_bytes,
                            int32_t flags, const int32_t *item_ids, void *stream, float *stage_ms);
/* Plan introspection: out5 = {sample tiles, item tiles, item splits S, segment capacity, group size}. */
int anncur_score_topk_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out5);
/* The plan a call with `flags` (ANNCUR_TOPK_*) would run: out[0 .. n_out), n_out <= 24 = {sample tiles, item tiles, item splits S,
 * segment capacity, group size, candidate segments per (query, item split) -- 2: 32x32x16 sweep, 1: 16x16x32 sweep, 4: wide
 * kernel --, 32-query sub-tiles per wave, number of sweep stages, stage_end[3] (tiles), body per stage[3] (0: 32x32x16 with the ballot
 * filter, 1: 32x32x16 with the exec-mask filter, 2: 16x16x32, 4: the Kp = 512 body with the wave-level queue on 16x16x32 MFMAs), ring
 * drain period per stage[3], threshold ladder (1: in-launch ladder, 0: none), rank of the ladder's top level among the sampled group
 * maxima, tiles between two fetches of a wave's ladder counters, workspace offset of the prepass' group maxima (256-byte units), group
 * maxima per query, prepass kernel (1: prepass16_kernel on the sweep's 16x16x32 body, 0: score_prepass_kernel<Kp, ..>), prepass item splits}.  Lets a caller (and the parity tests) see that a variant flag was
 * honoured for the shape. */
int anncur_score_topk_plan_ex(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, int32_t *out, int32_t n_out);
/* The plan anncur_eval_fused(_ex) runs for a cell (read-only, host code, no device needed): out[0 .. n_out), n_out <= 27 = the 24 words of
 * anncur_score_topk_plan_ex (body per stage: 6 = evalf_kernel; no ladder) followed by the tiles per item split of each sweep stage [3].
 * Item split s of stage g sweeps the 32-item tiles [begin_g + s tps_g, min(begin_g + (s + 1) tps_g, stage_end[g])) with begin_0 = 0 and
 * begin_g = stage_end[g - 1]: what a test needs to put an element on the first and last column of every split and stage.
 * ANNCUR_E_UNSUPPORTED where anncur_eval_fused_workspace_bytes gives 0. */
int anncur_eval_fused_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out, int32_t n_out);
/* Diagnostics: mean number of candidates per query the sweep of the last call on `workspace` kept (reads the segment counts it left
 * behind; synchronises `stream`).  k ln(I / k) is what a sequential threshold can reach. */
int anncur_score_topk_survivors(const void *workspace, int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, double *mean_per_query,
                                void *stream);
/* Diagnostics: the threshold ladder the sweep of the last call on `workspace` (same Q, I, Kp, k, flags) left behind; synchronises `stream`.
 * Host arrays: levels[Q x 8] (the levels above tau0, ascending), counts[Q x 8] (candidates counted with level j as the highest they
 * reach, one count per level: counts[q][j - 1]), tau_final[Q] (the select's prefilter: the highest threshold a workgroup ended with),
 * tau0[Q] (the prepass threshold; may be NULL).  ANNCUR_E_UNSUPPORTED when the plan has no ladder. */
int anncur_score_topk_ladder_state(const void *workspace, int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, float *levels,
                                   uint32_t *counts, float *tau_final, float *tau0, void *stream);

/* a8: exact re-rank of the approximately retrieved items + a10 overlap counts --------
 *   temp[approx_idx] = exact[approx_idx]; temp.topk(k)      ...crossenc.py:108-113 ; ..._splits.py:93-96
 *   compute_overlap(exact[:, :top_k], rerank[:, :top_k])    eval/eval_utils.py:115-150
 * A [Q x I] exact scores; approx_idx int32, row q at approx_idx + q*ld_idx, first k_retvr entries used
 * (distinct per row; ld_idx lets a prefix of a longer sorted list be re-ranked in place);
 * rerank_val float[Q x k_out], rerank_idx int32[Q x k_out]: the k_out best retrieved items
 * by exact score (k_out <= k_retvr <= ANNCUR_MAX_TOPK). */
int anncur_rerank(const void *A, int dtype, int64_t Q, int64_t I, int64_t lda,
                  const int32_t *approx_idx, int64_t ld_idx, int32_t k_retvr, int32_t k_out,
                  float *rerank_val, int32_t *rerank_idx, void *stream);
/* common[p*Q + q] = | a[q, :ka[p]] (set) intersect b[q, :kb[p]] | for each of n_pairs
 * (ka,kb) prefix-length pairs (host int32 arrays), a int32[Q x la], b int32[Q x lb].
 * Set semantics on both sides: an id that a prefix repeats is one member, and ids below zero (the -1 pads
 * of a top-k row with fewer than k items) are members of no set.  1 <= la, lb <= 4096, 0 <= ka[p] <= la,
 * 0 <= kb[p] <= lb, 1 <= n_pairs <= 64; every one of the n_pairs x Q counts is written (common may be
 * mapped host memory).  Q == 0 is valid and launches nothing; all other arguments are still checked. */
int anncur_overlap_counts(const int32_t *a, int32_t la, const int32_t *b, int32_t lb, int64_t Q,
                          const int32_t *ka, const int32_t *kb, int32_t n_pairs,
                          int32_t *common, void *stream);

/* ranks of given items -----------------------------------------------------------------------------------------------
 * The inverse of a top-k: where does item `id` stand in a score row?  For a row s[0..I) and a target id, a = s[id]:
 *
 *     rank = #{ i != id : s[i] > a  or  (s[i] == a and i < id) }
 *
 * i.e. the position of id in the row sorted by score descending, ties to the smaller id -- the order of anncur_rowwise_topk.  The compare
 * is the float compare: -0.0 and +0.0 tie, and only they: a subnormal of either sign, fp32 or bf16, is ahead of or behind the zeros
 * (anncur_score_rank keeps subnormal operands and scores as anncur_score_topk does); a NaN score is never ahead of anything; a target whose own score is NaN gets rank -1, and so
 * does a hole (id == -1).  Any other id outside [0, I) is the caller's error (the Python binding raises ValueError); the kernels treat it
 * as a hole and never read through it.  Duplicate ids in a row are allowed, each reports that item's rank.
 *   ids int32[Q x t], rank int32[Q x t], score float[Q x t] or NULL, all contiguous; 1 <= t <= ANNCUR_RANK_MAX_T.
 *   score[q, j] = the target's score as the route computed it (NaN for a hole).
 * Every score in one comparison comes from the same arithmetic, the target's own included: anncur_rank_in_rows reads a from the row it
 * counts over; anncur_score_rank computes a with the tile routine of its counting pass (same fragments, same k order), so a is
 * bit-identical to what that pass computes for (q, id) and an item with the target's embedding and a larger id lands right behind it.
 *
 * anncur_rank_in_rows: S [Q x I] (ANNCUR_F32 / ANNCUR_BF16), row pitch lds_ >= I elements, any alignment.  One workgroup per row: target keys
 *   sorted in LDS, the row streamed with 16-byte loads, elements that beat the weakest target binary-searched into t bins, prefix sum.
 *   0 <= Q < 2^31 (Q == 0 returns OK), 1 <= I < 2^31 - 1; anything else is ANNCUR_E_INVALID and nothing is written.  No workspace.
 * anncur_score_rank: ranks under S_hat = X . Et^T, which is never written.  X [Q x Kp] packed bf16 (pitch ldx, a multiple of 8), Et
 *   [ceil32(I) x Kp] packed bf16 in ITEM order (lde == Kp), both 16-byte aligned -- the operands of anncur_approx_error_packed; Kp in
 *   {64, 128, 256, 512} (ANNCUR_E_UNSUPPORTED otherwise).  Rows I .. ceil32(I) - 1 of Et are padding and are not counted; lanes past Q
 *   neither store nor count.  Workspace: caller-owned, anncur_score_rank_workspace_bytes(Q, I, Kp, t) bytes (0 = shape not taken), 256-byte
 *   aligned, nothing in it pre-filled by the caller; missing, misaligned or short is ANNCUR_E_WORKSPACE.  The counts of different item
 *   splits meet by integer atomics: results are deterministic. */
#define ANNCUR_RANK_MAX_T 1024
int anncur_rank_in_rows(const void *S, int dtype, int64_t Q, int64_t I, int64_t lds_, const int32_t *ids, int32_t t,
                        int32_t *rank, float *score, void *stream);
size_t anncur_score_rank_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t t);
int anncur_score_rank(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp,
                      const int32_t *ids, int32_t t, int32_t *rank, float *score,
                      void *workspace, size_t workspace_bytes, void *stream);

/* search without the exact matrix: re-rank from caller-supplied scores ---------------------------------------------
 *   temp[approx_idx] = exact[approx_idx]; temp.topk(k)      ..._splits.py:91-96 ; ...crossenc.py:108-113
 *   the anchor items' exact scores, which every query has paid for already        ..._w_fixed_train_test_splits.py:297-301
 * anncur_rerank reads exact scores from a resident [Q x I] matrix; a caller who searches holds them in two other forms, and the pool of
 * query q is the union of the two:
 *   shared source     sh_ids int32[n_sh], STRICTLY ASCENDING and non-negative (the kernel binary-searches them and trusts the order, as
 *                     anncur_filter_topk does), with scores sh_val[q*ld_sh + 0..n_sh) of sh_dtype (ANNCUR_F32 / ANNCUR_BF16) -- the anchor
 *                     scores X.  n_sh may be 0; both pointers may then be NULL;
 *   per-query source  pq_idx int32[Q x ld_pq], pq_val float[Q x ld_pq], the first n_pq entries of a row; an id < 0 is a hole and is
 *                     skipped; the ids of a row are distinct (a contract, as for anncur_rerank).  n_pq may be 0 (NULL pointers allowed).
 * A per-query entry whose id occurs in sh_ids is dropped and the shared source's score stands: a caller who did not exclude the anchors at
 * retrieval still gets every item once.  out_val float[Q x k_out], out_idx int32[Q x k_out], contiguous: the k_out best of the pool, score
 * descending, ties by the smaller id; NaN is never selected, -inf is an ordinary candidate, (-inf, -1) pads a row with fewer than k_out
 * valid entries.  0 <= n_sh <= 65535, 0 <= n_pq <= ANNCUR_MAX_TOPK, n_sh + n_pq >= 1, 1 <= k_out <= min(ANNCUR_MAX_TOPK, n_sh + n_pq),
 * Q >= 0 (Q == 0 returns OK); anything else is ANNCUR_E_INVALID and nothing is written.  One workgroup per query; no workspace. */
int anncur_rerank_scored(const int32_t *sh_ids, const void *sh_val, int sh_dtype, int64_t ld_sh, int64_t n_sh,
                         const int32_t *pq_idx, const float *pq_val, int64_t ld_pq, int32_t n_pq,
                         int64_t Q, int32_t k_out, float *out_val, int32_t *out_idx, void *stream);
/* out[q*ldo + j] = (float) A[q, idx[q*ld_idx + j]] for j < n: the exact scores of per-query candidates out of a stored matrix (the
 * evaluation mode's stand-in for the cross-encoder call of step 3; ..._splits.py:91-96 reads the same cells).  A [Q x I] (dtype, pitch
 * lda); an id outside [0, I) yields NaN, which no selector here takes.  Q n random sectors, as anncur_gather_cols. */
int anncur_gather_pairs(const void *A, int dtype, int64_t Q, int64_t I, int64_t lda, const int32_t *idx, int64_t ld_idx, int32_t n,
                        float *out, int64_t ldo, void *stream);

/* adaptive multi-round search: per-query least squares on the fp64 matrix cores --------------------------------------
 *   w_q = c_q . pinv(R[:, S_q])        replaces numpy.linalg.pinv of eval/matrix_approx_zeshel.py:47,49 called once PER QUERY AND ROUND
 *                                      (the index' own pseudo-inverse, anncur_amd/pinv.py, is one matrix: ~28 dependent products)
 * Rt float[m x kq], pitch ldr >= kq, item-major: row i = item i's scores under the kq anchor queries (the pitch pad is never read into a
 * sum; a subnormal fp32 entry is gathered as it is and widens to a normal fp64).  ids int32[Q x n] (pitch ld_ids), an id < 0 (or >= m) marks a hole; the ids of a row are distinct (a contract, as for
 * anncur_rerank).  C float[Q x n] (pitch ldc): C[q, j] = the exact score of query q on item ids[q, j], ignored at holes.  ridge = lambda >= 0.
 * Row q of W float[Q x kq] (pitch ldw) becomes
 *     w_q = argmin_w || w R_S - c ||^2 + lambda ||w||^2,      R_S = the columns Rt[ids[q, j], :]^T of the non-hole entries, kq x n_q,
 * at lambda = 0 the minimum-norm minimiser c . pinv(R_S) wherever R_S has full rank.  Normal equations on the smaller side, in fp64,
 * by Cholesky; the side is chosen per call:
 *   item side,  n <= kq:  G = R_S^T R_S + lambda I [n x n], G y = c^T, w = (R_S y)^T; a hole is a zero row and column with its diagonal
 *                         set to 1 and its right-hand side to 0 (y = 0 there);
 *   query side, n >  kq:  G = R_S R_S^T + lambda I [kq x kq], b = R_S c^T, G w^T = b; holes contribute nothing.
 * W is rounded to fp32 once, at the store.
 * PIVOT RULE (part of the contract): status[q] = 1 and row q of W = NaN if a Cholesky pivot is <= 2^-40 max_i G_ii, the diagonal taken
 * BEFORE lambda is added (the 1s of holes take no part); otherwise status[q] = 0.  The fp64 factorisation's backward error is of order
 * g 2^-53 ||G|| <= 2^-44 ||G|| at g = 512, so 2^-40 is 16 times the noise floor; it corresponds to cond_2(R_S) ~ 10^6, past which fp32
 * score data carries no information.  (A row whose entries are all holes: W = 0 on the item side, status 1 on the query side at lambda = 0.)
 * Limits: 1 <= n <= ANNCUR_MAX_TOPK, 1 <= kq <= ANNCUR_LSTSQ_MAX_KQ, g = min(n, kq) <= ANNCUR_LSTSQ_MAX_G, Q G-tiles < 2^31 per call
 * (split the queries); anything else is ANNCUR_E_INVALID and nothing is written.  Workspace: caller-owned, 256-byte aligned,
 * anncur_lstsq_rows_workspace_bytes(Q, n, kq) = Q (gp + 1) gp doubles, gp = ceil16(g) (0 for a shape outside the limits); nothing in it is
 * pre-filled by the caller.  anncur_lstsq_rows_timed: the same call, synchronised, with ms3 = HIP-event times of (Gram [+ right-hand
 * side on the query side], factor-and-solve, w = R_S y [item side; 0 on the query side]). */
#define ANNCUR_LSTSQ_MAX_KQ 4096
#define ANNCUR_LSTSQ_MAX_G  512
size_t anncur_lstsq_rows_workspace_bytes(int64_t Q, int32_t n, int32_t kq);
int anncur_lstsq_rows(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc,
                      int64_t Q, int32_t n, double ridge, float *W, int64_t ldw, int32_t *status, void *workspace, size_t workspace_bytes,
                      void *stream);
int anncur_lstsq_rows_timed(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc,
                            int64_t Q, int32_t n, double ridge, float *W, int64_t ldw, int32_t *status, void *workspace, size_t workspace_bytes,
                            void *stream, float *ms3);
/* The same solve, item side only, on a per-query STATE that persists from call to call: a caller whose id lists only grow at the end
 * (the rounds of the adaptive search) pays for the new rows alone.
 *   replaces anncur_lstsq_rows called once per round on the whole scored set: n^2 (kq + n / 3) there, about k n (kq + n) here for k new items
 * ids int32[Q x n_new] and C float[Q x n_new] are the FULL rows in insertion order; the positions < n_old must be what the previous call
 * on this state saw (the caller's contract, not checked).  Holes are allowed anywhere and decouple as above.  n_old = 0 initialises the
 * state: the caller pre-fills nothing, every cell that is ever read is written by this or an earlier call.  ridge must be the same in
 * every call on one state (the caller's contract).
 * RESULT: W and status after the call equal, bit for bit, what anncur_lstsq_rows returns for (ids[:, :n_new], C[:, :n_new], ridge).  Both
 * run the same kernels, which take the row pitch, the place of the right-hand side and the first row / panel to compute at run time:
 * anncur_lstsq_rows starts them at 0, this call at panel p0 = n_old / 16 (the partial 16-block's padding becomes real, so that panel is
 * formed again).  For panels < p0 only the row blocks from p0 down are computed (the same sum over the earlier panels, then the
 * triangular solve against the stored diagonal block), z is recomputed from 16 p0 on, the back substitution and w = R_S y run in full.
 * PIVOT RULE: the one above.  max_i G_ii grows as items arrive, so the smallest pivot accepted so far is tested against the new threshold
 * too: an old pivot that falls under it fails the query, as it does in anncur_lstsq_rows.  A failed query is STICKY: every later call on
 * that state returns status 1 and a NaN row for it at the cost of reading its header, and leaves its state as it is (pivots do not change
 * and the threshold never falls, so anncur_lstsq_rows fails it too).
 * State: caller-owned, 256-byte aligned, anncur_lstsq_state_bytes(Q, cap) bytes (0 outside 1 <= cap <= ANNCUR_LSTSQ_MAX_G, Q >= 0); per
 * query, in doubles at the row pitch capp = ceil16(cap): capp rows of G's lower triangle, which turns into L; a row of z = L^-1 c; a row
 * of y (z is never overwritten); a header of 16 (the largest Gram diagonal so far, the smallest accepted pivot so far, the status, the
 * number of leading entries of z that are valid).  Rows at or beyond ceil16(n_new) are neither read nor written.  The layout is this library's: anncur_lstsq_state_bytes is its only
 * authority.
 * Limits: 0 <= n_old < n_new <= min(cap, kq), 1 <= kq <= ANNCUR_LSTSQ_MAX_KQ; n_new > kq (the query side has no incremental form) and
 * anything else outside them is ANNCUR_E_INVALID and nothing is written; a missing, misaligned or short state is ANNCUR_E_WORKSPACE.
 * anncur_lstsq_extend_timed: the same call, synchronised, with ms3 = HIP-event times of (Gram, factor-and-solve, w = R_S y). */
size_t anncur_lstsq_state_bytes(int64_t Q, int32_t cap);
int anncur_lstsq_extend(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc,
                        int64_t Q, int32_t n_old, int32_t n_new, int32_t cap, double ridge, float *W, int64_t ldw, int32_t *status,
                        void *state, size_t state_bytes, void *stream);
int anncur_lstsq_extend_timed(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C,
                              int64_t ldc, int64_t Q, int32_t n_old, int32_t n_new, int32_t cap, double ridge, float *W, int64_t ldw,
                              int32_t *status, void *state, size_t state_bytes, void *stream, float *ms3);
/* Seed a state from a SHARED PREFIX: where the id rows of all Q queries begin with the same n_sh ids (the adaptive search's anchor items,
 * in the index' order), their n_sh x n_sh Gram block and its Cholesky factor are the same for every query.  This call forms and factors
 * them once -- the Gram and factor kernels of the calls above, for one query, without a right-hand side -- and copies the factor and the
 * header to every query's slot of the state.
 *   replaces the first anncur_lstsq_extend(n_old = 0) of a search forming and factoring that block Q times
 * shared_ids int32[n_sh] on the device, every id in [0, m) (a hole in it is allowed and decouples, but then every row must hold a hole
 * there).  The state must be fresh: this call takes the place of n_old = 0, the caller pre-fills nothing.
 * RESULT: take anncur_lstsq_extend(n_old = n_sh, n_new, ...) on the seeded state, n_sh < n_new <= min(cap, kq), where the first n_sh
 * columns of ids equal shared_ids in every row (the caller's contract, not checked, like "the positions < n_old are what the previous
 * call saw").  W and status equal anncur_lstsq_rows(ids[:, :n_new], C[:, :n_new], ridge) bit for bit, hence also
 * anncur_lstsq_extend(n_old = 0, n_new) on a fresh state; so does every later extension.  z = L^-1 c is the one per-query part of the
 * prefix: the header counts the leading entries of z that are valid (0 after this call, n_new after a successful extension), and an
 * extension that finds fewer than 16 p0 of them carries the right-hand side through the old panels too -- inside the same factor
 * kernel, by the same chain of operations as anncur_lstsq_rows.
 * FAILURE: a shared block that fails the pivot rule makes every query's header sticky-failed: every later extension returns status 1 and
 * a NaN row for all queries, as anncur_lstsq_rows does for each of them.  Every query gets the shared block's largest diagonal and
 * smallest pivot, so a shared pivot that falls under the threshold once an appended item has raised the maximum fails that query alone.
 * Limits: 1 <= n_sh <= min(cap, kq), 1 <= cap <= ANNCUR_LSTSQ_MAX_G, 1 <= kq <= ANNCUR_LSTSQ_MAX_KQ, ridge >= 0 (the one of every later
 * call), m >= 1, ldr >= kq; anything else is ANNCUR_E_INVALID; a missing, misaligned or short state (anncur_lstsq_state_bytes(Q, cap)
 * bytes, 256-byte aligned; layout and size as above) is ANNCUR_E_WORKSPACE; both before any pointer is read.  Q = 0 returns ANNCUR_OK.
 * Rows at or beyond ceil16(n_sh), and the rows of z and y, are neither read nor written. */
int anncur_lstsq_seed_shared(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *shared_ids, int32_t n_sh, int64_t Q,
                             int32_t cap, double ridge, void *state, size_t state_bytes, void *stream);
/* Rows of (id, score) pairs sorted ascending by id, holes (id < 0) last, scores carried along; equal keys keep their order.
 *   replaces the per-query numpy.unique of ops.exclusion (one host pass and one synchronisation per call) where a searcher re-sorts its
 *   scored set every round: the sorted full rows ARE the per-query exclusion lists of anncur_filter_topk (off[q] = q w).
 * in_ids int32 / in_val float [Q x w] (pitch ld_in), out_ids / out_val [Q x w] (pitch ld_out; may be the inputs), counts int32[Q] = the
 * non-holes of each row.  1 <= w <= ANNCUR_MAX_TOPK.  One workgroup per row, a bitonic sort in LDS. */
int anncur_sort_id_rows(const int32_t *in_ids, const float *in_val, int64_t ld_in, int64_t Q, int32_t w, int32_t *out_ids, float *out_val,
                        int64_t ld_out, int32_t *counts, void *stream);

/* SoftMax item sampling: k items per row drawn WITHOUT replacement with probability proportional to softmax(S / T) ------
 *   the paper's second strategy for a round's new items, next to TopK ("Adaptive Selection of Anchor Items for CUR-based k-NN search
 *   with Cross-Encoders"); negatives for distillation sampled from the approximate score distribution   utils/data_process.py:343-365
 * Sampling without replacement is Gumbel top-k: the k largest of key(q, i) = S[q, i] / T + g(q, i) with g i.i.d. standard Gumbel.
 * THE NOISE (a contract): g is a pure function of (seed, stream_id, row key, item id) -- not of the launch shape, the row chunking or the
 * row's position in the call --, so a draw is reproducible and can be restated on the host:
 *   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31        (uint64, wrapping)
 *   base = mix64(seed + 0x9E3779B97F4A7C15 * ((uint64)stream_id + 1))
 *   z    = mix64(base ^ ((uint64)row_key << 32 | (uint64)item))
 *   u    = ((z >> 41) + 0.5) * 2^-23          23 bits: exactly representable in fp32, strictly inside (0, 1)
 *   g    = -logf(-logf(u))                    the accurate logf, no fast intrinsic; g lies in [-2.82, 16.64], always finite
 *   key  = __fadd_rn(__fmul_rn(s, inv_T), g)  two separately rounded fp32 operations, never contracted to an fma
 * so key equals numpy.float32(numpy.float32(s * inv_T) + g) for the device's g.
 *
 * anncur_sample_topk: S float[Q x I] with row pitch lds >= I (the pad is never read; S is read once and never written).  row_keys
 *   int32[Q], read as uint32; NULL = the row number.  The exclusion arguments are anncur_filter_topk's: excl_off != NULL: query q never
 *   draws excl_ids[excl_off[q] .. excl_off[q+1]) (int64[Q + 1]); excl_off == NULL: no query draws excl_ids[0 .. n_excl_shared); segments
 *   STRICTLY ASCENDING, trusted; excl_ids may be NULL when there is nothing to exclude.
 *   out_key float[Q x k], out_idx int32[Q x k], contiguous: the k allowed items with the largest keys, key descending, ties by the
 *   smaller id; out_key holds the perturbed keys.  A NaN score is never selected, -inf is an ordinary candidate (its key is -inf),
 *   (-inf, -1) pads a row with fewer than k allowed non-NaN items.
 *   1 <= k <= min(I, ANNCUR_MAX_TOPK), I < 2^31, inv_T = 1 / T finite and > 0, 0 <= Q < 2^31 (Q == 0 returns OK); anything else is
 *   ANNCUR_E_INVALID and nothing is written.  One workgroup per query, no workspace.
 * anncur_gumbel_noise: out float[Q x I] (pitch ldo >= I) = g(q, i) alone, from the device function the sampler calls: for tests and for
 *   auditing a draw; the sampler itself never materialises it.  1 <= I <= 2^31 (item ids are 31-bit), Q >= 0. */
int anncur_sample_topk(const float *S, int64_t lds, int64_t Q, int64_t I, float inv_T, uint64_t seed, uint32_t stream_id,
                       const int32_t *row_keys, const int64_t *excl_off, const int32_t *excl_ids, int64_t n_excl_shared, int32_t k,
                       float *out_key, int32_t *out_idx, void *stream);
int anncur_gumbel_noise(uint64_t seed, uint32_t stream_id, const int32_t *row_keys, int64_t Q, int64_t I, float *out, int64_t ldo,
                        void *stream);

/* anchor item selection by column-pivoted QR ---------------------------------------------------------------------------
 *   replaces sorted(rng.choice(n_ent, n_anc, replace=False)), the index' choice of its anchor items        ..._splits.py:295
 * Column-subset selection for CUR: greedily the item whose score column has the largest component outside the span of those taken so far.
 * R [kq x m] row-major, dtype ANNCUR_F32 or ANNCUR_BF16 (widened exactly), row pitch ldr >= m (the pad is never read): the layout CURApprox
 * and CURRowIndex hold their rows in.  Outputs (device): out_ids int32[k] = the selected items in SELECTION ORDER, out_gain double[k] = the
 * squared residual norm each had when it was taken, n_sel int32[1]; positions >= n_sel hold (-1, 0.0).  The selection is nested: the call
 * with k' < k returns the first k' entries of the call with k, bit for bit.
 * THE ALGORITHM (a contract; all state is fp64):
 *   d_i = sum_a R[a,i]^2                                    fma in ascending a
 *   step t:  p = argmax_i d_i over the items not yet taken, ties -> the smaller id; an item whose d_i is NaN or +-inf is never taken
 *            STOP (this and every later step does nothing) if there is no such item, d_p <= 0 or d_p <= 2^-40 d_first, d_first = step 0's d_p
 *            ids[t] = p, gain[t] = d_p
 *            q_t = R[:, p] orthogonalised against q_0 .. q_{t-1} TWICE (classical Gram-Schmidt: the t coefficients <q_j, v> from one vector,
 *                  then v -= sum_j coef_j q_j; the whole pass a second time), then divided by its norm
 *            c_i = sum_a R[a,i] q_t[a]                      fma in ascending a
 *            d_i <- fma(-c_i, c_i, d_i);   item p is marked (its d becomes NaN) and cannot be taken again
 * Every sum runs in an order fixed by kq alone -- never by m, the launch shape or the dispatch order --, so a result is bit-reproducible from
 * call to call.  (A residual column whose computed norm is 0 or not finite would stop the selection too; it cannot arise while d tracks the
 * residual to kq 2^-53 d_first.)
 * STOP RULE = anncur_lstsq_rows' PIVOT RULE, on purpose: d_p is the Cholesky pivot of R_S^T R_S that the item-side solve meets on the selected
 * block in selection order, so a set that passes here is one that solve accepts (status 0).
 * Two launches per step on `stream`, the kernel boundary the only synchronisation: a step kernel over slices of
 * anncur_select_pivoted_slice_items(dtype) items (each step reads R once: k kq m elements in all) and a one-workgroup pick kernel; no host
 * synchronisation; after a stop the remaining launches read the flag and return.  16-byte loads where R and ldr are multiples of 16 bytes,
 * element loads otherwise (same result).
 * Limits: 1 <= k <= min(kq, m, ANNCUR_MAX_TOPK), 1 <= kq <= ANNCUR_LSTSQ_MAX_KQ, m < 2^31; anything else is ANNCUR_E_INVALID and nothing is
 * written.  Workspace: caller-owned, 256-byte aligned, anncur_select_pivoted_workspace_bytes(m, kq, k) bytes (0 outside the limits) = a
 * header, d[m], the basis [k x kq], one (value, id) per step-kernel workgroup; nothing in it is pre-filled; missing, short or misaligned:
 * ANNCUR_E_WORKSPACE. */
size_t anncur_select_pivoted_workspace_bytes(int64_t m, int32_t kq, int32_t k);
int32_t anncur_select_pivoted_slice_items(int dtype);   /* items per slice of the step kernel (0 for an unknown dtype): for tests of its edges */
int anncur_select_pivoted(const void *R, int dtype, int64_t ldr, int32_t kq, int64_t m, int32_t k, int32_t *out_ids, double *out_gain,
                          int32_t *n_sel, void *workspace, size_t workspace_bytes, void *stream);

/* a3b: singular value decomposition of ONE block by one-sided (Hestenes) Jacobi rotations in fp64, and the truncated pseudo-inverse --------
 *   U = numpy.linalg.pinv(W) with a cutoff the caller chooses                                               eval/matrix_approx_zeshel.py:47,49
 * (the reference's call fixes rcond = 1e-15; Newton-Schulz, the other device route, has no notion of a cutoff).  DESIGN 4.5a.
 * W [rows x cols] row-major, dtype ANNCUR_F32 or ANNCUR_BF16 (widened exactly), row pitch ldw >= cols (the pad is never read).
 * g = min(rows, cols), L = max(rows, cols).  The g short-side vectors of W -- its columns if rows >= cols, else its rows -- are made mutually
 * orthogonal; their norms are the singular values.
 * WORKSPACE (caller-owned, 256-byte aligned, anncur_svd_workspace_bytes(rows, cols) bytes, 0 outside the limits; nothing in it is pre-filled):
 *   H  [g x Lp] fp64, row i = vector i;  Vt [g x gp] fp64, starts as the identity;  Lp, gp = L, g rounded up to 32.  The pad is never read.
 * THE ALGORITHM (a contract):
 *   a sweep = the gE - 1 steps of the round-robin tournament on gE = g rounded up to even (circle method); in step s pair p holds
 *       (gE - 1, s) for p = 0,   ((s + p) mod (gE - 1), (s - p + gE - 1) mod (gE - 1)) for p >= 1;   a pair with an index >= g idles
 *   the pair (i, j), i < j:  alpha = |h_i|^2, beta = |h_j|^2, gamma = h_i . h_j, recomputed from the rows every time
 *       rotate iff alpha > 0, beta > 0 and |gamma| > sqrt(L) 2^-53 sqrt(alpha) sqrt(beta)        (dgesvj's tolerance)
 *       zeta = (beta - alpha) / (2 gamma),  t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2))  (t = 1 at zeta = 0),  c = 1 / sqrt(1 + t^2),  s = c t
 *       h_i <- c h_i - s h_j,  h_j <- s h_i + c h_j;  the same on rows i, j of Vt
 *   each sum: thread t of 256 takes the elements t, t + 256, .. by fma in ascending order, the lanes of a wave are combined by the xor
 *       butterfly 32 .. 1, the four waves are added in wave order: an order fixed by L alone, so a result is bit-reproducible from call to call
 * One launch per step, one workgroup per pair; the pairs of a step touch disjoint rows and the kernel boundary orders the steps: no
 * cooperative launch, no workgroup waits for another, no loop without a bound, no floating-point atomics.
 *  anncur_svd_init    widens W into H and sets Vt = I.
 *  anncur_svd_sweep   one sweep (gE - 1 launches).  rotations int32[1] (device) is zeroed on the stream first and then counts the pairs that
 *                     rotated (an integer atomic): 0 after a sweep means converged.  The caller's loop reads these 4 bytes; no call here
 *                     synchronises.
 *  anncur_svd_finish  sigma double[g] = |h_i| (in the workspace's order, NOT sorted), the normalised h_i (zeros where sigma_i = 0) and Vt^T in
 *                     W's own orientation: rows >= cols: U [rows x g] = the normalised vectors, V [cols x g] = Vt^T; rows < cols: U [rows x g] =
 *                     Vt^T, V [cols x g] = the normalised vectors; so W = U diag(sigma) V^T.  Row pitches ldu, ldv >= g; nothing beyond column g
 *                     of a row is written.  flag int32[1] (device): zeroed on the stream, then 1 if any sigma_i is not finite.
 *  anncur_svd_scale_cols  out[r, i] = V[r, i] / sigma[i] where sigma[i] > rcond max(sigma), else 0, for r < n (numpy.linalg.pinv's rule;
 *                     the pseudo-inverse is out . U^T); rank int32[1] (device) = the number of sigma kept.  0 <= rcond < 1, 1 <= n <= ANNCUR_SVD_MAX_L.
 * Limits: 1 <= g <= ANNCUR_SVD_MAX_G, L <= ANNCUR_SVD_MAX_L; anything else is ANNCUR_E_INVALID and nothing is written; a missing, short or
 * misaligned workspace is ANNCUR_E_WORKSPACE.  Every launch is asynchronous on `stream`; nothing is allocated. */
#define ANNCUR_SVD_MAX_G 2048
#define ANNCUR_SVD_MAX_L 8192
size_t anncur_svd_workspace_bytes(int64_t rows, int64_t cols);
int anncur_svd_init(const void *W, int dtype, int64_t ldw, int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, void *stream);
int anncur_svd_sweep(int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, int32_t *rotations, void *stream);
int anncur_svd_finish(int64_t rows, int64_t cols, const void *workspace, size_t workspace_bytes, double *sigma, double *U, int64_t ldu, double *V,
                      int64_t ldv, int32_t *flag, void *stream);
int anncur_svd_scale_cols(const double *V, int64_t ldv, int64_t n, int32_t g, const double *sigma, double rcond, double *out, int64_t ldo,
                          int32_t *rank, void *stream);

/* f3: IVF-flat inner-product index (the branch of build_flat_or_ivff_index above 11 000 vectors) -------------------------------
 *   faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT).train / .add / .search     models/nearest_nbr.py:40-52
 * FAISS is not vendored nor pinned by the reference (parity unpinned): restated from the published algorithm, judged on recall
 * against the exact search.  The dense steps (points x centroids, queries x centroids -> top-nprobe) are anncur_gemm +
 * anncur_rowwise_topk; these three hold what is particular to the inverted file.
 *  anncur_ivf_build_lists: assign int32[n] (list of every point) -> counts int32[nlist], offsets int32[nlist+1] (exclusive prefix),
 *    ids int32[n] (points of list l at ids[offsets[l] .. offsets[l+1]) in ascending id order; deterministic, no atomics);
 *  anncur_ivf_list_means: centroids[l] = mean of rows offsets[l]..offsets[l+1] of Xs (vectors stored in list order), summed in
 *    list order; an empty list keeps its centroid (k-means update step);
 *  anncur_renorm_rows: every row of the fp32 matrix M rescaled to unit L2 norm in place (a zero row stays) -- FAISS' fvec_renorm_L2:
 *    IndexIVF trains its coarse quantiser with cp.spherical = true for METRIC_INNER_PRODUCT, i.e. the centroids are renormalised after
 *    every k-means update (faiss/IndexIVF.cpp Level1Quantizer::train_q1; the reference reaches it through models/nearest_nbr.py:46-49);
 *  anncur_ivf_scan: per query, exact inner products with every vector of its nprobe lists (probe int32[nq x nprobe], -1 = skip)
 *    and the k best: out_val float[nq x k] descending, out_idx int32[nq x k] (ids of the points; (-inf, -1) where the probed lists
 *    hold fewer than k vectors).  Xs / Q rows zero-padded to dp floats, dp a multiple of 16, 16-byte aligned.  Subnormal vector or
 *    query entries and subnormal inner products are kept, here and in the batched searches below. */
int anncur_ivf_build_lists(const int32_t *assign, int64_t n, int32_t nlist, int32_t *counts, int32_t *offsets, int32_t *ids, void *stream);
int anncur_ivf_list_means(const float *Xs, int64_t ldx, int32_t d, const int32_t *offsets, int32_t nlist, float *centroids, int64_t ldc, void *stream);
int anncur_renorm_rows(float *M, int64_t n_rows, int64_t n_cols, int64_t ld, void *stream);
int anncur_ivf_scan(const float *Xs, int64_t ldx, int32_t dp, const int32_t *offsets, const int32_t *ids, const float *Q, int64_t ldq, int64_t nq,
                    const int32_t *probe, int32_t nprobe, int32_t k, float *out_val, int32_t *out_idx, void *stream);

/* Batched IVF search (many queries, e.g. the reference's hard-negative mining, utils/data_process.py:343-365, where every mention
 * queries the index): the (query, probe slot) pairs are sorted by list -- anncur_ivf_build_lists on the flattened probe array gives
 * pair_offsets[nlist+1] and pair_ids (pair = q * nprobe + slot) -- and every list is scored against its pairs' queries as a small GEMM on
 * the matrix cores, in 64-pair x 64-vector tiles, so a list's vectors are read once per 64 queries instead of once per query.
 * SLOTTED scores: S float[nq * nprobe x lmax] (lmax >= longest list), pre-filled with -inf by the caller; row pair = q * nprobe + slot
 * holds S[pair][position in its list] = <query, vector>.  Then anncur_rowwise_topk over S viewed as [nq x nprobe * lmax] and
 * anncur_ivf_map_ids (column -> id of the vector; -1 where the score is the -inf padding).
 * Operands: dtype ANNCUR_F32 -- Xs / Q fp32 rows of dp >= 1 floats, products and sums exact fp32 (v_mfma_f32_32x32x2_f32) -- or
 * ANNCUR_BF16 -- Xs / Q bf16 rows zero-padded to dp elements, dp a multiple of 16, ldx / ldq multiples of 8, 16-byte aligned (an index
 * built with dtype = "bf16" keeps such a copy of its lists): v_mfma_f32_32x32x16_bf16, fp32 accumulation, fp32 scores.
 * The tile worklist is built ON THE DEVICE (no host look at the pairs-per-list counts, no synchronisation inside a search):
 * tile_start int32[nlist + 1] is filled here (tile_start[l] = tiles of the lists before l), the GEMM is launched with max_tiles
 * workgroups -- any upper bound on sum_l ceil(pairs_l / 64) ceil(size_l / 64), e.g. (n_pairs / 64) * max_l ceil(size_l / 64) +
 * sum_l ceil(size_l / 64) -- and workgroup b finds its (list, pair tile, vector tile) by binary search; workgroups past the last tile
 * exit (max_tiles = 0: tile_start only). */
int anncur_ivf_group_scores_dev(const void *Xs, int dtype, int64_t ldx, int32_t dp, const int32_t *offsets, int32_t nlist, const void *Q, int64_t ldq,
                                int32_t nprobe, const int32_t *pair_ids, const int32_t *pair_offsets, int32_t *tile_start, int32_t max_tiles, int64_t lmax,
                                float *S, void *stream);
int anncur_ivf_map_ids(const int32_t *col, const float *val, int64_t nq, int32_t k, int64_t lmax, const int32_t *probe, int32_t nprobe,
                       const int32_t *offsets, const int32_t *ids, int32_t *out_idx, void *stream);

/* The batched search as ONE stream-ordered call (round 5) -- faiss.IndexIVFFlat.search for many queries, models/nearest_nbr.py:50-52 as
 * the reference's hard-negative mining drives it (utils/data_process.py:343-365).  From the probed lists (probe int32[nq x nprobe], entries
 * outside 0..nlist-1 skipped) to the k best (out_val float[nq x k] descending, out_idx int32[nq x k] ids; (-inf, -1) where the probed lists
 * hold fewer than k vectors): pairs grouped by list on the device, one tile GEMM launch on the matrix cores (bf16 rows with dp a multiple
 * of 128: 128 x 128 tiles, v_mfma_f32_32x32x16_bf16; fp32 rows or other bf16 row lengths: the 64 x 64 tiles of anncur_ivf_group_scores_dev),
 * scores written to PACKED rows -- S float[nq x pitch], 16-byte aligned, query q's probed lists back to back, nothing pre-filled -- and
 * scanned by anncur_rowwise_topk_ragged.  Xs / Q: the operand contracts of anncur_ivf_group_scores_dev (dtype selects fp32 or bf16 rows for BOTH).
 * pitch >= max(k, longest packed row) -- nprobe x longest list always suffices -- a multiple of 4, nq x pitch < 2^32 (split the queries); a
 * probed list that no longer fits a query's row is left out of that query's search (a pitch below the contract loses candidates, never memory).
 * max_tiles: any upper bound on sum_l ceil(pairs_l / T) ceil(size_l / T), T = anncur_ivf_search_tile(...) (the launch's grid: workgroups
 * past the last tile exit), e.g. (nq nprobe / T) max_l ceil(size_l / T) + sum_l ceil(size_l / T).  k <= 128 and nlist <= 8192
 * (ANNCUR_E_UNSUPPORTED otherwise: the calls above).  Workspace: anncur_ivf_search_workspace_bytes, 256-byte aligned.
 * All three tile bodies (fp32 and bf16 64 x 64, bf16 128 x 128) read subnormal operands as they are and keep subnormal scores. */
int32_t anncur_ivf_search_tile(int dtype, int32_t dp, int64_t ldx, int64_t ldq, int64_t nq);
size_t anncur_ivf_search_workspace_bytes(int64_t nq, int32_t nprobe, int32_t nlist, int32_t k, int64_t max_tiles);
int anncur_ivf_search_grouped(const void *Xs, int dtype, int64_t ldx, int32_t dp, const int32_t *offsets, const int32_t *ids, int32_t nlist,
                              const void *Q, int64_t ldq, int64_t nq, const int32_t *probe, int32_t nprobe, int32_t k, int64_t max_tiles,
                              float *S, int64_t pitch, void *workspace, size_t workspace_bytes, float *out_val, int32_t *out_idx, void *stream);

/* Index-build hint of anncur_score_topk_ex: bucket[i] in 0..n_buckets-1 by the squared norm of row i of the fp32 matrix A, largest
 * norms first (linear between the matrix' largest and smallest row norm); norms float[n_rows] and minmax2 uint32[2] are scratch
 * outputs.  anncur_ivf_build_lists(bucket, n_rows, n_buckets, ...) then returns the rows in coarse descending-norm order (a stable
 * counting sort): the order in which CURApprox stores the hint copy of E^T (matrix_approx_zeshel.py:65 builds latent_cols; the
 * ordering is this build's own and only moves speed). */
int anncur_norm_buckets(const float *A, int64_t n_rows, int64_t n_cols, int64_t lda, int32_t n_buckets, float *norms, uint32_t *minmax2,
                        int32_t *bucket, void *stream);

/* dtype plumbing: fp32 <-> bf16 (round-to-nearest-even), strided 2-D ------------------ */
int anncur_convert(const void *src, int src_dtype, int64_t lds_, void *dst, int dst_dtype, int64_t ldd,
                   int64_t n_rows, int64_t n_cols, void *stream);

/* Device-side byte copy (16-byte vector stores); `dst` may be mapped pinned HOST memory, so small per-step results
 * (the 4*Q overlap counts the reference's statistics are computed from, eval/eval_utils.py:131-136) reach the host from inside a
 * captured graph without a copy-engine hop.  src / dst 16-byte aligned. */
int anncur_copy_bytes(const void *src, void *dst, size_t nbytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANNCUR_HIP_H */
