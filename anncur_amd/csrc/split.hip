// The split-bf16 ("bf16x3") route's two kernels: the operand packer of the fused sweep and the fp32 rescore of its candidates.
//
// An fp32 operand x is written as hi + lo with hi = bf16(x), lo = bf16(x - hi) (round-to-nearest-even both; x - hi is exact in fp32).
// Then  x . e  ~=  lo_x hi_e + hi_x lo_e + hi_x hi_e,  which is ONE bf16 inner product of length 3K over
//     query row : [ lo(x) | hi(x) | hi(x) | 0 ]
//     item row  : [ hi(e) | lo(e) | hi(e) | 0 ]
// so anncur_score_topk_ex sweeps these operands unchanged with Kp = padded 3K (products exact, fp32 sums, the small terms first).
// Its candidates are then rescored by the k-ordered fp32 fmaf chain anncur_gemm is, and the caller sees the dense fp32 route's values.
#include "select.hpp"

using namespace anncur;

namespace {

// ------------------------------------------------------------------ pack
__device__ __forceinline__ bool bf16_bits_finite(uint16_t b) { return (b & 0x7f80u) != 0x7f80u; }

// element `seg` (0, 1, 2) of the split row for the source value at p: role 0 (query) [lo | hi | hi], role 1 (item) [hi | lo | hi]
template <typename T>
__device__ __forceinline__ uint16_t split_elem(const T *p, bool want_lo);
template <>
__device__ __forceinline__ uint16_t split_elem<float>(const float *p, bool want_lo) {
	const float x = *p;
	const uint16_t hi = f32_to_bf16_bits(x);
	if (!want_lo) return hi;
	if (!bf16_bits_finite(hi)) return 0;   // inf, NaN, or a finite x that rounds to inf: no inf - inf
	return f32_to_bf16_bits(x - bf16_bits_to_f32(hi));
}
template <>
__device__ __forceinline__ uint16_t split_elem<uint16_t>(const uint16_t *p, bool want_lo) { return want_lo ? (uint16_t)0 : *p; }

// One thread per 16-byte vector (8 bf16) of dst, pad columns and pad rows included: the kernel owns every byte of dst.
// The segments start at element offsets 0, K, 2K of a row -- any alignment --, so a vector is assembled element by element from the
// source (each source element is read three times, from cache).
template <typename T>
__global__ __launch_bounds__(256) void pack_split_kernel(const T *__restrict__ src, int64_t lds_, int64_t n_rows, int64_t K, int role,
														  uint16_t *__restrict__ dst, int64_t ldd, int64_t n_vec_row, int64_t n_vec) {
	const int lo_seg = role == 0 ? 0 : 1;
	for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vec; v += (int64_t)gridDim.x * 256) {
		const int64_t r = v / n_vec_row;
		const int64_t c0 = (v - r * n_vec_row) * 8;
		uint32_t w[4] = {0u, 0u, 0u, 0u};
		if (r < n_rows && c0 < 3 * K) {
			const T *row = src + r * lds_;
#pragma unroll
			for (int e = 0; e < 8; ++e) {
				const int64_t c = c0 + e;
				const int seg = (int)(c >= K) + (int)(c >= 2 * K);
				uint16_t b = 0;
				if (c < 3 * K) b = split_elem<T>(row + (c - seg * K), seg == lo_seg);
				w[e >> 1] |= (uint32_t)b << (16 * (e & 1));
			}
		}
		*reinterpret_cast<uint4 *>(dst + r * ldd + c0) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

// ------------------------------------------------------------------ rescore
constexpr int RS_WAVES = 4;       // queries per workgroup: one wave each
constexpr int RS_KC = 1024;       // floats of a query row staged in LDS at a time

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; };
template <> struct Vec16<uint16_t> { static constexpr int N = 8; };

// s = fmaf(x[k], e[k], s) for k = 0 .. n-1 in this order; x in LDS (every lane reads the same address: a broadcast), e this lane's row
template <typename TE, bool VEC>
__device__ __forceinline__ float chain(const float *x, const TE *e, int n, float s) {
	int k = 0;
	if (VEC) {
		constexpr int N = Vec16<TE>::N;
		for (; k + N <= n; k += N) {
			const uint4 u = *reinterpret_cast<const uint4 *>(e + k);
			const uint32_t w[4] = {u.x, u.y, u.z, u.w};
			if (N == 4) {
#pragma unroll
				for (int j = 0; j < 4; ++j) s = fmaf(x[k + j], __uint_as_float(w[j]), s);
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					s = fmaf(x[k + 2 * j], bf16_bits_to_f32(w[j] & 0xffffu), s);
					s = fmaf(x[k + 2 * j + 1], __uint_as_float(w[j] & 0xffff0000u), s);
				}
			}
		}
	}
	for (; k < n; ++k) s = fmaf(x[k], load_as_f32<TE>(e + k), s);
	return s;
}

// scratch[q, j] = the fp32 fmaf chain of <X[q, :], Et[cand[q, j], :]>, k ascending from 0 (bit for bit anncur_gemm's element); a hole
// (id < 0 or >= I) gets -inf and is left out by the select kernel through its id.  One wave per query, lane = candidate (j = lane,
// lane + 64, ...).  Rows longer than RS_KC run in chunks with the running sum parked in scratch between them.
template <typename TX, typename TE, bool VEC>
__global__ __launch_bounds__(RS_WAVES * WAVE) void rescore_kernel(const TX *__restrict__ X, int64_t ldx, const TE *__restrict__ Et, int64_t lde, int64_t K,
																   const int32_t *__restrict__ cand, int64_t ld_idx, int n_cand, int64_t Q, int64_t I,
																   float *__restrict__ scratch) {
	__shared__ __attribute__((aligned(16))) float xs[RS_WAVES][RS_KC];
	const int wave = threadIdx.x / WAVE, lane = lane_id();
	const int64_t q = (int64_t)blockIdx.x * RS_WAVES + wave;
	const bool live = q < Q;
	float *x = xs[wave];
	for (int64_t k0 = 0; k0 < K; k0 += RS_KC) {   // (K is uniform: every wave of the workgroup meets the same barriers)
		const int n = (int)(K - k0 < RS_KC ? K - k0 : RS_KC);
		__syncthreads();
		if (live)
			for (int k = lane; k < n; k += WAVE) x[k] = load_as_f32<TX>(X + q * ldx + k0 + k);
		__syncthreads();
		if (!live) continue;
		for (int j = lane; j < n_cand; j += WAVE) {
			const int32_t it = cand[q * ld_idx + j];
			float s = -INFINITY;
			if (it >= 0 && (int64_t)it < I) {
				s = k0 == 0 ? 0.f : scratch[q * n_cand + j];
				s = chain<TE, VEC>(x, Et + (int64_t)it * lde + k0, n, s);
			}
			scratch[q * n_cand + j] = s;
		}
	}
}

// the k_out best of one query's rescored candidates: score descending, ties by the smaller item id, NaN never selected, (-inf, -1) pad
template <int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void rescore_select_kernel(const float *__restrict__ scratch, const int32_t *__restrict__ cand, int64_t ld_idx,
																	  uint32_t n_cand, int64_t I, uint32_t k_out, float *__restrict__ out_val,
																	  int32_t *__restrict__ out_idx) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	sel_init(s);
	const int tid = threadIdx.x;
	const int64_t q = blockIdx.x;
	for (uint32_t j0 = 0; j0 < n_cand; j0 += SEL_THREADS) {   // n_cand <= 2048 <= SEL_PASS: no mid-stream compaction needed
		const uint32_t j = j0 + tid;
		const int32_t it = (j < n_cand) ? cand[q * ld_idx + j] : -1;
		const bool in = it >= 0 && (int64_t)it < I;
		const float v = in ? scratch[q * n_cand + j] : 0.f;
		sel_offer(s, in, v, (uint32_t)it, -INFINITY, 0ull);
	}
	sel_finish<KMAX>(s, k_out, out_val + q * (int64_t)k_out, out_idx + q * (int64_t)k_out);
}

}  // namespace

extern "C" int anncur_pack_split_bf16(const void *src, int src_dtype, int64_t lds_, int64_t n_rows, int64_t K, int role, void *dst, int64_t ldd,
									   int64_t n_rows_pad, void *stream) {
	ANNCUR_REQUIRE(dtype_ok(src_dtype), ANNCUR_E_INVALID, "pack_split_bf16: bad dtype %d", src_dtype);
	ANNCUR_REQUIRE(role == 0 || role == 1, ANNCUR_E_INVALID, "pack_split_bf16: role must be 0 (query) or 1 (item)");
	ANNCUR_REQUIRE(n_rows >= 0 && K >= 1 && lds_ >= K && n_rows_pad >= n_rows, ANNCUR_E_INVALID, "pack_split_bf16: bad shape");
	ANNCUR_REQUIRE(K <= ((int64_t)1 << 40) && ldd >= 3 * K && ldd % 8 == 0, ANNCUR_E_INVALID, "pack_split_bf16: ldd must be a multiple of 8 and >= 3 K");
	ANNCUR_REQUIRE(dst && (src || n_rows == 0), ANNCUR_E_INVALID, "pack_split_bf16: null pointer");
	ANNCUR_REQUIRE(((uintptr_t)dst & 15u) == 0, ANNCUR_E_INVALID, "pack_split_bf16: dst must be 16-byte aligned");
	if (n_rows_pad == 0) return ANNCUR_OK;
	const int64_t n_vec_row = ldd / 8, n_vec = n_rows_pad * n_vec_row;
	const int64_t want = ceil_div64(n_vec, 256);
	const unsigned grid = (unsigned)(want < (int64_t)anncur_num_cu() * 32 ? want : (int64_t)anncur_num_cu() * 32);
	hipStream_t st = (hipStream_t)stream;
	if (src_dtype == ANNCUR_F32)
		hipLaunchKernelGGL((pack_split_kernel<float>), dim3(grid), dim3(256), 0, st, (const float *)src, lds_, n_rows, K, role, (uint16_t *)dst, ldd, n_vec_row, n_vec);
	else
		hipLaunchKernelGGL((pack_split_kernel<uint16_t>), dim3(grid), dim3(256), 0, st, (const uint16_t *)src, lds_, n_rows, K, role, (uint16_t *)dst, ldd, n_vec_row,
						   n_vec);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_rescore_topk(const void *X, int x_dtype, int64_t ldx, const void *Et, int e_dtype, int64_t lde, int64_t K, const int32_t *cand_idx,
									int64_t ld_idx, int32_t n_cand, int64_t Q, int64_t I, int32_t k_out, float *out_val, int32_t *out_idx, float *scratch,
									void *stream) {
	ANNCUR_REQUIRE(dtype_ok(x_dtype) && dtype_ok(e_dtype), ANNCUR_E_INVALID, "rescore_topk: bad dtype %d / %d", x_dtype, e_dtype);
	ANNCUR_REQUIRE(Q >= 0 && I >= 1 && K >= 1 && ldx >= K && lde >= K && Q < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "rescore_topk: bad shape");
	ANNCUR_REQUIRE(n_cand >= 1 && n_cand <= ANNCUR_MAX_TOPK && k_out >= 1 && k_out <= n_cand, ANNCUR_E_INVALID,
				   "rescore_topk: need 1 <= k_out <= n_cand <= %d (got %d, %d)", ANNCUR_MAX_TOPK, k_out, n_cand);
	ANNCUR_REQUIRE(ld_idx >= n_cand, ANNCUR_E_INVALID, "rescore_topk: ld_idx < n_cand");
	ANNCUR_REQUIRE(X && Et && cand_idx && out_val && out_idx, ANNCUR_E_INVALID, "rescore_topk: null pointer");
	ANNCUR_REQUIRE(scratch, ANNCUR_E_WORKSPACE, "rescore_topk: scratch (float[Q x n_cand]) missing");
	if (Q == 0) return ANNCUR_OK;
	hipStream_t st = (hipStream_t)stream;
	// 16-byte loads of the item rows need aligned rows; anything else walks them element by element (same chain, same result)
	const bool vec = ((uintptr_t)Et & 15u) == 0 && (lde * (int64_t)dtype_size(e_dtype)) % 16 == 0;
	const dim3 grid((unsigned)ceil_div64(Q, RS_WAVES)), block(RS_WAVES * WAVE);
#define LAUNCH_RESCORE(TX, TE)                                                                                                                      \
	do {                                                                                                                                            \
		if (vec) hipLaunchKernelGGL((rescore_kernel<TX, TE, true>), grid, block, 0, st, (const TX *)X, ldx, (const TE *)Et, lde, K, cand_idx, ld_idx, \
									(int)n_cand, Q, I, scratch);                                                                                    \
		else hipLaunchKernelGGL((rescore_kernel<TX, TE, false>), grid, block, 0, st, (const TX *)X, ldx, (const TE *)Et, lde, K, cand_idx, ld_idx,  \
								(int)n_cand, Q, I, scratch);                                                                                        \
	} while (0)
	if (x_dtype == ANNCUR_F32) {
		if (e_dtype == ANNCUR_F32) LAUNCH_RESCORE(float, float); else LAUNCH_RESCORE(float, uint16_t);
	} else {
		if (e_dtype == ANNCUR_F32) LAUNCH_RESCORE(uint16_t, float); else LAUNCH_RESCORE(uint16_t, uint16_t);
	}
#undef LAUNCH_RESCORE
	ANNCUR_LAUNCH_OK();
#define LAUNCH_RSEL(KM)                                                                                                                              \
	do {                                                                                                                                             \
		{ const int rc_ = anncur_ensure_dyn_lds((const void *)rescore_select_kernel<KM>, (int)SelCfg<KM>::LDS_BYTES); if (rc_ != ANNCUR_OK) return rc_; } \
		hipLaunchKernelGGL((rescore_select_kernel<KM>), dim3((unsigned)Q), dim3(SEL_THREADS), SelCfg<KM>::LDS_BYTES, st, scratch, cand_idx, ld_idx,  \
						   (uint32_t)n_cand, I, (uint32_t)k_out, out_val, out_idx);                                                                  \
	} while (0)
	if (k_out <= 128) LAUNCH_RSEL(128); else if (k_out <= 512) LAUNCH_RSEL(512); else LAUNCH_RSEL(2048);
#undef LAUNCH_RSEL
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
