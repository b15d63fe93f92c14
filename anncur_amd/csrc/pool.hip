// Re-rank from caller-supplied scores: the last step of a search that never holds the exact [Q x I] matrix.
//
// anncur_rerank looks exact scores up in a resident matrix; a caller who SEARCHES holds them in two other forms -- the anchor items' scores
// X [Q x kc] with one id list for all queries, and the scores of the candidates it retrieved, in candidate order, one id per cell.  The pool
// of a query is the union of the two, and rerank_scored_kernel returns its k_out best.  gather_pairs_kernel is the exact-score source of the
// evaluation mode: the cells A[q, idx[q, j]] of a stored matrix, in candidate order.
#include "select.hpp"

using namespace anncur;

namespace {

// One 256-thread workgroup per query on the workgroup selector of select.hpp, as rerank_kernel.  The pool may exceed SEL_PASS offers
// (up to 65535 shared entries), so -- unlike rerank_kernel and rescore_select_kernel -- the stream is cut into batches of SEL_PASS offers
// with the selector's overflow check between them; `pending` counts the offers since the last check and runs across the two sources.
// A per-query entry whose id occurs among the shared ids is dropped (the shared score stands): every lane binary-searches its id in the
// ascending shared list, a fixed number of steps for the whole workgroup.  The keys of a row are therefore distinct.
template <typename TS, int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void rerank_scored_kernel(const int32_t *__restrict__ sh_ids, const TS *__restrict__ sh_val, int64_t ld_sh,
																		 uint32_t n_sh, const int32_t *__restrict__ pq_idx, const float *__restrict__ pq_val,
																		 int64_t ld_pq, uint32_t n_pq, uint32_t k_out, float *__restrict__ out_val,
																		 int32_t *__restrict__ out_idx) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	sel_init(s);
	const uint32_t tid = threadIdx.x;
	const int64_t q = blockIdx.x;
	float tau = -INFINITY;
	uint64_t tau_key = 0;
	uint32_t pending = 0;   // (uniform)
	const TS *sv = sh_val + q * ld_sh;
	for (uint32_t j0 = 0; j0 < n_sh; j0 += SEL_THREADS) {
		const uint32_t j = j0 + tid;
		const bool in = j < n_sh;
		const float v = in ? load_as_f32<TS>(sv + j) : 0.f;
		const uint32_t id = in ? (uint32_t)sh_ids[j] : 0u;
		sel_offer(s, in, v, id, tau, tau_key);   // (NaN fails v >= tau: never pushed)
		pending += SEL_THREADS;
		if (pending == (uint32_t)SEL_PASS) { sel_maybe_compact<KMAX>(s, k_out, tau, tau_key); pending = 0; }
	}
	const int32_t *pi = pq_idx + q * ld_pq;
	const float *pv = pq_val + q * ld_pq;
	for (uint32_t j0 = 0; j0 < n_pq; j0 += SEL_THREADS) {
		const uint32_t j = j0 + tid;
		const bool in = j < n_pq;
		const int32_t id = in ? pi[j] : -1;
		const float v = in ? pv[j] : 0.f;
		bool dup = false;
		if (n_sh) {
			// lower bound without a lane-dependent branch (filter_topk_kernel): pos + half - 1 < n_sh throughout
			uint32_t pos = 0, len = n_sh;
			while (len > 1) {
				const uint32_t half = len >> 1;
				pos += (sh_ids[pos + half - 1] < id) ? half : 0u;
				len -= half;
			}
			dup = sh_ids[pos] == id;
		}
		sel_offer(s, id >= 0 && !dup, v, (uint32_t)id, tau, tau_key);
		pending += SEL_THREADS;
		if (pending == (uint32_t)SEL_PASS) { sel_maybe_compact<KMAX>(s, k_out, tau, tau_key); pending = 0; }
	}
	sel_finish<KMAX>(s, k_out, out_val + q * (int64_t)k_out, out_idx + q * (int64_t)k_out);
}

// out[q, j] = A[q, idx[q, j]] as float: one wave per row, four rows per workgroup, four element loads in flight per lane
// (gather_cols_kernel's shape; here the ids differ per row, so they are a coalesced read of the row's own list).
template <typename TS>
__global__ __launch_bounds__(256) void gather_pairs_kernel(const TS *__restrict__ A, int64_t Q, int64_t I, int64_t lda, const int32_t *__restrict__ idx,
															int64_t ld_idx, int32_t n, float *__restrict__ out, int64_t ldo) {
	const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (q >= Q) return;
	const TS *row = A + q * lda;
	const int32_t *ri = idx + q * ld_idx;
	float *ro = out + q * ldo;
	constexpr int U = 4;
	for (int j0 = threadIdx.x & 63; j0 < n; j0 += 64 * U) {
		int32_t c[U];
		float v[U];
#pragma unroll
		for (int u = 0; u < U; ++u) c[u] = (j0 + 64 * u < n) ? ri[j0 + 64 * u] : -1;
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const bool in = c[u] >= 0 && (int64_t)c[u] < I;
			v[u] = in ? load_as_f32<TS>(row + c[u]) : __uint_as_float(0x7fc00000u);   // an id outside [0, I): NaN, which no selector takes
		}
#pragma unroll
		for (int u = 0; u < U; ++u)
			if (j0 + 64 * u < n) ro[j0 + 64 * u] = v[u];
	}
}

int pool_kmax_class(int k) { return k <= 128 ? 128 : (k <= 512 ? 512 : 2048); }   // as kmax_class of topk.hip

template <typename TS, int KM>
int launch_rerank_scored(const int32_t *sh_ids, const void *sh_val, int64_t ld_sh, int64_t n_sh, const int32_t *pq_idx, const float *pq_val, int64_t ld_pq,
						 int32_t n_pq, int64_t Q, int32_t k_out, float *out_val, int32_t *out_idx, hipStream_t st) {
	const int rc = anncur_ensure_dyn_lds((const void *)rerank_scored_kernel<TS, KM>, (int)SelCfg<KM>::LDS_BYTES);
	if (rc != ANNCUR_OK) return rc;
	hipLaunchKernelGGL((rerank_scored_kernel<TS, KM>), dim3((unsigned)Q), dim3(SEL_THREADS), SelCfg<KM>::LDS_BYTES, st, sh_ids, (const TS *)sh_val, ld_sh,
					   (uint32_t)n_sh, pq_idx, pq_val, ld_pq, (uint32_t)n_pq, (uint32_t)k_out, out_val, out_idx);
	return ANNCUR_OK;
}

template <typename TS>
int launch_rerank_scored_k(int kc, const int32_t *sh_ids, const void *sh_val, int64_t ld_sh, int64_t n_sh, const int32_t *pq_idx, const float *pq_val,
						   int64_t ld_pq, int32_t n_pq, int64_t Q, int32_t k_out, float *out_val, int32_t *out_idx, hipStream_t st) {
	if (kc == 128) return launch_rerank_scored<TS, 128>(sh_ids, sh_val, ld_sh, n_sh, pq_idx, pq_val, ld_pq, n_pq, Q, k_out, out_val, out_idx, st);
	if (kc == 512) return launch_rerank_scored<TS, 512>(sh_ids, sh_val, ld_sh, n_sh, pq_idx, pq_val, ld_pq, n_pq, Q, k_out, out_val, out_idx, st);
	return launch_rerank_scored<TS, 2048>(sh_ids, sh_val, ld_sh, n_sh, pq_idx, pq_val, ld_pq, n_pq, Q, k_out, out_val, out_idx, st);
}

}  // namespace

extern "C" int anncur_rerank_scored(const int32_t *sh_ids, const void *sh_val, int sh_dtype, int64_t ld_sh, int64_t n_sh, const int32_t *pq_idx,
									 const float *pq_val, int64_t ld_pq, int32_t n_pq, int64_t Q, int32_t k_out, float *out_val, int32_t *out_idx,
									 void *stream) {
	ANNCUR_REQUIRE(dtype_ok(sh_dtype), ANNCUR_E_INVALID, "rerank_scored: bad dtype %d", sh_dtype);
	ANNCUR_REQUIRE(Q >= 0 && Q < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "rerank_scored: need 0 <= Q < 2^31 (got %lld)", (long long)Q);
	ANNCUR_REQUIRE(n_sh >= 0 && n_sh <= 65535, ANNCUR_E_INVALID, "rerank_scored: need 0 <= n_sh <= 65535 (got %lld)", (long long)n_sh);
	ANNCUR_REQUIRE(n_pq >= 0 && n_pq <= ANNCUR_MAX_TOPK, ANNCUR_E_INVALID, "rerank_scored: need 0 <= n_pq <= %d (got %d)", ANNCUR_MAX_TOPK, (int)n_pq);
	ANNCUR_REQUIRE(n_sh + n_pq >= 1, ANNCUR_E_INVALID, "rerank_scored: the pool is empty (n_sh + n_pq = 0)");
	ANNCUR_REQUIRE(k_out >= 1 && k_out <= ANNCUR_MAX_TOPK && (int64_t)k_out <= n_sh + n_pq, ANNCUR_E_INVALID,
				   "rerank_scored: need 1 <= k_out <= min(%d, n_sh + n_pq = %lld) (got %d)", ANNCUR_MAX_TOPK, (long long)(n_sh + n_pq), (int)k_out);
	ANNCUR_REQUIRE(ld_sh >= n_sh && ld_pq >= n_pq, ANNCUR_E_INVALID, "rerank_scored: a row pitch is shorter than its row (ld_sh %lld < n_sh %lld or ld_pq %lld < n_pq %d)",
				   (long long)ld_sh, (long long)n_sh, (long long)ld_pq, (int)n_pq);
	ANNCUR_REQUIRE(n_sh == 0 || (sh_ids && sh_val), ANNCUR_E_INVALID, "rerank_scored: sh_ids / sh_val is NULL but n_sh = %lld", (long long)n_sh);
	ANNCUR_REQUIRE(n_pq == 0 || (pq_idx && pq_val), ANNCUR_E_INVALID, "rerank_scored: pq_idx / pq_val is NULL but n_pq = %d", (int)n_pq);
	ANNCUR_REQUIRE(out_val && out_idx, ANNCUR_E_INVALID, "rerank_scored: null output pointer");
	if (Q == 0) return ANNCUR_OK;
	hipStream_t st = (hipStream_t)stream;
	const int kc = pool_kmax_class(k_out);
	const int rc = sh_dtype == ANNCUR_F32
					   ? launch_rerank_scored_k<float>(kc, sh_ids, sh_val, ld_sh, n_sh, pq_idx, pq_val, ld_pq, n_pq, Q, k_out, out_val, out_idx, st)
					   : launch_rerank_scored_k<uint16_t>(kc, sh_ids, sh_val, ld_sh, n_sh, pq_idx, pq_val, ld_pq, n_pq, Q, k_out, out_val, out_idx, st);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_gather_pairs(const void *A, int dtype, int64_t Q, int64_t I, int64_t lda, const int32_t *idx, int64_t ld_idx, int32_t n, float *out,
									int64_t ldo, void *stream) {
	ANNCUR_REQUIRE(dtype_ok(dtype), ANNCUR_E_INVALID, "gather_pairs: bad dtype %d", dtype);
	ANNCUR_REQUIRE(Q >= 0 && Q < (int64_t)0x7fffffff && I >= 1 && lda >= I && n >= 0 && ld_idx >= n && ldo >= n, ANNCUR_E_INVALID, "gather_pairs: bad shape");
	if (Q == 0 || n == 0) return ANNCUR_OK;   // (empty tensors have null data pointers: nothing to do comes first)
	ANNCUR_REQUIRE(A && idx && out, ANNCUR_E_INVALID, "gather_pairs: null pointer");
	hipStream_t st = (hipStream_t)stream;
	if (dtype == ANNCUR_F32)
		hipLaunchKernelGGL((gather_pairs_kernel<float>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), 0, st, (const float *)A, Q, I, lda, idx, ld_idx, n, out, ldo);
	else
		hipLaunchKernelGGL((gather_pairs_kernel<uint16_t>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), 0, st, (const uint16_t *)A, Q, I, lda, idx, ld_idx, n, out, ldo);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
