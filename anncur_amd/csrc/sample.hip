// SoftMax item sampling: k items per row drawn without replacement with probability proportional to softmax(S / T), as
// Gumbel top-k -- the k largest of key(q, i) = S[q, i] / T + g(q, i), g i.i.d. standard Gumbel (gumbel.hpp).  The perturbation differs per
// (query, item) pair, so no top-k route of this library can carry it: the row of scores is read once and the keys exist only in registers.
#include "select.hpp"
#include "gumbel.hpp"

using namespace anncur;

namespace {

// native 16-byte vector (topk.hip: HIP's float4 struct gets scalarised when used conditionally)
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SMP_VEC = 4;                                         // floats per 16-byte load
constexpr int SMP_U = SEL_PASS / (SEL_THREADS * SMP_VEC);          // vectors per thread between two overflow checks of the selector
constexpr int64_t SMP_STEP = (int64_t)SEL_THREADS * SMP_U;         // vectors per batch

// One 256-thread workgroup per query on the workgroup selector of select.hpp.  The row is cut into its unaligned head and tail (fewer than
// four elements each, offered first) and 16-byte vectors, streamed in batches of SEL_PASS offers with the selector's overflow check between
// them (rerank_scored_kernel's shape); the next batch's vectors are in flight while the current one is hashed.  The loads are unconditional
// on a clamped index and `ok` masks the offers (rowwise_topk_kernel), so nothing outside the row's I elements is read.
// A vector none of whose keys can reach the threshold -- scaled score + the noise's upper bound below tau, for the whole wave -- skips the
// hash and the logarithms; only keys that would be pushed (key >= tau) pay the exclusion test, filter_topk_kernel's branch-free lower bound
// in the query's ascending segment.  A NaN score gives a NaN key, which fails key >= tau; -inf is an ordinary candidate with key -inf.
template <int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void sample_topk_kernel(const float *__restrict__ S, int64_t lds, int64_t I, float inv_T, uint64_t base,
																   const int32_t *__restrict__ row_keys, const int64_t *__restrict__ excl_off,
																   const int32_t *__restrict__ excl_ids, int64_t n_excl_shared, uint32_t k,
																   float *__restrict__ out_key, int32_t *__restrict__ out_idx) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	sel_init(s);
	const int tid = threadIdx.x;
	const int64_t q = blockIdx.x;
	const float *row = S + q * lds;
	const uint64_t noise_row = gumbel_row(base, row_keys ? (uint32_t)row_keys[q] : (uint32_t)q);
	int64_t s0 = 0, s1 = n_excl_shared;
	if (excl_off) { s0 = excl_off[q]; s1 = excl_off[q + 1]; }
	const uint32_t n_ex = (excl_ids && s1 > s0) ? (uint32_t)(s1 - s0) : 0u;   // distinct int32 ids: a segment is shorter than 2^31
	const int32_t *seg = excl_ids + s0;
	float tau = -INFINITY;
	uint64_t tau_key = 0;

	// one element per lane (wave-uniform call): noise, key, and -- for the keys that would be pushed -- the exclusion test
	auto offer = [&](bool in, float a, uint32_t id) {
		const float key = __fadd_rn(a, gumbel_noise(noise_row, id));
		const bool maybe = in && key >= tau;
		if (__ballot(maybe) == 0ull) return;
		bool hit = false;
		if (n_ex) {
			// lower bound without a lane-dependent branch (filter_topk_kernel): pos + half - 1 < n_ex throughout
			uint32_t pos = 0, len = n_ex;
			while (len > 1) {
				const uint32_t half = len >> 1;
				pos += (seg[pos + half - 1] < (int32_t)id) ? half : 0u;
				len -= half;
			}
			hit = seg[pos] == (int32_t)id;
		}
		const uint64_t ck = make_key(key, id);
		sel_push(maybe && !hit && ck > tau_key, ck, s.buf, &s.scal[0]);
	};

	const uintptr_t addr = reinterpret_cast<uintptr_t>(row);
	int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(float));
	if (head > I) head = I;
	const int64_t nvec = (I - head) / SMP_VEC;
	const int64_t tail0 = head + nvec * SMP_VEC;
	const f32x4 *vp = reinterpret_cast<const f32x4 *>(row + head);
	const int64_t vlast = nvec > 0 ? nvec - 1 : 0;
	{  // unaligned head and the tail: fewer than 2 * SMP_VEC elements in total
		int64_t i = -1;
		if (tid < head) i = tid;
		else if (tid - head < I - tail0) i = tail0 + (tid - head);
		const bool in = i >= 0;
		offer(in, in ? __fmul_rn(row[i], inv_T) : 0.f, (uint32_t)i);
	}
	if (nvec == 0) {   // (uniform) nothing to stream: a row of fewer than 2 * SMP_VEC elements
		sel_finish<KMAX>(s, k, out_key + q * (int64_t)k, out_idx + q * (int64_t)k);
		return;
	}
	f32x4 nxt[SMP_U];
#pragma unroll
	for (int u = 0; u < SMP_U; ++u) {
		const int64_t iv = (int64_t)u * SEL_THREADS + tid;
		nxt[u] = vp[iv < nvec ? iv : vlast];
	}
	for (int64_t vb = 0; vb < nvec; vb += SMP_STEP) {
		f32x4 cur[SMP_U];
#pragma unroll
		for (int u = 0; u < SMP_U; ++u) {
			cur[u] = nxt[u];
			const int64_t ivn = vb + SMP_STEP + (int64_t)u * SEL_THREADS + tid;
			nxt[u] = vp[ivn < nvec ? ivn : vlast];
		}
		sel_maybe_compact<KMAX>(s, k, tau, tau_key);   // (the check for the batch before: at most SEL_PASS pushes follow)
#pragma unroll
		for (int u = 0; u < SMP_U; ++u) {
			const int64_t iv = vb + (int64_t)u * SEL_THREADS + tid;
			const bool ok = iv < nvec;
			const uint32_t i0 = (uint32_t)(head + iv * SMP_VEC);
			float a[SMP_VEC];
#pragma unroll
			for (int e = 0; e < SMP_VEC; ++e) a[e] = __fmul_rn(cur[u][e], inv_T);
			// rounding is monotonic: key = rn(a + g) <= rn(a + GUMBEL_MAX); fmaxf drops NaN (a vector of NaN alone fails the compare)
			const float ub = __fadd_rn(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), GUMBEL_MAX);
			if (__ballot(ok && ub >= tau) == 0ull) continue;
#pragma unroll
			for (int e = 0; e < SMP_VEC; ++e) offer(ok, a[e], i0 + (uint32_t)e);
		}
	}
	sel_finish<KMAX>(s, k, out_key + q * (int64_t)k, out_idx + q * (int64_t)k);
}

// out[q, i] = g(q, i): the noise alone, for tests and for auditing a draw.  grid.x covers the items, grid.y strides over the rows.
__global__ __launch_bounds__(256) void gumbel_noise_kernel(uint64_t base, const int32_t *__restrict__ row_keys, int64_t Q, int64_t I,
															float *__restrict__ out, int64_t ldo) {
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= I) return;
	for (int64_t q = blockIdx.y; q < Q; q += gridDim.y)
		out[q * ldo + i] = gumbel_noise(gumbel_row(base, row_keys ? (uint32_t)row_keys[q] : (uint32_t)q), (uint32_t)i);
}

template <int KM>
int launch_sample_topk(const float *S, int64_t lds, int64_t Q, int64_t I, float inv_T, uint64_t base, const int32_t *row_keys, const int64_t *excl_off,
					   const int32_t *excl_ids, int64_t n_excl_shared, int32_t k, float *out_key, int32_t *out_idx, hipStream_t st) {
	const int rc = anncur_ensure_dyn_lds((const void *)sample_topk_kernel<KM>, (int)SelCfg<KM>::LDS_BYTES);
	if (rc != ANNCUR_OK) return rc;
	hipLaunchKernelGGL((sample_topk_kernel<KM>), dim3((unsigned)Q), dim3(SEL_THREADS), SelCfg<KM>::LDS_BYTES, st, S, lds, I, inv_T, base, row_keys, excl_off,
					   excl_ids, n_excl_shared, (uint32_t)k, out_key, out_idx);
	return ANNCUR_OK;
}

}  // namespace

extern "C" int anncur_sample_topk(const float *S, int64_t lds, int64_t Q, int64_t I, float inv_T, uint64_t seed, uint32_t stream_id, const int32_t *row_keys,
								   const int64_t *excl_off, const int32_t *excl_ids, int64_t n_excl_shared, int32_t k, float *out_key, int32_t *out_idx,
								   void *stream) {
	ANNCUR_REQUIRE(Q >= 0 && Q < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "sample_topk: need 0 <= Q < 2^31 (got %lld)", (long long)Q);
	ANNCUR_REQUIRE(I >= 1 && I < (int64_t)0x80000000ll, ANNCUR_E_INVALID, "sample_topk: need 1 <= I < 2^31 items (got %lld)", (long long)I);
	ANNCUR_REQUIRE(k >= 1 && k <= ANNCUR_MAX_TOPK && (int64_t)k <= I, ANNCUR_E_INVALID, "sample_topk: need 1 <= k <= min(I, ANNCUR_MAX_TOPK) = min(%lld, %d) (got %d)",
				   (long long)I, ANNCUR_MAX_TOPK, (int)k);
	ANNCUR_REQUIRE(inv_T > 0.f && inv_T < INFINITY, ANNCUR_E_INVALID, "sample_topk: inv_T = 1 / temperature must be finite and > 0 (got %g)", (double)inv_T);
	ANNCUR_REQUIRE(lds >= I, ANNCUR_E_INVALID, "sample_topk: the row pitch lds = %lld is shorter than the row of I = %lld", (long long)lds, (long long)I);
	ANNCUR_REQUIRE(excl_off || (n_excl_shared >= 0 && n_excl_shared < (int64_t)0x7fffffff), ANNCUR_E_INVALID,
				   "sample_topk: the shared list's length must be in [0, 2^31) (got %lld)", (long long)n_excl_shared);
	ANNCUR_REQUIRE(excl_off || excl_ids || n_excl_shared == 0, ANNCUR_E_INVALID, "sample_topk: excl_ids is NULL but the shared list is not empty");
	ANNCUR_REQUIRE(S && out_key && out_idx, ANNCUR_E_INVALID, "sample_topk: null pointer");
	if (Q == 0) return ANNCUR_OK;
	hipStream_t st = (hipStream_t)stream;
	const uint64_t base = gumbel_base(seed, stream_id);
	int rc;
	if (k <= 128) rc = launch_sample_topk<128>(S, lds, Q, I, inv_T, base, row_keys, excl_off, excl_ids, n_excl_shared, k, out_key, out_idx, st);   // as pool.hip
	else if (k <= 512) rc = launch_sample_topk<512>(S, lds, Q, I, inv_T, base, row_keys, excl_off, excl_ids, n_excl_shared, k, out_key, out_idx, st);
	else rc = launch_sample_topk<2048>(S, lds, Q, I, inv_T, base, row_keys, excl_off, excl_ids, n_excl_shared, k, out_key, out_idx, st);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_gumbel_noise(uint64_t seed, uint32_t stream_id, const int32_t *row_keys, int64_t Q, int64_t I, float *out, int64_t ldo, void *stream) {
	ANNCUR_REQUIRE(Q >= 0 && I >= 1 && I <= (int64_t)0x80000000ll, ANNCUR_E_INVALID, "gumbel_noise: need Q >= 0 and 1 <= I <= 2^31 item ids (got %lld, %lld)",
				   (long long)Q, (long long)I);
	ANNCUR_REQUIRE(ldo >= I, ANNCUR_E_INVALID, "gumbel_noise: the row pitch ldo = %lld is shorter than the row of I = %lld", (long long)ldo, (long long)I);
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(out, ANNCUR_E_INVALID, "gumbel_noise: null pointer");
	hipLaunchKernelGGL(gumbel_noise_kernel, dim3((unsigned)ceil_div64(I, 256), (unsigned)(Q < 65535 ? Q : 65535)), dim3(256), 0, (hipStream_t)stream,
					   gumbel_base(seed, stream_id), row_keys, Q, I, out, ldo);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
