// Filtered retrieval: the one kernel behind every top-k's `exclude=` argument.
//
// If query q excludes e_q distinct items, the unfiltered top-(k + e_q) contains the filtered top-k, so the caller asks its usual top-k
// for k + max_q e_q candidates and this kernel compacts each row: it drops the excluded ids and the holes (id < 0), keeps the order the
// producer wrote -- descending -- and pads with (-inf, -1).  No producer kernel, plan or workspace knows about it.
#include "common.hpp"

namespace {

constexpr int FT_WAVES = 4;   // queries per workgroup: one wave each, no LDS, no barrier

// One wave per query.  The row is walked in chunks of 64 candidates, lane = candidate: every lane binary-searches its id in the query's
// ascending exclusion segment (a fixed number of steps for the whole wave: the segment length is wave-uniform), one ballot gives the
// chunk's survivors and a lane's output slot is the running count plus the survivors in the lanes below it.  Lanes past the row's end
// take part with a hole, so the ballot always sees the whole wave.  The walk ends as soon as k_out survivors are out.
__global__ __launch_bounds__(FT_WAVES * WAVE) void filter_topk_kernel(const float *__restrict__ in_val, const int32_t *__restrict__ in_idx, int64_t ld_in,
																	   int n_cand, int64_t Q, const int64_t *__restrict__ excl_off,
																	   const int32_t *__restrict__ excl_ids, int64_t n_excl_shared, int k_out,
																	   float *__restrict__ out_val, int32_t *__restrict__ out_idx) {
	const int lane = lane_id();
	const int64_t q = (int64_t)blockIdx.x * FT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
	if (q >= Q) return;   // (the whole wave: the last workgroup is ragged)
	int64_t s0 = 0, s1 = n_excl_shared;
	if (excl_off) { s0 = excl_off[q]; s1 = excl_off[q + 1]; }
	const uint32_t n = (excl_ids && s1 > s0) ? (uint32_t)(s1 - s0) : 0u;   // distinct int32 ids: a segment is shorter than 2^31
	const int32_t *seg = excl_ids + s0;
	const float *rv = in_val + q * ld_in;
	const int32_t *ri = in_idx + q * ld_in;
	float *ov = out_val + q * (int64_t)k_out;
	int32_t *oi = out_idx + q * (int64_t)k_out;
	int base = 0;   // survivors written so far (wave-uniform: it only grows by ballot counts)
	for (int j0 = 0; j0 < n_cand && base < k_out; j0 += WAVE) {
		const int j = j0 + lane;
		int32_t id = -1;
		float v = 0.f;
		if (j < n_cand) { id = ri[j]; v = rv[j]; }
		bool hit = false;
		if (n) {
			// lower bound without a lane-dependent branch: the id, if present, stays inside [pos, pos + len); pos + half - 1 < n throughout
			uint32_t pos = 0, len = n;
			while (len > 1) {
				const uint32_t half = len >> 1;
				pos += (seg[pos + half - 1] < id) ? half : 0u;
				len -= half;
			}
			hit = seg[pos] == id;
		}
		const bool keep = id >= 0 && !hit;
		const unsigned long long mask = __ballot(keep);
		const int p = base + __popcll(mask & ((1ull << lane) - 1ull));
		if (keep && p < k_out) { ov[p] = v; oi[p] = id; }
		base += __popcll(mask);
	}
	for (int p = (base < k_out ? base : k_out) + lane; p < k_out; p += WAVE) { ov[p] = -INFINITY; oi[p] = -1; }
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int anncur_filter_topk(const float *in_val, const int32_t *in_idx, int64_t ld_in, int64_t n_cand, int64_t Q, const int64_t *excl_off,
								   const int32_t *excl_ids, int64_t n_excl_shared, int32_t k_out, float *out_val, int32_t *out_idx, void *stream) {
	ANNCUR_REQUIRE(Q >= 1 && Q < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "filter_topk: need 1 <= Q < 2^31 (got %lld)", (long long)Q);
	ANNCUR_REQUIRE(n_cand >= 1 && n_cand <= ANNCUR_MAX_TOPK && k_out >= 1 && k_out <= n_cand, ANNCUR_E_INVALID,
				   "filter_topk: need 1 <= k_out <= n_cand <= %d (got %d, %lld)", ANNCUR_MAX_TOPK, (int)k_out, (long long)n_cand);
	ANNCUR_REQUIRE(ld_in >= n_cand, ANNCUR_E_INVALID, "filter_topk: ld_in < n_cand");
	ANNCUR_REQUIRE(in_val && in_idx && out_val && out_idx, ANNCUR_E_INVALID, "filter_topk: null pointer");
	ANNCUR_REQUIRE(excl_off || (n_excl_shared >= 0 && n_excl_shared < (int64_t)0x7fffffff), ANNCUR_E_INVALID,
				   "filter_topk: the shared list's length must be in [0, 2^31) (got %lld)", (long long)n_excl_shared);
	ANNCUR_REQUIRE(excl_off || excl_ids || n_excl_shared == 0, ANNCUR_E_INVALID, "filter_topk: excl_ids is NULL but the shared list is not empty");
	const size_t in_elems = (size_t)((Q - 1) * ld_in + n_cand), out_elems = (size_t)(Q * (int64_t)k_out);
	ANNCUR_REQUIRE(!overlaps(out_val, 4 * out_elems, in_val, 4 * in_elems) && !overlaps(out_val, 4 * out_elems, in_idx, 4 * in_elems) &&
					   !overlaps(out_idx, 4 * out_elems, in_val, 4 * in_elems) && !overlaps(out_idx, 4 * out_elems, in_idx, 4 * in_elems) &&
					   !overlaps(out_val, 4 * out_elems, out_idx, 4 * out_elems),
				   ANNCUR_E_INVALID, "filter_topk: the outputs must not alias the inputs or each other");
	hipLaunchKernelGGL(filter_topk_kernel, dim3((unsigned)ceil_div64(Q, FT_WAVES)), dim3(FT_WAVES * WAVE), 0, (hipStream_t)stream, in_val, in_idx, ld_in,
					   (int)n_cand, Q, excl_off, excl_ids, n_excl_shared, (int)k_out, out_val, out_idx);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
