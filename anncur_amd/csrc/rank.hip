// Ranks of given items: where does item `id` stand in a score row sorted by (score descending, id ascending)?
//
//   rank = #{ i != id : s[i] > a  or  (s[i] == a and i < id) },  a = s[id]        (the contract: include/anncur_hip.h)
//
// Both entry points count with ONE order, the 64-bit key (sortable score bits, ~id) -- larger key = further ahead; -0.0 is folded
// onto +0.0 first and a NaN score never gets a key.  A row's t targets are sorted by key (descending) once; an element that beats the
// weakest target is placed by a binary search among them and counted in the bin of the first target it beats; a prefix sum over the
// bins is every target's rank at once; the result goes back in the caller's target order.
//
//   anncur_rank_in_rows   S is in memory (the exact matrix, or a row chunk of a materialised S_hat): one workgroup per row, target
//                         keys, bins and prefix sums in LDS, the row streamed with 16-byte loads.  A target's score is read from the row.
//   anncur_score_rank     S_hat = X . Et^T tile by tile on v_mfma_f32_32x32x16_bf16 (items = A operand, queries = B operand, so the
//                         query sits on the lane and its weakest key is one lane-local 64-bit value); S_hat is never written.
//                         Four launches: collect (the targets' scores), sort (keys per query, bins zeroed), count (all tiles), finish.
//
// Self-consistency of the fused route: the collect pass runs the SAME tile routine (tile_scores: one 16-byte fragment of the item row
// and one of the query row per k step, k ascending, one accumulator) on the gathered target rows -- query c's target in tile row c, its
// score on the diagonal -- so a target's score has the bits the count pass computes for that (query, item) pair: an MFMA output
// element depends on its A row, its B column and the k order alone, not on where the row sits in the tile
// (tests/test_gpu_rank_items.py G3 holds it to that).
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int RK_THREADS = 256;
constexpr int RK_MAX_T = ANNCUR_RANK_MAX_T;
constexpr uint64_t KEY_NONE = ~0ull;   // a hole or a NaN target: sorts in front of every real key, so nothing is ever counted against it
constexpr int RK_TILE = 32;            // items per MFMA tile
constexpr int RK_BQ = 128;             // queries per workgroup of the fused kernels: 4 waves x 32

// (score descending, id ascending) as one unsigned compare.  v is not NaN.  No real key is 0 or KEY_NONE: the sortable words
// 0 and 0xffffffff belong to NaN bit patterns.
__device__ __forceinline__ uint64_t rank_key(float v, uint32_t id) {
	uint32_t u = __float_as_uint(v);
	if (v == 0.0f) u = 0u;   // -0.0 ties with +0.0
	const uint32_t s = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
	return ((uint64_t)s << 32) | (uint64_t)(0xffffffffu - id);
}

// keys[0..P) (P a power of two) descending, by the whole workgroup; ends on a barrier
__device__ void sort_desc(uint64_t *keys, int P) {
	for (int k = 2; k <= P; k <<= 1)
		for (int j = k >> 1; j > 0; j >>= 1) {
			__syncthreads();
			for (int i = threadIdx.x; i < P; i += RK_THREADS) {
				const int l = i ^ j;
				if (l > i) {
					const uint64_t a = keys[i], b = keys[l];
					const bool desc = (i & k) == 0;
					if (desc ? (a < b) : (a > b)) {
						keys[i] = b;
						keys[l] = a;
					}
				}
			}
		}
	__syncthreads();
}

// in a descending list: how many keys are >= key (= the first target that `key` beats), how many are > key
template <typename P>
__device__ __forceinline__ int count_ge(P keys, int t, uint64_t key) {
	int lo = 0, hi = t;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (keys[mid] >= key) lo = mid + 1; else hi = mid;
	}
	return lo;
}
template <typename P>
__device__ __forceinline__ int count_gt(P keys, int t, uint64_t key) {
	int lo = 0, hi = t;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (keys[mid] > key) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// h[0..n) (LDS, n <= RK_MAX_T) -> inclusive prefix sums, by wave 0; a barrier on either side
__device__ void prefix_incl(uint32_t *h, int n) {
	__syncthreads();
	if (threadIdx.x < WAVE) {
		const int per = (n + WAVE - 1) / WAVE, b = (int)threadIdx.x * per;
		uint32_t s = 0;
		for (int i = 0; i < per; ++i)
			if (b + i < n) s += h[b + i];
		uint32_t run = wave_scan_incl<DppAdd>(s) - s;
		for (int i = 0; i < per; ++i)
			if (b + i < n) {
				run += h[b + i];
				h[b + i] = run;
			}
	}
	__syncthreads();
}

__device__ __forceinline__ int pow2_at_least(int t) {
	int p = 1;
	while (p < t) p <<= 1;
	return p;
}

// ------------------------------------------------------------------ ranks in rows that are in memory
template <typename T> struct RowVec;
template <> struct RowVec<float> {
	static constexpr int N = 4;
	__device__ static __forceinline__ float get(const u32x4 &w, int e) { return __uint_as_float(w[e]); }
};
template <> struct RowVec<uint16_t> {
	static constexpr int N = 8;
	__device__ static __forceinline__ float get(const u32x4 &w, int e) { return bf16_bits_to_f32((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu)); }
};

template <typename T>
__global__ __launch_bounds__(RK_THREADS) void rank_rows_kernel(const T *__restrict__ S, int64_t lds_, int64_t I, const int32_t *__restrict__ ids, int t,
																int32_t *__restrict__ rank, float *__restrict__ score) {
	__shared__ uint64_t sorted[RK_MAX_T];
	__shared__ uint64_t orig[RK_MAX_T];
	__shared__ uint32_t hist[RK_MAX_T];
	const int64_t q = blockIdx.x;
	const T *row = S + q * lds_;
	const int P = pow2_at_least(t);
	for (int j = threadIdx.x; j < P; j += RK_THREADS) {
		uint64_t key = 0;   // padding up to the power of two: behind every real key
		if (j < t) {
			const int32_t id = ids[q * t + j];
			float v = __uint_as_float(0x7fc00000u);
			key = KEY_NONE;
			if (id >= 0 && id < I) {   // anything else is a hole: no read
				v = load_as_f32<T>(row + id);
				if (v == v) key = rank_key(v, (uint32_t)id);
			}
			orig[j] = key;
			hist[j] = 0;
			if (score) score[q * t + j] = v;
		}
		sorted[j] = key;
	}
	sort_desc(sorted, P);
	const uint64_t weakest = sorted[t - 1];   // KEY_NONE when no target is valid: nothing passes

	auto visit = [&](float v, int64_t i) {
		if (v == v) {
			const uint64_t key = rank_key(v, (uint32_t)i);
			if (key > weakest) atomicAdd(&hist[count_ge(sorted, t, key)], 1u);   // the bin is < t: sorted[t - 1] < key
		}
	};
	constexpr int N = RowVec<T>::N;
	int64_t head = (int64_t)(((16 - ((uintptr_t)row & 15)) & 15) / sizeof(T));   // elements in front of the first 16-byte boundary
	if (head > I) head = I;
	const int64_t nvec = (I - head) / N;
	for (int64_t i = threadIdx.x; i < head; i += RK_THREADS) visit(load_as_f32<T>(row + i), i);
	const u32x4 *vp = reinterpret_cast<const u32x4 *>(row + head);
	for (int64_t v = threadIdx.x; v < nvec; v += RK_THREADS) {
		const u32x4 w = vp[v];
#pragma unroll
		for (int e = 0; e < N; ++e) visit(RowVec<T>::get(w, e), head + v * N + e);
	}
	for (int64_t i = head + nvec * N + threadIdx.x; i < I; i += RK_THREADS) visit(load_as_f32<T>(row + i), i);

	prefix_incl(hist, t);
	for (int j = threadIdx.x; j < t; j += RK_THREADS) {
		const uint64_t key = orig[j];
		// equal keys (a duplicated id) share a rank: the bins between them are empty, so the first position serves all
		rank[q * t + j] = key == KEY_NONE ? -1 : (int32_t)hist[count_gt(sorted, t, key)];
	}
}

// ------------------------------------------------------------------ ranks under S_hat = X . Et^T, S_hat never written
// the lane's B fragments: query row (lane & 31), k = 16 s + 8 (lane >> 5) + 0..7 -- resident for the whole kernel
template <int KP>
__device__ __forceinline__ void load_query(const uint16_t *__restrict__ X, int64_t ldx, int64_t Q, int64_t q, int h, bf16x8 (&xb)[KP / 16]) {
	const int64_t qc = q < Q ? q : Q - 1;   // a lane past Q reads a real row and never counts
	const u32x4 *p = reinterpret_cast<const u32x4 *>(X + qc * ldx + 8 * h);
#pragma unroll
	for (int s = 0; s < KP / 16; ++s) xb[s] = __builtin_bit_cast(bf16x8, p[2 * s]);
}

// THE tile routine of both passes: arow = the lane's item row (tile row lane & 31) + 8 (lane >> 5).  acc[r] of lane l is
// S_hat[query l & 31][tile row (r & 3) + 8 (r >> 2) + 4 (l >> 5)].
template <int KP>
__device__ __forceinline__ f32x16 tile_scores(const uint16_t *__restrict__ arow, const bf16x8 (&xb)[KP / 16]) {
	const u32x4 *p = reinterpret_cast<const u32x4 *>(arow);
	f32x16 acc;
#pragma unroll
	for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
	for (int s = 0; s < KP / 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, p[2 * s]), xb[s], acc, 0, 0, 0);
	return acc;
}

template <int KP>
__global__ __launch_bounds__(RK_THREADS) void rank_collect_kernel(const uint16_t *__restrict__ X, int64_t ldx, const uint16_t *__restrict__ Et, int64_t Q, int64_t I,
																   const int32_t *__restrict__ ids, int t, float *__restrict__ tscore) {
	const int lane = lane_id(), c = lane & 31, h = lane >> 5;
	const int64_t q0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
	if (q0 >= Q) return;   // wave-uniform
	const int64_t q = q0 + c;
	bf16x8 xb[KP / 16];
	load_query<KP>(X, ldx, Q, q, h, xb);
	// tile row c holds query c's own target: its score is the diagonal element, in lane half (c >> 2) & 1, register (c & 3) + 4 (c >> 3)
	const bool mine = h == ((c >> 2) & 1) && q < Q;
	const int reg = (c & 3) + 4 * (c >> 3);
	for (int j = blockIdx.y; j < t; j += gridDim.y) {
		const int32_t id = q < Q ? ids[q * t + j] : -1;
		const bool ok = id >= 0 && id < I;
		const f32x16 acc = tile_scores<KP>(Et + (int64_t)(ok ? id : 0) * KP + 8 * h, xb);
		float v = acc[0];
#pragma unroll
		for (int r = 1; r < 16; ++r) v = reg == r ? acc[r] : v;
		if (mine) tscore[q * t + j] = ok ? v : __uint_as_float(0x7fc00000u);
	}
}

__device__ __forceinline__ uint64_t target_key(int32_t id, float v, int64_t I) { return (id >= 0 && id < I && v == v) ? rank_key(v, (uint32_t)id) : KEY_NONE; }

// one workgroup per query: its target keys, descending, and its bins zeroed (the caller pre-fills nothing)
__global__ __launch_bounds__(RK_THREADS) void rank_sort_kernel(const int32_t *__restrict__ ids, const float *__restrict__ tscore, int64_t I, int t,
																uint64_t *__restrict__ sorted, uint32_t *__restrict__ hist) {
	__shared__ uint64_t keys[RK_MAX_T];
	const int64_t q = blockIdx.x;
	const int P = pow2_at_least(t);
	for (int j = threadIdx.x; j < P; j += RK_THREADS) keys[j] = j < t ? target_key(ids[q * t + j], tscore[q * t + j], I) : 0ull;
	sort_desc(keys, P);
	for (int j = threadIdx.x; j < t; j += RK_THREADS) {
		sorted[q * t + j] = keys[j];
		hist[q * t + j] = 0u;
	}
}

template <int KP>
__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(const uint16_t *__restrict__ X, int64_t ldx, const uint16_t *__restrict__ Et, int64_t Q, int64_t I, int t,
																 const uint64_t *__restrict__ sorted, uint32_t *__restrict__ hist, int64_t ntiles, int64_t tiles_per_split) {
	const int lane = lane_id(), c = lane & 31, h = lane >> 5;
	const int64_t q0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
	if (q0 >= Q) return;   // wave-uniform
	const int64_t q = q0 + c;
	bf16x8 xb[KP / 16];
	load_query<KP>(X, ldx, Q, q, h, xb);
	const bool live = q < Q;
	const uint64_t *sq = sorted + (live ? q : 0) * t;
	uint32_t *hq = hist + (live ? q : 0) * t;
	const uint64_t weakest = live ? sq[t - 1] : KEY_NONE;   // a lane past Q passes nothing: it neither counts nor stores
	const int64_t t0 = (int64_t)blockIdx.y * tiles_per_split;
	const int64_t t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
	for (int64_t tile = t0; tile < t1; ++tile) {
		const f32x16 acc = tile_scores<KP>(Et + (tile * RK_TILE + c) * KP + 8 * h, xb);
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int64_t item = tile * RK_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
			const float v = acc[r];
			if (item < I && v == v) {   // rows I .. ceil32(I) - 1 are padding: a 0 there would be ahead of every negative target
				const uint64_t key = rank_key(v, (uint32_t)item);
				if (key > weakest) atomicAdd(&hq[count_ge(sq, t, key)], 1u);   // the bin is < t: sq[t - 1] < key
			}
		}
	}
}

__global__ __launch_bounds__(RK_THREADS) void rank_finish_kernel(const int32_t *__restrict__ ids, const float *__restrict__ tscore, int64_t I, int t,
																  const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ hist, int32_t *__restrict__ rank,
																  float *__restrict__ score) {
	__shared__ uint64_t keys[RK_MAX_T];
	__shared__ uint32_t h[RK_MAX_T];
	const int64_t q = blockIdx.x;
	for (int j = threadIdx.x; j < t; j += RK_THREADS) {
		keys[j] = sorted[q * t + j];
		h[j] = hist[q * t + j];
	}
	prefix_incl(h, t);
	for (int j = threadIdx.x; j < t; j += RK_THREADS) {
		const float v = tscore[q * t + j];
		const uint64_t key = target_key(ids[q * t + j], v, I);
		rank[q * t + j] = key == KEY_NONE ? -1 : (int32_t)h[count_gt(keys, t, key)];
		if (score) score[q * t + j] = v;
	}
}

bool rank_kp_ok(int64_t Kp) { return Kp == 64 || Kp == 128 || Kp == 256 || Kp == 512; }
constexpr int64_t RK_MAX_ROWS = 0x7fffffff;   // grid.x of the one-workgroup-per-row kernels

struct RankWs {
	size_t sorted_off, tscore_off, hist_off, total;
};
RankWs rank_ws(int64_t Q, int32_t t) {
	RankWs w;
	const size_t n = (size_t)Q * (size_t)t;
	w.sorted_off = 0;
	w.tscore_off = n * 8;
	w.hist_off = n * 12;
	w.total = (n * 16 + 255) / 256 * 256;
	return w;
}

template <int KP>
int launch_score_rank(const uint16_t *X, int64_t ldx, const uint16_t *Et, int64_t Q, int64_t I, const int32_t *ids, int32_t t, int32_t *rank, float *score, char *ws,
					  hipStream_t st) {
	const RankWs w = rank_ws(Q, t);
	uint64_t *sorted = reinterpret_cast<uint64_t *>(ws + w.sorted_off);
	float *tscore = reinterpret_cast<float *>(ws + w.tscore_off);
	uint32_t *hist = reinterpret_cast<uint32_t *>(ws + w.hist_off);
	const int64_t qblocks = ceil_div64(Q, RK_BQ), ntiles = ceil_div64(I, RK_TILE);
	rank_collect_kernel<KP><<<dim3((unsigned)qblocks, (unsigned)(t < 64 ? t : 64)), RK_THREADS, 0, st>>>(X, ldx, Et, Q, I, ids, t, tscore);
	ANNCUR_LAUNCH_OK();
	rank_sort_kernel<<<dim3((unsigned)Q), RK_THREADS, 0, st>>>(ids, tscore, I, t, sorted, hist);
	ANNCUR_LAUNCH_OK();
	// item splits: enough workgroups to fill the chip when the query blocks alone do not; their counts meet by integer atomics
	int64_t splits = ceil_div64(8 * (int64_t)anncur_num_cu(), qblocks);
	if (splits > ntiles) splits = ntiles;
	if (splits > 65535) splits = 65535;
	if (splits < 1) splits = 1;
	const int64_t per = ceil_div64(ntiles, splits);
	splits = ceil_div64(ntiles, per);
	rank_count_kernel<KP><<<dim3((unsigned)qblocks, (unsigned)splits), RK_THREADS, 0, st>>>(X, ldx, Et, Q, I, t, sorted, hist, ntiles, per);
	ANNCUR_LAUNCH_OK();
	rank_finish_kernel<<<dim3((unsigned)Q), RK_THREADS, 0, st>>>(ids, tscore, I, t, sorted, hist, rank, score);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

}  // namespace

extern "C" int anncur_rank_in_rows(const void *S, int dtype, int64_t Q, int64_t I, int64_t lds_, const int32_t *ids, int32_t t, int32_t *rank, float *score,
								   void *stream) {
	ANNCUR_REQUIRE(dtype_ok(dtype), ANNCUR_E_INVALID, "rank_in_rows: bad dtype");
	ANNCUR_REQUIRE(Q >= 0 && Q <= RK_MAX_ROWS && I >= 1 && I < (int64_t)0x7fffffff && lds_ >= I, ANNCUR_E_INVALID, "rank_in_rows: bad shape (Q=%lld I=%lld pitch=%lld)",
				   (long long)Q, (long long)I, (long long)lds_);
	ANNCUR_REQUIRE(t >= 1 && t <= RK_MAX_T, ANNCUR_E_INVALID, "rank_in_rows: t = %d outside 1..%d", t, RK_MAX_T);
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(S && ids && rank, ANNCUR_E_INVALID, "rank_in_rows: null pointer");
	hipStream_t st = (hipStream_t)stream;
	if (dtype == ANNCUR_F32)
		rank_rows_kernel<float><<<dim3((unsigned)Q), RK_THREADS, 0, st>>>((const float *)S, lds_, I, ids, t, rank, score);
	else
		rank_rows_kernel<uint16_t><<<dim3((unsigned)Q), RK_THREADS, 0, st>>>((const uint16_t *)S, lds_, I, ids, t, rank, score);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" size_t anncur_score_rank_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t t) {
	if (!rank_kp_ok(Kp) || Q < 1 || Q > RK_MAX_ROWS || I < 1 || I >= (int64_t)0x7fffffff - 64 || t < 1 || t > RK_MAX_T) return 0;
	return rank_ws(Q, t).total;
}

extern "C" int anncur_score_rank(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, const int32_t *ids, int32_t t,
								 int32_t *rank, float *score, void *workspace, size_t workspace_bytes, void *stream) {
	ANNCUR_REQUIRE(rank_kp_ok(Kp), ANNCUR_E_UNSUPPORTED, "score_rank: Kp must be 64, 128, 256 or 512 (got %d): use anncur_rank_in_rows on a dense S_hat", Kp);
	ANNCUR_REQUIRE(Q >= 0 && Q <= RK_MAX_ROWS && I >= 1 && I < (int64_t)0x7fffffff - 64, ANNCUR_E_INVALID, "score_rank: bad shape (Q=%lld I=%lld)", (long long)Q, (long long)I);
	ANNCUR_REQUIRE(t >= 1 && t <= RK_MAX_T, ANNCUR_E_INVALID, "score_rank: t = %d outside 1..%d", t, RK_MAX_T);
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(X && Et && ids && rank, ANNCUR_E_INVALID, "score_rank: null pointer");
	ANNCUR_REQUIRE(lde == Kp && ldx >= Kp && ldx % 8 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Et & 15) == 0, ANNCUR_E_INVALID,
				   "score_rank: X / Et must be packed bf16 (lde == Kp, ldx a multiple of 8, 16-byte aligned)");
	const size_t need = anncur_score_rank_workspace_bytes(Q, I, Kp, t);
	ANNCUR_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= need, ANNCUR_E_WORKSPACE,
				   "score_rank: workspace missing, misaligned or too small (need %zu bytes, 256-byte aligned)", need);
	const uint16_t *x = (const uint16_t *)X, *e = (const uint16_t *)Et;
	hipStream_t st = (hipStream_t)stream;
	switch (Kp) {
	case 64: return launch_score_rank<64>(x, ldx, e, Q, I, ids, t, rank, score, (char *)workspace, st);
	case 128: return launch_score_rank<128>(x, ldx, e, Q, I, ids, t, rank, score, (char *)workspace, st);
	case 256: return launch_score_rank<256>(x, ldx, e, Q, I, ids, t, rank, score, (char *)workspace, st);
	default: return launch_score_rank<512>(x, ldx, e, Q, I, ids, t, rank, score, (char *)workspace, st);
	}
}
