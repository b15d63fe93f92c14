// Small-batch search: S = X . E^T for 1..64 queries streamed once over the item matrix, then a group-sparse top-k.
//   CURApprox.get_complete_row + topk_in_row   eval/matrix_approx_zeshel.py:121-126
//   faiss IndexFlatIP.search                   models/nearest_nbr.py:36-38
//
// Two launches, no memset.
//
// few_score_kernel (HBM-bound: the call costs one read of Et).  v_mfma_f32_16x16x32_bf16 with the ITEMS as the A operand and the queries as
// B, as score16_kernel: lane l holds item row l & 15, k = 32 s + 8 (l >> 4) + j of k-step s, and D[item 4 (l >> 4) + r][query l & 15].  A wave
// owns whole 64-item groups (four 16-item tiles each) and reads a tile's A fragments straight from global memory in fragment layout: one
// 16-byte load per lane and k-step, 16 rows x 64 contiguous bytes per wave and load, so the tile's 32 Kp bytes are read exactly once and never
// pass through LDS.  All loads of a tile are issued before its first MFMA, and the next tile's are issued before the current tile's MFMAs
// (two register buffers; the compiler counts vmcnt).  The queries are staged once per workgroup in LDS, rows q >= Q as zeros (X rows >= Q are
// never read); a B fragment is one ds_read_b128, and one A fragment feeds all ceil(Q / 16) query sub-tiles.  k-steps ascend into ONE
// accumulator per (tile, sub-tile) from zero: the k order of score16_kernel, so a score equals the fused route's bit for bit at Kp <= 256.
// Kp > 512 (the wide operands) runs the same loop over 128-element pieces of a tile's rows, still ascending into the one accumulator.
// Addressing: the tile base (tile x 32 Kp bytes) and q x pitch are formed in 64 bits, offsets inside a tile in 32.
// Outputs, for q < Q and i < I only: S[q][i] (a lane holds four consecutive items of one query: one 16-byte store) and one maximum per 64
// consecutive items, GM[q][g], an fmaxf chain from NaN (a NaN is skipped, an all-NaN group stays NaN).  Et's pad rows reach neither.
//
// few_select_kernel (one workgroup per query, the selector of select.hpp):
//  (a) tau = the k-th largest non-NaN group maximum (-inf with fewer than k);
//  (b) GM[q] is walked in rounds of FEW_ROUND groups; only the groups with maximum >= tau are read (256 contiguous bytes each) and every
//      v >= tau goes into the candidate buffer.  Any item >= tau lies in such a group, and k groups hold one: the buffer holds the true top-k;
//  (c) select + sort (score descending, smaller id on ties, NaN never, -inf ordinary, (-inf, -1) pads);
//  (d) more than cand_cap candidates at the end of a round (heavy ties, or no threshold on a long row): the walk stops and the workgroup
//      scans the whole row with the streaming selector, which is exact; fallback = 1.
#include "select.hpp"

using namespace anncur;

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int FEW_QMAX = 64;                  // queries per call
constexpr int FEW_WAVES = 4;                  // waves per workgroup of the score kernel
constexpr int FEW_MAX_WAVES = 2048;           // waves of a launch: eight per CU on 256 CUs (a host constant: the plan needs no device)
constexpr int FEW_GROUP = 64;                 // items per group maximum = four tiles
constexpr int FEW_TILE = 16;
constexpr int FEW_STAGE_BYTES = 64 * 1024;    // the staged queries: 16 ceil(Q / 16) x Kp x 2 bytes at most (ANNCUR_FEW_STAGE_BYTES)
constexpr int FEW_ROW_PAD = 32;               // bytes between staged rows: the sixteen rows of a ds_read_b128 lane group fall on distinct banks (Kp >= 128)
constexpr int FEW_HEADER_BYTES = 1024;        // [64 queries][groups_read, n_cand, fallback, 0]
constexpr int FEW_ROUND = 1024;               // group maxima walked between two barriers of the select
constexpr int FEW_READ_UNROLL = 8;            // groups a wave has in flight while collecting
static_assert(FEW_STAGE_BYTES == ANNCUR_FEW_STAGE_BYTES && FEW_QMAX == ANNCUR_FEW_MAX_Q, "include/anncur_hip.h states both");
static_assert(FEW_QMAX * 4 * 4 == FEW_HEADER_BYTES && FEW_HEADER_BYTES / 4 == FEW_WAVES * 64, "workgroup 0 zeroes the header, one word per thread");

struct FewPlan {
	bool ok;
	int64_t tiles, groups, pitch, ldg;
	int workgroups, gpw, tiles_min, tiles_max, nsub, kmax, cand_cap;
	size_t gm_off, s_off, total;
};

bool few_kp_ok(int32_t Kp) { return Kp == 64 || Kp == 128 || Kp == 256 || Kp == 512 || (Kp > 512 && Kp <= 4096 && Kp % 128 == 0); }
int few_kmax_class(int k) { return k <= 128 ? 128 : (k <= 512 ? 512 : 2048); }   // as kmax_class of topk.hip

// shape -> launch geometry and workspace layout (host only)
FewPlan few_plan_of(int64_t Q, int64_t I, int32_t Kp) {
	FewPlan P{};
	if (Q < 1 || Q > FEW_QMAX || !few_kp_ok(Kp) || I < 1 || I >= (int64_t)0x7fffffff) return P;
	P.nsub = (int)((Q + 15) / 16);
	if ((int64_t)16 * P.nsub * Kp * 2 > FEW_STAGE_BYTES) return P;
	P.ok = true;
	P.tiles = ceil_div64(I, FEW_TILE);
	P.groups = ceil_div64(I, FEW_GROUP);
	P.pitch = ceil_div64(I, 32) * 32;
	P.ldg = ceil_div64(P.groups, 64) * 64;
	P.gpw = (int)ceil_div64(P.groups, FEW_MAX_WAVES);
	P.workgroups = (int)ceil_div64(P.groups, (int64_t)P.gpw * FEW_WAVES);
	const int64_t lead_groups = (ceil_div64(P.groups, P.gpw) - 1) * P.gpw;   // groups of the waves before the last one that has any
	P.tiles_max = (int)(P.tiles < 4 * (int64_t)P.gpw ? P.tiles : 4 * (int64_t)P.gpw);
	P.tiles_min = (int)(P.tiles - lead_groups * 4);
	P.gm_off = FEW_HEADER_BYTES;
	P.s_off = P.gm_off + (((size_t)Q * (size_t)P.ldg * 4 + 255) & ~(size_t)255);
	P.total = P.s_off + (size_t)Q * (size_t)P.pitch * 4;
	return P;
}
FewPlan few_plan_of(int64_t Q, int64_t I, int32_t Kp, int32_t k) {
	FewPlan P = few_plan_of(Q, I, Kp);
	if (k < 1 || k > ANNCUR_MAX_TOPK || (int64_t)k > I) P.ok = false;
	if (!P.ok) return P;
	P.kmax = few_kmax_class(k);
	P.cand_cap = SEL_PASS + 2 * P.kmax;
	return P;
}

// ------------------------------------------------------------------ launch 1
struct FewScoreArgs {
	const uint16_t *X;
	int64_t ldx;
	const unsigned char *Et;
	int32_t Q, Kp, gpw, nsub;
	uint32_t I, n_tiles, n_groups;
	float *S;
	int64_t lds;
	float *GM;
	int64_t ldg;
	uint32_t *hdr;
};

template <int STEPS>
__device__ __forceinline__ void few_issue(u32x4 (&a)[STEPS], const unsigned char *p) {
#pragma unroll
	for (int s = 0; s < STEPS; ++s) a[s] = *reinterpret_cast<const u32x4 *>(p + 64 * s);
}

// Tile t is complete in acc: its scores and its share of the group maximum; the accumulators start the next tile from zero.  After the
// group's last tile (or the wave's last) the maximum goes out: the four lanes that share a query hold four items each.
__device__ __forceinline__ void few_tile_done(const FewScoreArgs &p, uint32_t t, uint32_t t_hi, int c16, int g4, f32x4 (&acc)[4], float (&gmx)[4]) {
	const uint32_t item0 = t * FEW_TILE + 4u * (uint32_t)g4;
	const bool full = t * FEW_TILE + FEW_TILE <= p.I;   // (uniform)
	const bool last = (t & 3u) == 3u || t + 1u == t_hi; // (uniform)
#pragma unroll
	for (int st = 0; st < 4; ++st) {
		if (st < p.nsub) {
			const int q = 16 * st + c16;
			const f32x4 v = acc[st];
			acc[st] = (f32x4){0.f, 0.f, 0.f, 0.f};
			float *dst = p.S + (int64_t)q * p.lds + item0;
			if (full || item0 + 3u < p.I) {
				if (q < p.Q) *reinterpret_cast<f32x4 *>(dst) = v;
				gmx[st] = fmaxf(fmaxf(fmaxf(fmaxf(gmx[st], v[0]), v[1]), v[2]), v[3]);
			} else {
#pragma unroll
				for (int r = 0; r < 4; ++r)
					if (item0 + (uint32_t)r < p.I) {
						if (q < p.Q) dst[r] = v[r];
						gmx[st] = fmaxf(gmx[st], v[r]);
					}
			}
			if (last) {
				float m = gmx[st];
				m = fmaxf(m, __shfl_xor(m, 16));
				m = fmaxf(m, __shfl_xor(m, 32));
				if (g4 == 0 && q < p.Q) p.GM[(int64_t)q * p.ldg + (t >> 2)] = m;
				gmx[st] = __uint_as_float(0x7fc00000u);
			}
		}
	}
}

// STEPS k-steps of 32 per unit of work; CHUNKED: a tile's rows in Kp / 128 units of four k-steps (Kp > 512), otherwise a unit is a tile
template <int STEPS, bool CHUNKED>
__global__ __launch_bounds__(FEW_WAVES * 64) void few_score_kernel(const FewScoreArgs p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int c16 = lane & 15, g4 = lane >> 4;
	const int Kp = CHUNKED ? p.Kp : STEPS * 32;
	const uint32_t rowb = (uint32_t)Kp * 2u + FEW_ROW_PAD;   // bytes between staged query rows
	if (p.hdr && blockIdx.x == 0) p.hdr[tid] = 0u;           // the workspace header: 256 words (the select writes its query's four after this launch)

	// ---- the queries, once per workgroup: 16-byte pieces, rows past Q as zeros
	{
		const int cpr = Kp / 8, n = 16 * p.nsub * cpr;
		for (int i = tid; i < n; i += FEW_WAVES * 64) {
			const int r = i / cpr, c = i - r * cpr;
			u32x4 v = {0u, 0u, 0u, 0u};
			if (r < p.Q) v = *reinterpret_cast<const u32x4 *>(p.X + (int64_t)r * p.ldx + 8 * c);
			*reinterpret_cast<u32x4 *>(smem + (uint32_t)r * rowb + 16u * (uint32_t)c) = v;
		}
	}
	__syncthreads();

	// ---- this wave's groups, tiles and units
	const int64_t g_lo = ((int64_t)blockIdx.x * FEW_WAVES + wave) * p.gpw;
	if (g_lo >= (int64_t)p.n_groups) return;
	const uint32_t g_hi = (uint32_t)(g_lo + p.gpw < (int64_t)p.n_groups ? g_lo + p.gpw : (int64_t)p.n_groups);
	const uint32_t t_lo = (uint32_t)g_lo * 4u, t_hi = g_hi * 4u < p.n_tiles ? g_hi * 4u : p.n_tiles;
	const uint32_t n_chunks = CHUNKED ? (uint32_t)Kp / (32u * STEPS) : 1u;
	const uint32_t n_units = (t_hi - t_lo) * n_chunks;
	const uint32_t lane_off = (uint32_t)c16 * (uint32_t)Kp * 2u + 16u * (uint32_t)g4;   // inside a tile: 32 bits
	const unsigned char *bq = smem + (uint32_t)c16 * rowb + 16u * (uint32_t)g4;         // this lane's B fragments: + 16 rows per sub-tile, + 64 bytes per k-step

	f32x4 acc[4];
	float gmx[4];
#pragma unroll
	for (int st = 0; st < 4; ++st) { acc[st] = (f32x4){0.f, 0.f, 0.f, 0.f}; gmx[st] = __uint_as_float(0x7fc00000u); }

	// unit u -> (tile, piece of its rows); the tile base in 64 bits
#define FEW_UNIT_PTR(u) (p.Et + (int64_t)(t_lo + (CHUNKED ? (u) / n_chunks : (u))) * (32 * (int64_t)Kp) + lane_off + (CHUNKED ? ((u) % n_chunks) * (64u * STEPS) : 0u))
#define FEW_CONSUME(BUF, u)                                                                                                     \
	do {                                                                                                                        \
		const uint32_t chunk_ = CHUNKED ? (u) % n_chunks : 0u;                                                                  \
		const uint32_t kb_ = chunk_ * (64u * STEPS);                                                                            \
		_Pragma("unroll") for (int s = 0; s < STEPS; ++s) {                                                                     \
			const bf16x8 a_ = __builtin_bit_cast(bf16x8, BUF[s]);                                                               \
			_Pragma("unroll") for (int st = 0; st < 4; ++st)                                                                    \
				if (st < p.nsub) {                                                                                              \
					const bf16x8 b_ = *reinterpret_cast<const bf16x8 *>(bq + (uint32_t)(16 * st) * rowb + kb_ + 64u * s);       \
					acc[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_, b_, acc[st], 0, 0, 0);                                \
				}                                                                                                               \
		}                                                                                                                       \
		if (chunk_ + 1u == n_chunks) few_tile_done(p, t_lo + (CHUNKED ? (u) / n_chunks : (u)), t_hi, c16, g4, acc, gmx);        \
	} while (0)

	u32x4 bufA[STEPS], bufB[STEPS];
	few_issue<STEPS>(bufA, FEW_UNIT_PTR(0u));
	for (uint32_t u = 0; u < n_units; u += 2) {
		if (u + 1 < n_units) few_issue<STEPS>(bufB, FEW_UNIT_PTR(u + 1));
		FEW_CONSUME(bufA, u);
		if (u + 1 >= n_units) break;
		if (u + 2 < n_units) few_issue<STEPS>(bufA, FEW_UNIT_PTR(u + 2));
		FEW_CONSUME(bufB, u + 1);
	}
#undef FEW_CONSUME
#undef FEW_UNIT_PTR
}

int launch_few_score(const FewPlan &P, const void *X, int64_t ldx, const void *Et, int64_t Q, int64_t I, int32_t Kp, float *S, int64_t lds, float *GM,
					 int64_t ldg, uint32_t *hdr, hipStream_t st) {
	FewScoreArgs a;
	a.X = (const uint16_t *)X; a.ldx = ldx; a.Et = (const unsigned char *)Et;
	a.Q = (int32_t)Q; a.Kp = Kp; a.gpw = P.gpw; a.nsub = P.nsub;
	a.I = (uint32_t)I; a.n_tiles = (uint32_t)P.tiles; a.n_groups = (uint32_t)P.groups;
	a.S = S; a.lds = lds; a.GM = GM; a.ldg = ldg; a.hdr = hdr;
	const int lds_bytes = 16 * P.nsub * (Kp * 2 + FEW_ROW_PAD);
#define FEW_LAUNCH(STEPS, CH)                                                                                                   \
	do {                                                                                                                        \
		const int rc_ = anncur_ensure_dyn_lds((const void *)few_score_kernel<STEPS, CH>, lds_bytes);                            \
		if (rc_ != ANNCUR_OK) return rc_;                                                                                       \
		hipLaunchKernelGGL((few_score_kernel<STEPS, CH>), dim3((unsigned)P.workgroups), dim3(FEW_WAVES * 64), lds_bytes, st, a); \
	} while (0)
	switch (Kp) {
		case 64: FEW_LAUNCH(2, false); break;
		case 128: FEW_LAUNCH(4, false); break;
		case 256: FEW_LAUNCH(8, false); break;
		case 512: FEW_LAUNCH(16, false); break;
		default: FEW_LAUNCH(4, true); break;
	}
#undef FEW_LAUNCH
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

// ------------------------------------------------------------------ launch 2
// sel_push with a capacity: the count goes on past `cap`, nothing is written there (the caller reads the count and falls back)
__device__ __forceinline__ void few_push(bool hit, uint64_t key, uint64_t *dst, uint32_t *cnt_ptr, uint32_t cap) {
	const unsigned long long mask = __ballot(hit);
	if (mask == 0ull) return;
	const int lane = lane_id();
	const int leader = __ffsll((long long)mask) - 1;
	uint32_t base = 0;
	if (lane == leader) base = atomicAdd(cnt_ptr, (uint32_t)__popcll(mask));
	base = __shfl(base, leader);
	const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
	if (hit && pos < cap) dst[pos] = key;
}

// the smallest of buf[0..n) (n >= 1), by the whole workgroup
__device__ uint64_t few_min_key(const SelState &s, uint32_t n) {
	if (threadIdx.x == 0) *reinterpret_cast<uint64_t *>(&s.scal[6]) = ~0ull;
	__syncthreads();
	uint64_t lmin = ~0ull;
	for (uint32_t i = threadIdx.x; i < n; i += SEL_THREADS) lmin = s.buf[i] < lmin ? s.buf[i] : lmin;
	for (int d = WAVE / 2; d > 0; d >>= 1) {
		const uint64_t o = __shfl_xor(lmin, d);
		if (o < lmin) lmin = o;
	}
	if (lane_id() == 0) atomicMin(reinterpret_cast<unsigned long long *>(&s.scal[6]), (unsigned long long)lmin);
	__syncthreads();
	return *reinterpret_cast<uint64_t *>(&s.scal[6]);
}

template <int KMAX>
struct FewSelCfg {
	static constexpr int CAP = SelCfg<KMAX>::CAP;                                   // cand_cap: the selector's own buffer
	static constexpr size_t LIST_OFF = (SelCfg<KMAX>::LDS_BYTES + 15) & ~(size_t)15;   // the round's groups to read
	static constexpr size_t LDS_BYTES = LIST_OFF + (size_t)FEW_ROUND * 4;
};

template <int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void few_select_kernel(const float *__restrict__ S, int64_t lds, const float *__restrict__ GM, int64_t ldg, uint32_t I,
																  uint32_t G, uint32_t k, float *__restrict__ out_val, int32_t *__restrict__ out_idx,
																  uint32_t *__restrict__ hdr) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	uint32_t *const glist = reinterpret_cast<uint32_t *>(smem + FewSelCfg<KMAX>::LIST_OFF);
	constexpr uint32_t CAP = FewSelCfg<KMAX>::CAP;
	sel_init(s);
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const int64_t q = blockIdx.x;
	const float *gm = GM + q * ldg;
	const float *row = S + q * lds;

	// ---- (a) tau: the k-th largest non-NaN group maximum (a NaN fails v >= tau and is never pushed)
	float tau = -INFINITY;
	uint64_t tau_key = 0;
	uint32_t pending = 0;   // (uniform)
	for (uint32_t g0 = 0; g0 < G; g0 += SEL_THREADS) {
		const uint32_t g = g0 + tid;
		const bool in = g < G;
		sel_offer(s, in, in ? gm[g] : 0.f, g, tau, tau_key);
		pending += SEL_THREADS;
		if (pending == (uint32_t)SEL_PASS) { sel_maybe_compact<KMAX>(s, k, tau, tau_key); pending = 0; }
	}
	__syncthreads();
	const uint32_t n_max = s.scal[0];
	float thr = -INFINITY;
	if (n_max > k) thr = key_val(sel_compact<KMAX>(s, k));
	else if (n_max == k) thr = key_val(few_min_key(s, k));
	__syncthreads();
	if (tid == 0) { s.scal[0] = 0u; s.scal[8] = 0u; }   // candidates, groups read

	// ---- (b) the groups at or above tau, FEW_ROUND maxima per round
	bool over = false;   // (uniform)
	for (uint32_t r0 = 0; r0 < G && !over; r0 += FEW_ROUND) {
		if (tid == 0) s.scal[9] = 0u;   // entries of glist
		__syncthreads();
		float m[FEW_ROUND / SEL_THREADS];
#pragma unroll
		for (int j = 0; j < FEW_ROUND / SEL_THREADS; ++j) {
			const uint32_t g = r0 + (uint32_t)j * SEL_THREADS + tid;
			m[j] = g < G ? gm[g] : __uint_as_float(0x7fc00000u);
		}
#pragma unroll
		for (int j = 0; j < FEW_ROUND / SEL_THREADS; ++j) {
			const bool hit = m[j] >= thr;
			const unsigned long long mask = __ballot(hit);
			if (mask != 0ull) {
				uint32_t base = 0;
				if (lane == 0) base = atomicAdd(&s.scal[9], (uint32_t)__popcll(mask));
				base = __shfl(base, 0);
				if (hit) glist[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = r0 + (uint32_t)j * SEL_THREADS + tid;
			}
		}
		__syncthreads();
		const uint32_t n_list = s.scal[9];
		for (uint32_t e0 = wave * FEW_READ_UNROLL; e0 < n_list; e0 += (SEL_THREADS / 64) * FEW_READ_UNROLL) {   // (wave-uniform)
			float v[FEW_READ_UNROLL];
			uint32_t item[FEW_READ_UNROLL];
#pragma unroll
			for (int j = 0; j < FEW_READ_UNROLL; ++j) {
				const bool in_list = e0 + (uint32_t)j < n_list;
				item[j] = (in_list ? glist[e0 + (uint32_t)j] : 0u) * FEW_GROUP + lane;
				v[j] = (in_list && item[j] < I) ? row[item[j]] : __uint_as_float(0x7fc00000u);
			}
#pragma unroll
			for (int j = 0; j < FEW_READ_UNROLL; ++j) few_push(v[j] >= thr, make_key(v[j], item[j]), s.buf, &s.scal[0], CAP);
		}
		__syncthreads();
		if (tid == 0) s.scal[8] += n_list;
		over = s.scal[0] > CAP;
	}
	__syncthreads();
	const uint32_t n_cand = s.scal[0], groups_read = s.scal[8];
	__syncthreads();

	// ---- (d) too many candidates: the whole row through the streaming selector (k items score >= thr, so it may start there)
	if (over) {
		if (tid == 0) s.scal[0] = 0u;
		__syncthreads();
		tau = thr; tau_key = 0; pending = 0;
		for (uint32_t i0 = 0; i0 < I; i0 += SEL_THREADS) {
			const uint32_t i = i0 + tid;
			const bool in = i < I;
			sel_offer(s, in, in ? row[i] : 0.f, i, tau, tau_key);
			pending += SEL_THREADS;
			if (pending == (uint32_t)SEL_PASS) { sel_maybe_compact<KMAX>(s, k, tau, tau_key); pending = 0; }
		}
	}
	// ---- (c) the k best of the buffer, sorted; pads behind them
	sel_finish<KMAX>(s, k, out_val + q * (int64_t)k, out_idx + q * (int64_t)k);
	if (tid == 0) {
		hdr[q * 4 + 0] = groups_read;
		hdr[q * 4 + 1] = n_cand;
		hdr[q * 4 + 2] = over ? 1u : 0u;
		hdr[q * 4 + 3] = 0u;
	}
}

template <int KM>
int launch_few_select_km(const FewPlan &P, const float *S, const float *GM, int64_t Q, int64_t I, int32_t k, float *out_val, int32_t *out_idx, uint32_t *hdr,
						 hipStream_t st) {
	const int rc = anncur_ensure_dyn_lds((const void *)few_select_kernel<KM>, (int)FewSelCfg<KM>::LDS_BYTES);
	if (rc != ANNCUR_OK) return rc;
	hipLaunchKernelGGL((few_select_kernel<KM>), dim3((unsigned)Q), dim3(SEL_THREADS), FewSelCfg<KM>::LDS_BYTES, st, S, P.pitch, GM, P.ldg, (uint32_t)I,
					   (uint32_t)P.groups, (uint32_t)k, out_val, out_idx, hdr);
	return ANNCUR_OK;
}

int few_check_operands(const char *what, const void *X, int64_t ldx, const void *Et, int64_t lde, int32_t Kp) {
	ANNCUR_REQUIRE(X && Et, ANNCUR_E_INVALID, "%s: null pointer", what);
	ANNCUR_REQUIRE(lde == Kp, ANNCUR_E_INVALID, "%s: Et must be packed (lde == Kp), got lde=%lld", what, (long long)lde);
	ANNCUR_REQUIRE(ldx >= Kp && (ldx % 8) == 0, ANNCUR_E_INVALID, "%s: ldx must be >= Kp and a multiple of 8 (got %lld)", what, (long long)ldx);
	ANNCUR_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)Et % 16) == 0, ANNCUR_E_INVALID, "%s: X and Et must be 16-byte aligned", what);
	return ANNCUR_OK;
}

#define FEW_LIMITS_FMT "1<=Q<=%d, Kp in {64,128,256,512} or a multiple of 128 up to 4096, 16*ceil(Q/16)*Kp*2 <= %d bytes of staged queries, I < 2^31-1"

}  // namespace

extern "C" int anncur_score_topk_few_supported(int64_t Q, int64_t I, int32_t Kp, int32_t k) { return few_plan_of(Q, I, Kp, k).ok ? 1 : 0; }

extern "C" size_t anncur_score_topk_few_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k) {
	const FewPlan P = few_plan_of(Q, I, Kp, k);
	return P.ok ? P.total : 0;
}

extern "C" int anncur_score_topk_few_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out, int32_t n_out) {
	ANNCUR_REQUIRE(out && n_out >= 1, ANNCUR_E_INVALID, "score_topk_few_plan: need an output array");
	const FewPlan P = few_plan_of(Q, I, Kp, k);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "score_topk_few_plan: (Q=%lld, I=%lld, Kp=%d, k=%d) is outside the small-batch route (" FEW_LIMITS_FMT ", 1<=k<=min(I, %d))",
				   (long long)Q, (long long)I, Kp, k, FEW_QMAX, FEW_STAGE_BYTES, ANNCUR_MAX_TOPK);
	const int32_t w[ANNCUR_FEW_PLAN_WORDS] = {(int32_t)P.tiles, P.workgroups, FEW_WAVES, P.tiles_min, P.tiles_max, P.nsub, (int32_t)P.groups, P.cand_cap,
											  (int32_t)(P.pitch / 32), P.gpw, (int32_t)(P.gm_off / 256), (int32_t)(P.s_off / 256)};
	for (int i = 0; i < n_out && i < ANNCUR_FEW_PLAN_WORDS; ++i) out[i] = w[i];
	return ANNCUR_OK;
}

extern "C" int anncur_score_rows_few(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, float *S, int64_t lds,
									  float *GM, int64_t ldg, void *stream) {
	const FewPlan P = few_plan_of(Q, I, Kp);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "score_rows_few: (Q=%lld, I=%lld, Kp=%d) is outside the small-batch route (" FEW_LIMITS_FMT ")", (long long)Q,
				   (long long)I, Kp, FEW_QMAX, FEW_STAGE_BYTES);
	if (const int rc = few_check_operands("score_rows_few", X, ldx, Et, lde, Kp)) return rc;
	ANNCUR_REQUIRE(S && GM, ANNCUR_E_INVALID, "score_rows_few: null output pointer");
	ANNCUR_REQUIRE(lds >= I && (lds % 4) == 0 && ((uintptr_t)S % 16) == 0, ANNCUR_E_INVALID, "score_rows_few: S must be 16-byte aligned with lds >= I and a multiple of 4 (got %lld)",
				   (long long)lds);
	ANNCUR_REQUIRE(ldg >= P.groups, ANNCUR_E_INVALID, "score_rows_few: ldg = %lld is shorter than the %lld groups of 64 items", (long long)ldg, (long long)P.groups);
	return launch_few_score(P, X, ldx, Et, Q, I, Kp, S, lds, GM, ldg, nullptr, (hipStream_t)stream);
}

extern "C" int anncur_score_topk_few(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, int32_t k, float *out_val,
									  int32_t *out_idx, void *workspace, size_t workspace_bytes, void *stream) {
	ANNCUR_REQUIRE(Q >= 1 && Q <= FEW_QMAX, ANNCUR_E_UNSUPPORTED, "score_topk_few: Q = %lld is outside 1..%d queries per call", (long long)Q, FEW_QMAX);
	ANNCUR_REQUIRE(I >= 1 && k >= 1 && k <= ANNCUR_MAX_TOPK && (int64_t)k <= I, ANNCUR_E_INVALID, "score_topk_few: k = %d is outside 1..min(I = %lld, %d)", k, (long long)I,
				   ANNCUR_MAX_TOPK);
	const FewPlan P = few_plan_of(Q, I, Kp, k);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "score_topk_few: (Q=%lld, I=%lld, Kp=%d, k=%d) is outside the small-batch route (" FEW_LIMITS_FMT ")", (long long)Q,
				   (long long)I, Kp, k, FEW_QMAX, FEW_STAGE_BYTES);
	if (const int rc = few_check_operands("score_topk_few", X, ldx, Et, lde, Kp)) return rc;
	ANNCUR_REQUIRE(out_val && out_idx, ANNCUR_E_INVALID, "score_topk_few: null output pointer");
	ANNCUR_REQUIRE(workspace && workspace_bytes >= P.total && ((uintptr_t)workspace % 256) == 0, ANNCUR_E_WORKSPACE,
				   "score_topk_few: workspace of %zu bytes (256-byte aligned) required, got %zu", P.total, workspace_bytes);
	hipStream_t st = (hipStream_t)stream;
	unsigned char *ws = (unsigned char *)workspace;
	uint32_t *hdr = reinterpret_cast<uint32_t *>(ws);
	float *GM = reinterpret_cast<float *>(ws + P.gm_off), *S = reinterpret_cast<float *>(ws + P.s_off);
	int rc = launch_few_score(P, X, ldx, Et, Q, I, Kp, S, P.pitch, GM, P.ldg, hdr, st);
	if (rc != ANNCUR_OK) return rc;
	switch (P.kmax) {
		case 128: rc = launch_few_select_km<128>(P, S, GM, Q, I, k, out_val, out_idx, hdr, st); break;
		case 512: rc = launch_few_select_km<512>(P, S, GM, Q, I, k, out_val, out_idx, hdr, st); break;
		default: rc = launch_few_select_km<2048>(P, S, GM, Q, I, k, out_val, out_idx, hdr, st); break;
	}
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
