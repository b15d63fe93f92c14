// The select side of the fused top-k (included by score_fused.hip): exact top-k of a query's candidate segments, with the repair of
// overflowed segments, and the threshold refinement between sweep stages.
#pragma once

// ------------------------------------------------------------------ select
// Item-tile ranges of the sweep stages (which tiles item split s swept in stage g): [begin[g] + s*tps[g], + tps[g]) below end[g].
// stride > 1: interleaved instead (split s swept begin[g] + s, + stride, ... below end[g]).
// chunk > 0: dynamic schedule -- stage g's tiles were swept in chunks of `chunk` tiles, chunk c of query row block rb by the item
// split owner[g][rb * n_chunks[g] + c] (row block = q / bq); chunk id c covers the tiles of position chunk_pos(c, rot, n_chunks[g]) (rot > 0:
// score16_kernel met the sampled tiles last; one stage).
struct SweepStages {
	int n, begin[3], end[3], tps[3], stride;
	int chunk, bq, n_chunks[3], rot;
	const uint8_t *owner[3];
};

// One workgroup per query: exact top-k of the query's candidate segments.  A segment that overflowed (or whose LDS ring
// wrapped: poisoned count) is repaired locally: the scores of the item tiles its split swept are recomputed here (fp32 dot
// products of the same bf16 operands) and offered unfiltered, the stored candidates of that split are ignored.  Only a query
// that still ends with fewer than k candidates is recomputed in full.
template <int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void select_candidates_kernel(
	const uint2 *__restrict__ cand, const uint32_t *__restrict__ seg_cnt, int nseg, int S, SweepStages stg, int capg,
	const uint16_t *__restrict__ X, int64_t ldx, const uint16_t *__restrict__ Et, int64_t I, int KP, uint32_t k,
	float *__restrict__ out_val, int32_t *__restrict__ out_idx, uint32_t *__restrict__ n_fallback,
	const int32_t *__restrict__ hard_list, const uint32_t *__restrict__ hard_cnt, const float *__restrict__ tau_in, int tau_stride,
	const int32_t *__restrict__ remap) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	float *xq = reinterpret_cast<float *>(smem + SelCfg<KMAX>::LDS_BYTES);  // [KP], repair / fallback only
	uint32_t *bad = reinterpret_cast<uint32_t *>(xq + KP);                  // [8]: bitmap of splits to repair (S <= 256)
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	auto score_of = [&](int64_t i) {
		float v = 0.f;
		const uint4 *er = reinterpret_cast<const uint4 *>(Et + i * KP);
		for (int c = 0; c < KP / 8; ++c) {
			const uint4 w = er[c];
			const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				v = fmaf(__uint_as_float(ww[d] << 16), xq[8 * c + 2 * d], v);
				v = fmaf(__uint_as_float(ww[d] & 0xffff0000u), xq[8 * c + 2 * d + 1], v);
			}
		}
		return v;
	};
	// either one query per workgroup (hard_list == nullptr) or a grid-stride walk over the queries the wave kernel deferred
	const uint32_t n_work = hard_list ? *hard_cnt : gridDim.x;
	for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
	__syncthreads();
	sel_init(s);
	if (tid < 8) bad[tid] = 0u;
	__syncthreads();
	const int64_t q = hard_list ? (int64_t)hard_list[wi] : (int64_t)wi;
	const uint32_t *cnts = seg_cnt + q * nseg;
	for (int sg = tid; sg < nseg; sg += SEL_THREADS) {
		const uint32_t c = cnts[sg];
		if (c > (uint32_t)capg) { const int sp = sg % S; atomicOr(&bad[sp >> 5], 1u << (sp & 31)); }
	}
	__syncthreads();
	const bool repair = (bad[0] | bad[1] | bad[2] | bad[3] | bad[4] | bad[5] | bad[6] | bad[7]) != 0u;
	for (int sg = tid; sg < nseg; sg += SEL_THREADS) {
		const int sp = sg % S;
		const uint32_t cc = ((bad[sp >> 5] >> (sp & 31)) & 1u) ? 0u : cnts[sg];
		atomicAdd(&s.scal[9], cc);
		atomicMax(&s.scal[10], cc);
	}
	__syncthreads();
	const uint32_t total = s.scal[9], maxc = s.scal[10];
	// (the threshold the last sweep stage ran with: earlier stages' candidates below it are dropped at the load)
	float tau = tau_in ? tau_in[q * tau_stride] : -INFINITY;
	uint64_t tau_key = 0;
	bool full = !repair && total < k;  // the sweep ran without a usable threshold -- a NaN query row, fewer than k non-NaN group maxima, or a k-th
	                                    // maximum of -inf (a NaN out of the coarse threshold kernel): nothing was offered, the whole row is rescanned (nfb counts it)
	if (!full) {
		for (int sb = 0; sb < nseg; sb += 4) {
			const int sg = sb + wave;
			const int sp = sg % S;
			const bool use = sg < nseg && !((bad[sp >> 5] >> (sp & 31)) & 1u);
			const uint32_t c = use ? cnts[sg] : 0u;
			const uint2 *sp_ptr = cand + (q * nseg + (sg < nseg ? sg : 0)) * (int64_t)capg;
			for (uint32_t e0 = 0; e0 < maxc; e0 += WAVE) {
				const uint32_t e = e0 + lane;
				const bool in = e < c;
				const uint2 ce = in ? sp_ptr[e] : make_uint2(0, 0);
				sel_offer(s, in, __uint_as_float(ce.x), ce.y, tau, tau_key);
				sel_maybe_compact<KMAX>(s, k, tau, tau_key);
			}
		}
	}
	if (repair || full) {
		if (tid == 0) atomicAdd(n_fallback, 1u);
		for (int c = tid; c < KP; c += SEL_THREADS) xq[c] = bf16_bits_to_f32(X[q * ldx + c]);
		__syncthreads();
	}
	if (repair) {
		for (int sp = 0; sp < S; ++sp) {
			if (!((bad[sp >> 5] >> (sp & 31)) & 1u)) continue;  // uniform
			for (int g = 0; g < stg.n; ++g) {
				if (stg.chunk > 0) {  // (uniform) dynamic schedule: the chunks of this query's row block that split sp drew
					const uint8_t *own = stg.owner[g] + (q / stg.bq) * (int64_t)stg.n_chunks[g];
					int it = 0;
					for (int c = 0; c < stg.n_chunks[g]; ++c) {
						if (own[c] != (uint8_t)sp) continue;  // (uniform: every thread reads the same byte)
						const int cp = chunk_pos(c, stg.rot, stg.n_chunks[g]);
						const int64_t i_beg = (int64_t)(stg.begin[g] + cp * stg.chunk) * TILE_I;
						const int64_t i_end = (int64_t)min(stg.begin[g] + (cp + 1) * stg.chunk, stg.end[g]) * TILE_I;
						for (int64_t i0 = i_beg; i0 < i_end; i0 += SEL_THREADS, ++it) {
							const int64_t i = i0 + tid;
							const bool in = i < i_end && i < I;
							const float v = in ? score_of(i) : 0.f;
							sel_offer(s, in, v, (uint32_t)i, tau, tau_key);
							if ((it & 15) == 15) sel_maybe_compact<KMAX>(s, k, tau, tau_key);
						}
					}
					sel_maybe_compact<KMAX>(s, k, tau, tau_key);
					continue;
				}
				if (stg.stride > 1) {  // (uniform) interleaved splits: tiles begin + sp, + stride, ...; 8 tiles (256 items) per pass
					int it = 0;
					for (int tb = stg.begin[g] + sp; tb < stg.end[g]; tb += 8 * stg.stride, ++it) {
						const int tile = tb + (tid >> 5) * stg.stride;
						const int64_t i = (int64_t)tile * TILE_I + (tid & 31);
						const bool in = tile < stg.end[g] && i < I;
						const float v = in ? score_of(i) : 0.f;
						sel_offer(s, in, v, (uint32_t)i, tau, tau_key);
						if ((it & 15) == 15) sel_maybe_compact<KMAX>(s, k, tau, tau_key);
					}
					sel_maybe_compact<KMAX>(s, k, tau, tau_key);
					continue;
				}
				const int t0 = stg.begin[g] + sp * stg.tps[g];
				const int t1 = min(t0 + stg.tps[g], stg.end[g]);
				int it = 0;
				for (int64_t i0 = (int64_t)t0 * TILE_I; i0 < (int64_t)t1 * TILE_I; i0 += SEL_THREADS, ++it) {
					const int64_t i = i0 + tid;
					const bool in = i < (int64_t)t1 * TILE_I && i < I;
					const float v = in ? score_of(i) : 0.f;
					sel_offer(s, in, v, (uint32_t)i, tau, tau_key);
					if ((it & 15) == 15) sel_maybe_compact<KMAX>(s, k, tau, tau_key);
				}
				sel_maybe_compact<KMAX>(s, k, tau, tau_key);
			}
		}
		__syncthreads();
		full = s.scal[0] < k && tau_key == 0;  // fewer than k even after the repair (and nothing was compacted away)
	}
	if (full) {
		__syncthreads();
		if (tid == 0) s.scal[0] = 0;
		__syncthreads();
		tau = -INFINITY; tau_key = 0;
		int it = 0;
		for (int64_t i0 = 0; i0 < I; i0 += SEL_THREADS, ++it) {
			const int64_t i = i0 + tid;
			const bool in = i < I;
			const float v = in ? score_of(i) : 0.f;
			sel_offer(s, in, v, (uint32_t)i, tau, tau_key);
			if ((it & 15) == 15) sel_maybe_compact<KMAX>(s, k, tau, tau_key);
		}
	}
	sel_finish<KMAX>(s, k, out_val + q * (int64_t)k, out_idx + q * (int64_t)k, remap);
	}
}

// Threshold refinement between sweep stages for k > 128 (workgroup-level selector): tau[q] = max(tau[q], k-th best candidate so far).
// A query with an overflowed segment, or with fewer than k candidates yet, keeps its (still valid) threshold.
template <int KMAX>
__global__ __launch_bounds__(SEL_THREADS) void tau_block_kernel(const uint2 *__restrict__ cand, const uint32_t *__restrict__ seg_cnt, int nseg,
																 int capg, uint32_t k, float *__restrict__ tau_out, int tau_stride, int prefilter) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const SelState s = sel_carve<KMAX>(smem);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t q = blockIdx.x;
	sel_init(s);
	const uint32_t *cnts = seg_cnt + q * nseg;
	for (int sg = tid; sg < nseg; sg += SEL_THREADS) {
		const uint32_t c = cnts[sg];
		if (c > (uint32_t)capg) atomicOr(&s.scal[8], 1u);
		atomicAdd(&s.scal[9], c > (uint32_t)capg ? 0u : c);
		atomicMax(&s.scal[10], c > (uint32_t)capg ? 0u : c);
	}
	__syncthreads();
	if (s.scal[8] != 0u || s.scal[9] <= k) return;  // (uniform)
	const uint32_t maxc = s.scal[10];
	float tau = prefilter ? tau_out[q * tau_stride] : -INFINITY;  // earlier candidates below the running threshold cannot be the k-th best
	uint64_t tau_key = 0;
	for (int sb = 0; sb < nseg; sb += 4) {
		const int sg = sb + wave;
		const uint32_t c = sg < nseg ? cnts[sg] : 0u;
		const uint2 *sp = cand + (q * nseg + (sg < nseg ? sg : 0)) * (int64_t)capg;
		for (uint32_t e0 = 0; e0 < maxc; e0 += WAVE) {
			const uint32_t e = e0 + lane;
			const bool in = e < c;
			const uint2 ce = in ? sp[e] : make_uint2(0, 0);
			sel_offer(s, in, __uint_as_float(ce.x), ce.y, tau, tau_key);
			sel_maybe_compact<KMAX>(s, k, tau, tau_key);
		}
	}
	__syncthreads();
	if (s.scal[0] > k) {  // (uniform) cut to k: the k-th best key is the new threshold
		tau_key = sel_compact<KMAX>(s, k);
		tau = key_val(tau_key);
	}
	if (tid == 0 && tau_key != 0 && s.scal[0] >= k) tau_out[q * tau_stride] = fmaxf(tau_out[q * tau_stride], tau);
}

// One WAVE per query (k <= 128, <= 64 segments): the query's candidate segments are streamed through the wave-level
// selector of wave_select.hpp (wave-private LDS buffer, ballot/popcount radix select, in-register bitonic sort).
// No workgroup barrier.  Queries whose segments overflowed or that collected fewer than k candidates are appended to
// hard_list for the workgroup-level kernel (which recomputes them exactly).
constexpr int WQ_CAP = 1024;
constexpr int WQ_K2 = 1024;  // largest k of the wave-level candidate select (select_stream.hpp: 16 keys per lane in the final sort)
template <int KW> struct WqCfg { static constexpr int CAP = KW <= 128 ? WQ_CAP : 2048, TRIGGER = CAP - WAVE, E = KW / 64; };

// TAU_ONLY (between sweep stages): no output, the query's threshold is raised to the k-th best candidate collected so far.
// KW = 128 or 512: capacity class of k.
template <bool TAU_ONLY, int KW = 128>
__global__ __launch_bounds__(256) void select_wave_kernel(const uint2 *__restrict__ cand, const uint32_t *__restrict__ seg_cnt, int nseg,
														   int capg, int64_t Q, uint32_t k, float *__restrict__ out_val,
														   int32_t *__restrict__ out_idx, uint32_t *__restrict__ hard_cnt,
														   int32_t *__restrict__ hard_list, float *__restrict__ tau, int tau_stride, int prefilter,
														   const int32_t *__restrict__ remap) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const int64_t q = (int64_t)blockIdx.x * 4 + wave;
	if (q >= Q) return;
	const uint32_t c = (lane < nseg) ? seg_cnt[q * nseg + lane] : 0u;
	const uint32_t inc = wave_scan_incl<DppAdd>(c);
	const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1), pre = inc - c;
	if (__ballot(c > (uint32_t)capg) != 0ull || total < k) {
		if (!TAU_ONLY && lane == 0) hard_list[atomicAdd(hard_cnt, 1u)] = (int32_t)q;
		return;  // TAU_ONLY: keep the old (still valid) threshold
	}
	constexpr int CAP = WqCfg<KW>::CAP, TRIGGER = WqCfg<KW>::TRIGGER;
	WaveSel w = wsel_init<CAP>(smem + wave * WaveSelLayout<CAP>::BYTES);
	// the threshold the last sweep stage ran with is a valid lower bound on the k-th best: candidates of earlier stages below it
	// are dropped at the load (at least k candidates are >= it by construction)
	if (tau && prefilter) w.tau = tau[q * tau_stride];
	const uint2 *qc = cand + q * nseg * (int64_t)capg;
	// The candidates are fetched LOAD_U chunks of 64 at a time: the batch's flat-index -> (segment, entry) searches advance in
	// LOCKSTEP (one round = LOAD_U independent ds_bpermute, one wait), the loads are unconditional (clamped address) and issued back
	// to back.  Written chunk by chunk hipcc emitted LOAD_U serial chains of seven LDS round trips and one exposed HBM latency per chunk.
	// (A search without LDS -- the segment ends read into scalars with v_readlane, every lane counting the ends at or below its index --
	//  was slower: 9.5 k instead of 5 k cycles per wave for the 23 ends x 8 chunks.)
	constexpr int LOAD_U = 8;
	for (uint32_t j0 = 0; j0 < total; j0 += LOAD_U * WAVE) {
		int sg[LOAD_U];  // last segment whose exclusive prefix is <= j (skips empty segments)
#pragma unroll
		for (int u = 0; u < LOAD_U; ++u) sg[u] = 0;
#pragma unroll
		for (int step = 32; step >= 1; step >>= 1) {
			if (step < nseg) {  // (uniform: segments >= nseg do not exist)
				uint32_t pv[LOAD_U];
#pragma unroll
				for (int u = 0; u < LOAD_U; ++u) pv[u] = __shfl(pre, (sg[u] + step) & 63);
#pragma unroll
				for (int u = 0; u < LOAD_U; ++u)
					if (sg[u] + step < nseg && pv[u] <= j0 + (uint32_t)(u * WAVE + lane)) sg[u] += step;
			}
		}
		uint32_t ps[LOAD_U];
#pragma unroll
		for (int u = 0; u < LOAD_U; ++u) ps[u] = __shfl(pre, sg[u]);
		uint2 e[LOAD_U];
#pragma unroll
		for (int u = 0; u < LOAD_U; ++u) {
			const uint32_t j = j0 + (uint32_t)(u * WAVE + lane);
			e[u] = qc[j < total ? (int64_t)sg[u] * capg + (j - ps[u]) : 0];
		}
#pragma unroll
		for (int u = 0; u < LOAD_U; ++u) {
			if (j0 + (uint32_t)(u * WAVE) < total) {  // (uniform)
				wsel_offer(w, j0 + (uint32_t)(u * WAVE + lane) < total, __uint_as_float(e[u].x), e[u].y);
				if (w.cnt > (uint32_t)TRIGGER) wsel_compact<4, false, true>(w, k);
			}
		}
	}
	if (TAU_ONLY) {
		if (w.cnt > k) wsel_compact<4, false, true>(w, k);
		if (lane == 0 && w.cnt >= k) tau[q * tau_stride] = fmaxf(tau[q * tau_stride], w.tau);
		return;
	}
	wsel_finish<0, 4, WqCfg<KW>::E, true>(w, k, out_val + q * (int64_t)k, out_idx + q * (int64_t)k, remap);
}
