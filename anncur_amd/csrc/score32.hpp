// The 32x32x16 bodies (included by score_fused.hip): the per-lane candidate rings (filter_one, mark_wrapped_raw, flush_queue), the tile
// functions stagger_tile / stagger1_tile, score_prepass_kernel and score_sweep_kernel.  Orientation and data layout: score_fused.hip.
#pragma once

// One accumulator element of the filter (element index e is a compile-time constant after unrolling).  The hit path is kept
// to the bare minimum (slot address, item id, one LDS store, count): the sweep is vector-issue bound, every instruction here is
// paid ~0.3 times per MFMA.  The queue is a ring of D slots; what does not belong in it is sorted out at flush time
// (items past I of the matrix' last, partial tile; a count above D = the ring wrapped = overflow).
// Measured on cfg2 (MI355X): branch version 0.58 ms per sweep, predicated version 0.655 ms independent of the hit rate (its
// compare -> exec -> store chain sits in front of the wave's next MFMA) -> the branch version is the one in use.
// (plan_stages picks the variant per sweep stage from the expected hit rate: predicated above ~0.5 taken branches per compare)
template <int D, bool FILTER_PREDICATED = false>
__device__ __forceinline__ void filter_one(float v, int e, float tau, uint32_t item0, uint32_t lq, uint32_t &qcnt) {
	static_assert((D & (D - 1)) == 0, "queue depth must be a power of two");
	// qcnt is kept pre-shifted (slot stride 2048 B); lq has bits 11..13 clear (16 KiB-aligned ring), so OR == ADD
	if (FILTER_PREDICATED) {
		// Branch-free: no wave-level "any hit" test, the push runs under the compare's lane mask (a block this short gets no
		// s_cbranch_execz from hipcc).  With lane = query the wave-level branch is taken by ~35 % of the compares at k = 100 and by nearly
		// all of them at k >= 500, and a taken branch (out and back) costs more than these always-issued instructions.
		// The compare is compiler-generated, so hipcc keeps its own MFMA -> VALU distance; the first version of this variant did the
		// compare INSIDE an inline-asm string, 0-6 wait states behind the MFMA whose result it read, and lost a survivor now and then
		// (found by the randomised parity run; scripts/check_mfma_hazards.py flags exactly that string).
		if (v >= tau) {
			lds_write_2x32((qcnt & (uint32_t)((D - 1) << 11)) | lq, __float_as_uint(v), item0 + (uint32_t)((e & 3) + 8 * (e >> 2)));
			qcnt += 2048u;
		}
	} else if (__builtin_expect(__ballot(v >= tau) != 0ull, 0)) {
		if (v >= tau) {
			lds_write_2x32((qcnt & (uint32_t)((D - 1) << 11)) | lq, __float_as_uint(v), item0 + (uint32_t)((e & 3) + 8 * (e >> 2)));
			qcnt += 2048u;
		}
	}
}

// Dense splits (norm-ordered rows: the leading splits of the first stage; their rings are drained every tile): a lane that finds
// more than D survivors in ONE tile has wrapped its ring.  At k = 500 the prepass threshold lets about half of the leading tiles'
// elements through and a handful of queries did this in every call -- each one a whole-split repair by the workgroup-level kernel
// (0.26 ms per call for five queries).  The tile's accumulator is still in registers when its filter ends, and the lane's ring is
// 8 slots x 8 bytes = 16 floats: the lane overwrites its ring with the RAW accumulator (mark_wrapped_raw) and flags its count; the
// next flush filters those 16 scores itself.  Exact, no repair, and nothing but the accumulator, the ring address and the count is
// live where it happens (a direct store to the segment from inside the tile function cost the headline kernel its registers: the
// query operand went to scratch).  The ring must hold nothing but that tile's survivors, i.e. the split drains every tile.
constexpr uint32_t RING_RAW = 0x80000000u;
template <int D>
__device__ __forceinline__ void mark_wrapped_raw(const f32x16 &acc, uint32_t lq, uint32_t &qcnt) {
	static_assert(D == 8, "the raw tile (16 floats) fills the ring exactly");
	const bool wrapped = (qcnt >> 11) > (uint32_t)D && qcnt < RING_RAW;
	if (__builtin_expect(__ballot(wrapped) != 0ull, 0)) {
		if (wrapped) {
#pragma unroll
			for (int i = 0; i < D; ++i) lds_write_2x32(lq + (uint32_t)i * 2048u, __float_as_uint(acc[2 * i]), __float_as_uint(acc[2 * i + 1]));
			qcnt = RING_RAW;
		}
	}
}

// Drain the lane's ring to its HBM candidate segment: one store instruction per queue slot for the whole wave.
// raw_item0: first item (+ 4 h) of the tile a RING_RAW ring holds (dense splits only).
template <int D, bool BATCH = true>
__device__ __forceinline__ void flush_queue(uint32_t lq, uint32_t &qcnt, uint2 *__restrict__ seg, uint32_t &ncand, uint32_t capg,
											 uint32_t n_items, float tau, uint32_t raw_item0) {
	if (__builtin_expect(__ballot(qcnt >= RING_RAW) != 0ull, 0)) {
		if (qcnt >= RING_RAW) {
			for (int i = 0; i < D; ++i) {
				const uint2 w = lds_load_u64(lq + (uint32_t)i * 2048u);
#pragma unroll
				for (int half = 0; half < 2; ++half) {
					const int e = 2 * i + half;
					const float v = __uint_as_float(half ? w.y : w.x);
					const uint32_t item = raw_item0 + (uint32_t)((e & 3) + 8 * (e >> 2));
					if (v >= tau && item < n_items) {
						if (ncand < capg) seg[ncand] = make_uint2(__float_as_uint(v), item);
						ncand++;
					}
				}
			}
			qcnt = 0;
		}
	}
	uint32_t n = qcnt >> 11;  // (the filter keeps the count pre-shifted by the slot stride)
	if (__builtin_expect(__ballot(n > (uint32_t)D) != 0ull, 0)) {
		// ring wrapped between two flushes of a multi-tile window (p ~ 1e-9 per window): poison the segment count -> the select
		// kernel recomputes this query exactly
		if (n > (uint32_t)D) { ncand = 0x80000000u; n = D; }
	}
	if constexpr (!BATCH) {  // (the three-workgroups-per-CU body of ANNCUR_TOPK_QT1 has no sixteen registers to spare: slot by slot)
		for (uint32_t i = 0; __ballot(i < n) != 0ull; ++i) {
			if (i < n) {
				const uint2 w = lds_load_u64(lq + i * 2048u);
				if (w.y < n_items) {
					if (ncand < capg) seg[ncand] = w;
					ncand++;
				}
			}
		}
		qcnt = 0;
		return;
	}
	// Read the occupied slots back to back, wait ONCE, then store.  (Round 2 read, waited and stored slot by slot: a drain with three
	// entries in its fullest ring paid three exposed LDS round trips -- at k = 500, where every tile is drained and the fullest of the 64
	// rings holds 3-4 entries, that was more wave time than the tile's MFMAs.)  Slot i is read if ANY lane holds more than i entries.
	unsigned long long e[D];
	int n_read = 0;  // (uniform) slots read = the fullest ring's count
#pragma unroll
	for (int i = 0; i < D; ++i) {
		if (__ballot((uint32_t)i < n) == 0ull) break;
#if defined(__HIP_DEVICE_COMPILE__)
		asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(e[i]) : "v"(lq), "n"(i * 2048));
#endif
		n_read = i + 1;
	}
#if defined(__HIP_DEVICE_COMPILE__)
	static_assert(D == 8, "the wait below names eight slots");
	// (the destinations are in flight until here; naming them as in/out operands keeps every use below the wait)
	asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3]), "+v"(e[4]), "+v"(e[5]), "+v"(e[6]), "+v"(e[7])::"memory");
#endif
#pragma unroll
	for (int i = 0; i < D; ++i) {
		if (i >= n_read) break;
		if ((uint32_t)i < n) {
			const uint2 w = make_uint2((uint32_t)e[i], (uint32_t)(e[i] >> 32));
			if (w.y < n_items) {               // (items past I exist only in the matrix' last, partial tile)
				if (ncand < capg) seg[ncand] = w;
				ncand++;                        // (a poisoned count stays > capg)
			}
		}
	}
	qcnt = 0;
}

// One 32-item tile of the staggered sweep (Kp <= 256): the wave's two 32-query sub-tiles run half a tile apart.  While the
// MFMA chain of one sub-tile executes on the matrix pipe, the threshold filter of the OTHER sub-tile's finished accumulator
// is issued element by element in the MFMA shadow (one accumulator register per k-step at Kp = 256):
//   steps 0..K-1   : accA (sub-tile 0 of this tile)  ||  filter of acc1 = sub-tile 1 of the PREVIOUS tile
//   steps K..2K-1  : acc1 (sub-tile 1 of this tile)  ||  filter of accA
// The A fragments (same K fragments for both halves) stream through one ring of AR registers, AR-1 steps ahead, without a
// break between the halves.  CUR = tile buffer parity (compile-time: an immediate offset of the LDS reads).
// Fragment address of k-step s (tile buffer 0): row r, chunk (2 s + h) ^ f(r).  For Kp = 256 (32 chunks per row, f(r) = r & 15) the XOR
// leaves bit 4 of the chunk alone, so k-steps s and s + 8 are 256 bytes apart: eight address registers plus an immediate offset serve
// the sixteen k-steps (the eight registers this saves are what the dynamic tile schedule's ticket lives in).
template <int KP, int CUR, bool PRED>
__device__ __forceinline__ void stagger_tile(const uint32_t (&aoff)[FusedCfg<KP>::NAOFF], const bf16x8 (&xb)[2][FusedCfg<KP>::KSTEPS],
											  f32x16 &acc1, float tau0, float tau1_prev, uint32_t item0, uint32_t item0_prev,
											  uint32_t lq0, uint32_t lq1, uint32_t &q0, uint32_t &q1, bool dense) {
	using Cfg = FusedCfg<KP>;
	constexpr int K = Cfg::KSTEPS, AR = 5, DIST = 3, OFF = CUR * Cfg::TILE_BYTES;  // ring slots / prefetch distance in k-steps
	constexpr int NA = Cfg::NAOFF;
	constexpr int EPS = 16 / K > 0 ? 16 / K : 1;  // filter elements per k-step (Kp = 64: 4, 128: 2, 256: 1)
	static_assert(K <= 16 && 2 * K >= DIST && AR >= DIST + 2, "staggered path: 2..16 k-steps; a slot is rewritten two MFMAs after its use");
	static_assert(K <= NA || Cfg::CPR == 32, "k-steps beyond the address registers: + 256 bytes needs 32 chunks per row");
	u32x4 ring[AR];
#define ST_READ(slot, s) lds_read_frag_at(ring[slot], aoff[((s) % K) % NA], OFF + (((s) % K) / NA) * 256)
#pragma unroll
	for (int i = 0; i < DIST; ++i) ST_READ(i, i);
	f32x16 accA = {0}, accB = {0};
#pragma unroll
	for (int g = 0; g < 2 * K; ++g) {
		// the slot the new fragment lands in was consumed by the MFMA of step g-2: the asynchronous LDS return can never meet
		// an MFMA that is still reading its operands
		const int nxt = g + DIST;
		if (nxt < 2 * K) ST_READ(nxt % AR, nxt);
#if defined(__HIP_DEVICE_COMPILE__)
		// (keeps the register allocator from handing that read the registers of the fragment the PREVIOUS MFMA was given)
		if (g >= 1) asm volatile("" ::"v"(ring[(g - 1) % AR]));
#endif
		const int after = 2 * K - 1 - g;
		lds_wait_frag(ring[g % AR], after < DIST ? after : DIST);
		const bf16x8 a = __builtin_bit_cast(bf16x8, ring[g % AR]);
		if (g < K) {
			accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[0][g], accA, 0, 0, 0);
#pragma unroll
			for (int e = (g == 1 ? 0 : g) * EPS; e < (g == 0 ? 0 : g + 1) * EPS; ++e)
				filter_one<Cfg::QDEPTH, PRED>(acc1[e], e, tau1_prev, item0_prev, lq1, q1);
			if (g == K - 1 && dense) mark_wrapped_raw<Cfg::QDEPTH>(acc1, lq1, q1);  // (uniform) the previous tile's sub-tile 1 is filtered
		} else {
			// no filter in the first step of the half: accA's last MFMA is still in the pipe (and the predicated filter is
			// inline asm, invisible to the compiler's MFMA -> VALU hazard handling); step 1 takes two groups instead
			accB = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[1][g - K], accB, 0, 0, 0);
#pragma unroll
			for (int e = (g - K == 1 ? 0 : g - K) * EPS; e < (g == K ? 0 : g - K + 1) * EPS; ++e)
				filter_one<Cfg::QDEPTH, PRED>(accA[e], e, tau0, item0, lq0, q0);
		}
	}
#undef ST_READ
	if (dense) mark_wrapped_raw<Cfg::QDEPTH>(accA, lq0, q0);  // (uniform) this tile's sub-tile 0 is filtered
	acc1 = accB;
}

// Wait states between the last MFMA of an accumulate chain and the first instruction that is not the next MFMA of that chain
// (hipcc's own floor for the 8-pass 32x32x16 bf16 MFMA is 11).  hipcc pads this itself -- except where it does not: in the first
// version of stagger1_tile (one accumulator, `accP = acc` at the end of the tile) it copied the accumulator EIGHT states after the
// last MFMA on one path of the unrolled loop (MFMA, s_cbranch, v_lshl_or, s_nop 5, v_mov ...), so three registers were copied without
// the last k-step's contribution whenever instruction fetch did not happen to supply the missing states -- which depended on where
// the loop sat in memory: the shipped build passed every parity test, a diagnostic build with two more instructions in the prologue
// returned wrong scores for item rows 24-26 / 28-30 of every second tile.  scripts/check_mfma_hazards.py (run by the CPU tests on the
// built library) now walks every kernel for this; the statement below makes the distance explicit where a chain ends.
__device__ __forceinline__ void mfma_chain_done(f32x16 &acc) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("s_nop 7\n\ts_nop 2" : "+v"(acc));
#endif
}

// One 32-query sub-tile per wave (Kp = 512, where the query operand alone takes 128 VGPRs; Kp = 128 / 256 under ANNCUR_TOPK_QT1, for
// three workgroups per CU): the same idea across TILES -- while the
// 32-MFMA chain of tile j executes into `acc`, the filter of tile j-1's accumulator `accP` is issued in its shadow, one element every
// second k-step; A fragments through the counted-wait register ring as in stagger_tile.  The caller alternates two accumulators
// (no copy: see mfma_chain_done).  Fragment address of k-step s:
// row * CPR * 16 + ((2 s + h) ^ (r & 15)) * 16 = aoff8[s & 7] + (s >> 3) * 256 (the XOR only touches the chunk's low four bits),
// so eight address registers serve the 32 k-steps.
template <int KP, int CUR>
__device__ __forceinline__ void stagger1_tile(const uint32_t (&aoff8)[8], const bf16x8 (&xb)[FusedCfg<KP, 1>::KSTEPS], f32x16 &acc,
											   const f32x16 &accP, float tau, uint32_t item0_prev, uint32_t lq, uint32_t &qcnt, bool dense) {
	using Cfg = FusedCfg<KP, 1>;
	constexpr int K = Cfg::KSTEPS, AR = 5, DIST = 3, OFF = CUR * Cfg::TILE_BYTES;
	static_assert((K == 32 || K == 16 || K == 8) && Cfg::CPR >= 16, "Kp = 128, 256 or 512");
	u32x4 ring[AR];
#define S1_READ(slot, s) lds_read_frag_at(ring[slot], aoff8[(s) & 7], OFF + ((s) >> 3) * 256)
	S1_READ(0, 0); S1_READ(1, 1); S1_READ(2, 2);
#pragma unroll
	for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
	for (int g = 0; g < K; ++g) {
		const int nxt = g + DIST;
		if (nxt < K) S1_READ(nxt % AR, nxt);
#if defined(__HIP_DEVICE_COMPILE__)
		if (g >= 1) asm volatile("" ::"v"(ring[(g - 1) % AR]));
#endif
		const int after = K - 1 - g;
		lds_wait_frag(ring[g % AR], after < DIST ? after : DIST);
		acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ring[g % AR]), xb[g], acc, 0, 0, 0);
		if constexpr (K == 32) {  // one element every second k-step
			if (g & 1) filter_one<Cfg::QDEPTH>(accP[g >> 1], g >> 1, tau, item0_prev, lq, qcnt);
		} else {                  // 16 / K elements per k-step
#pragma unroll
			for (int e = g * (16 / K); e < (g + 1) * (16 / K); ++e) filter_one<Cfg::QDEPTH>(accP[e], e, tau, item0_prev, lq, qcnt);
		}
	}
#undef S1_READ
	mfma_chain_done(acc);
	if (dense) mark_wrapped_raw<Cfg::QDEPTH>(accP, lq, qcnt);  // (uniform) the previous tile is filtered
}

// Prepass on the 32x32x16 body: group maxima (GROUP = 16 or 4 items per maximum) of S_hat over the sample tiles, plain double-buffered
// tile loop with compiler-placed fragment reads.  (The plans that sweep with score16_kernel run prepass16_kernel instead.)
template <int KP, int GROUP, int QTV = FusedCfg<KP>::QT>
__global__ __launch_bounds__(256, (QTV == 1 && KP <= 256) ? 3 : 2) void score_prepass_kernel(const FusedParams p) {
	using Cfg = FusedCfg<KP, QTV>;
	constexpr int KSTEPS = Cfg::KSTEPS, QT = Cfg::QT, CPR = Cfg::CPR;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int r = lane & 31, h = lane >> 5;
	zero_ws_header(p);
	const int wid = xcd_remap(blockIdx.x, p.n_wg);
	const int n_rb = (int)((p.Q + Cfg::BQ - 1) / Cfg::BQ);
	const int split = wid / n_rb, rb = wid - split * n_rb;

	// ---- this wave's queries: B operand fragments, resident for the whole kernel
	bf16x8 xb[QT][KSTEPS];
	int64_t qv[QT];
#pragma unroll
	for (int t = 0; t < QT; ++t) {
		qv[t] = (int64_t)rb * Cfg::BQ + wave * 32 * QT + 32 * t + r;
		LOAD_QUERIES32(qv[t], h, xb[t]);
	}
	__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the fragments are complete before the tile loop (see score_sweep_kernel)

	// ---- work range: sample tiles [j_begin, j_end) of p.n_st; sample tile j is the matrix' tile tile_of(j)
	const int j_begin = split * p.st_per_split, j_end = min(j_begin + p.st_per_split, p.n_st);
#define tile_of(j) (!p.sample_leading ? (int)(((int64_t)(j) * p.n_full_tiles) / p.n_st) : (j))
	if (j_begin < j_end) tile_dma<KP>(p.Et, tile_of(j_begin), smem, wave, lane);
	__builtin_amdgcn_s_waitcnt(0x0F70);
	__syncthreads();
	ANNCUR_PAD_HERE();

	int cur = 0;
	for (int j = j_begin; j < j_end; ++j, cur ^= 1) {
		if (j + 1 < j_end) tile_dma<KP>(p.Et, tile_of(j + 1), smem + (cur ^ 1) * Cfg::TILE_BYTES, wave, lane);
		f32x16 acc[QT];
#pragma unroll
		for (int t = 0; t < QT; ++t)
#pragma unroll
			for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
		const u32x4 *tb = reinterpret_cast<const u32x4 *>(smem + cur * Cfg::TILE_BYTES);
#pragma unroll
		for (int s = 0; s < KSTEPS; ++s) {
			const u32x4 w = tb[r * CPR + swz<CPR>(r, 2 * s + h)];
			const bf16x8 a = __builtin_bit_cast(bf16x8, w);
#pragma unroll
			for (int t = 0; t < QT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[t][s], acc[t], 0, 0, 0);
		}

		// ---- epilogue.  C/D layout: query = lane & 31 (col), item row = (e & 3) + 8 * (e >> 2) + 4 * h
#pragma unroll
		for (int t = 0; t < QT; ++t) {
			if (GROUP == 16) {
				float m = acc[t][0];
#pragma unroll
				for (int e = 1; e < 16; ++e) m = fmaxf(m, acc[t][e]);
				if (qv[t] < p.Q) p.gmax[qv[t] * p.n_groups + (int64_t)j * 2 + h] = m;
			} else {
				float4 m;
				m.x = fmaxf(fmaxf(acc[t][0], acc[t][1]), fmaxf(acc[t][2], acc[t][3]));
				m.y = fmaxf(fmaxf(acc[t][4], acc[t][5]), fmaxf(acc[t][6], acc[t][7]));
				m.z = fmaxf(fmaxf(acc[t][8], acc[t][9]), fmaxf(acc[t][10], acc[t][11]));
				m.w = fmaxf(fmaxf(acc[t][12], acc[t][13]), fmaxf(acc[t][14], acc[t][15]));
				if (qv[t] < p.Q) *reinterpret_cast<float4 *>(p.gmax + qv[t] * p.n_groups + ((int64_t)j * 2 + h) * 4) = m;
			}
		}
		__builtin_amdgcn_s_waitcnt(0x0F70);  // the DMA of tile j+1 has landed
		__syncthreads();
	}
#undef tile_of
}

// Filter sweep on the 32x32x16 body with per-lane rings (PRED: branch-free filter, for stages in which most compares find a survivor in
// some lane -- large k).  Three tile functions on one schedule: two sub-tiles per wave staggered inside a tile (stagger_tile, Kp <= 256),
// one sub-tile per wave pipelined across tiles (stagger1_tile: Kp = 512, and Kp = 128 / 256 under ANNCUR_TOPK_QT1).
template <int KP, bool PRED = false, int QTV = FusedCfg<KP>::QT>
__global__ __launch_bounds__(256, (QTV == 1 && KP <= 256) ? 3 : 2) void score_sweep_kernel(const FusedParams p) {
	using Cfg = FusedCfg<KP, QTV>;
	constexpr int KSTEPS = Cfg::KSTEPS, QT = Cfg::QT, CPR = Cfg::CPR;
	static_assert(QT == 2 || (KP >= 128 && !PRED), "one sub-tile per wave: stagger1_tile (Kp >= 128, branch filter)");
	constexpr bool FLUSH_BATCH = !(QTV == 1 && KP <= 256);   // (see flush_queue)
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int r = lane & 31, h = lane >> 5;
	const int wid = xcd_remap(blockIdx.x, p.n_wg);
	const int n_rb = (int)((p.Q + Cfg::BQ - 1) / Cfg::BQ);
	const int split = wid / n_rb, rb = wid - split * n_rb;

	// ---- this wave's queries: B operand fragments, resident for the whole kernel
	bf16x8 xb[QT][KSTEPS];
	int64_t qv[QT];
#pragma unroll
	for (int t = 0; t < QT; ++t) {
		qv[t] = (int64_t)rb * Cfg::BQ + wave * 32 * QT + 32 * t + r;
		LOAD_QUERIES32(qv[t], h, xb[t]);
	}

	// The X fragments must be complete before the tile loop: otherwise hipcc's wait-count merge at the loop header
	// (fragment loads possibly pending + an unknown number of candidate stores on the back edge) makes it wait
	// vmcnt(0) in front of the first MFMA of EVERY tile, i.e. right after issuing the next tile's loads.
	__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only

	// ---- work range
	int j_begin, j_end;  // tile iterations
	if (p.tile_step > 1) { j_begin = p.tile_begin + split; j_end = p.tile_end; }                                        // interleaved splits
	else { j_begin = p.tile_begin + split * p.tiles_per_split; j_end = min(j_begin + p.tiles_per_split, p.tile_end); }  // contiguous shares
	const int ts = p.tile_step > 1 ? p.tile_step : 1;  // distance between two tiles of this workgroup
	// Norm-ordered rows: the survivors crowd into the leading tiles (several times the average density: about half of their elements
	// pass the prepass threshold at large k).  The first quarter of the first stage's tiles is swept with the rings drained every
	// tile (a ring then holds nothing but one tile: see mark_wrapped_raw); a step drains when the tile before it was such a tile.
	const int dense_end = (p.sample_leading && !p.carry) ? p.tile_begin + (p.tile_end - p.tile_begin + 3) / 4 : p.tile_begin;
	const bool every_tile = p.flush_tiles <= 1;  // (uniform) the whole stage drains every tile (large k): every ring holds one tile

	float tau[QT];
	uint32_t ncand[QT], qcnt[QT];
#pragma unroll
	for (int t = 0; t < QT; ++t) {
		tau[t] = qv[t] < p.Q ? p.tau[qv[t] * p.tau_stride] : INFINITY;
		ncand[t] = qv[t] < p.Q ? (p.carry ? p.seg_cnt[qv[t] * p.nseg + h * p.S + split] : 0u) : PAD_ROW_COUNT;
		qcnt[t] = 0;
	}
	// candidate segment of (query, lane half, split); sub-tile t adds a wave-uniform stride
	uint2 *seg0 = p.cand + (qv[0] * p.nseg + h * p.S + split) * (int64_t)p.capg;
	const int64_t seg_dt = (int64_t)32 * p.nseg * p.capg;
	const uint32_t lq0 = lds_addr(smem + Cfg::QUEUE_OFF) + (uint32_t)tid * 8u;  // slot i of sub-tile t at byte lq0 + (t*QDEPTH + i)*2048
	static_assert(Cfg::QUEUE_OFF % (Cfg::QDEPTH * 2048) == 0 && Cfg::QDEPTH * 2048 == 16384, "ring must be 16 KiB aligned");
	if ((lds_addr(smem) & 0x3fffu) != 0u) __builtin_trap();  // filter_one() ORs the slot offset into the address

	uint32_t last_item0 = 0;  // first item (+ 4 h) of the last tile filtered: what a raw ring holds at the final flush
	// ---- tile schedule (tile_schedule.hpp): static shares (contiguous, or interleaved with step ts), or tickets for the two-sub-tile body
	TILE_SCHEDULE_BEGIN(QT == 2 && p.chunk_tiles > 0, false, lds_addr(smem + Cfg::TICKET_OFF), TILE_OF_CHUNK)
	const int t_step = dyn ? 1 : ts;
	int t_prev = -1;
	const int wave_u = __builtin_amdgcn_readfirstlane(wave);             // (the compiler does not know tid >> 6 is wave-uniform)
	const uint32_t lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr(smem));
	uint32_t dma_off[Cfg::TILE_BYTES / 4096];
	tile_dma_offsets<KP>(dma_off, wave_u, lane);
	if (t_cur >= 0) tile_dma_s<KP>(p.Et, t_cur, lds_base, wave_u, dma_off);
	__builtin_amdgcn_s_waitcnt(0x0F70);
	__syncthreads();
	ANNCUR_PAD_HERE();


	if constexpr (QT == 2) {
		// ---- staggered sweep (stagger_tile): tile loop unrolled by two so that the LDS buffer parity is a compile-time offset
		f32x16 acc1;
#pragma unroll
		for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
		float tau1_prev = INFINITY;  // no previous tile yet: the filter of acc1 never fires
		uint32_t item0_prev = 0, item0_pp = 0;   // first item (+ 4 h) of the previous tile and of the one before it
		const uint32_t lq1 = lq0 + Cfg::QDEPTH * 2048;
		uint32_t aoff[Cfg::NAOFF];   // LDS byte address of this lane's A fragment of k-step s (< NAOFF) in tile buffer 0
#pragma unroll
		for (int s = 0; s < Cfg::NAOFF; ++s) aoff[s] = lds_addr(smem) + (uint32_t)(r * CPR + swz<CPR>(r, 2 * s + h)) * 16u;
		int flush_in2 = p.flush_tiles;
		// stagger_tile() counts LDS reads with lgkmcnt(n): no scalar load of the prologue may still be in flight (scalar loads share
		// the counter and return out of order)
		__builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
// (Round 3 tried draining by occupancy as well -- a ballot "some lane's ring holds >= 3 / >= 4 entries" per step, beside or instead of the
//  planned window: both cost 4 % of the sweep at cfg2, same box, alternating -- the check itself, not the drains.  The planned window stays.)
#define STAGGER_STEP(CUR)                                                                                                       \
		do {                                                                                                                    \
			TILE_STEP_HEAD(KP, CUR, TILE_OF_CHUNK, t_step)                                                                      \
			if (t_prev < dense_end || --flush_in2 <= 0) {                                                                       \
				flush_in2 = p.flush_tiles;                                                                                      \
				/* (a raw ring holds one tile: sub-tile 0 of the previous tile, sub-tile 1 of the one before) */                \
				flush_queue<Cfg::QDEPTH>(lq0, qcnt[0], seg0, ncand[0], (uint32_t)p.capg, (uint32_t)p.I, tau[0], item0_prev);    \
				flush_queue<Cfg::QDEPTH>(lq1, qcnt[1], seg0 + seg_dt, ncand[1], (uint32_t)p.capg, (uint32_t)p.I, tau[1], item0_pp); \
			}                                                                                                                   \
			const uint32_t item0 = (uint32_t)J * TILE_I + 4 * h;                                                                \
			stagger_tile<KP, CUR, PRED>(aoff, xb, acc1, tau[0], tau1_prev, item0, item0_prev, lq0, lq1, qcnt[0], qcnt[1], J < dense_end || every_tile); \
			tau1_prev = tau[1]; item0_pp = item0_prev; item0_prev = item0;                                                      \
			TILE_STEP_TAIL(false, )                                                                                             \
			t_prev = J;                                                                                                         \
		} while (0)
		while (t_cur >= 0) {
			STAGGER_STEP(0);
			if (t_cur < 0) break;
			STAGGER_STEP(1);
		}
#undef STAGGER_STEP
		flush_queue<Cfg::QDEPTH>(lq1, qcnt[1], seg0 + seg_dt, ncand[1], (uint32_t)p.capg, (uint32_t)p.I, tau[1], item0_pp);  // keep one tile's hits per queue window
#pragma unroll
		for (int e = 0; e < 16; ++e)  // drain: sub-tile 1 of the last tile
			filter_one<Cfg::QDEPTH>(acc1[e], e, tau1_prev, item0_prev, lq1, qcnt[1]);
		mark_wrapped_raw<Cfg::QDEPTH>(acc1, lq1, qcnt[1]);  // (its ring was just drained: exact in every split)
		last_item0 = item0_prev;
	} else {
		// ---- one sub-tile per wave, software-pipelined across tiles (stagger1_tile): tile loop unrolled by two (buffer parity =
		// immediate offset); even steps accumulate into accA and filter accB, odd steps the other way round
		f32x16 accA, accB;
#pragma unroll
		for (int e = 0; e < 16; ++e) { accA[e] = 0.f; accB[e] = 0.f; }
		float tau_prev = INFINITY;   // no previous tile yet: the filter never fires
		uint32_t item0_prev = 0, item0_pp = 0;
		uint32_t aoff8[8];
#pragma unroll
		for (int s = 0; s < 8; ++s) aoff8[s] = lds_addr(smem) + (uint32_t)(r * CPR + ((2 * s + h) ^ (r & 15))) * 16u;
		int flush_in2 = p.flush_tiles;
		__builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): stagger1_tile() counts LDS reads
#define STAGGER1_STEP(CUR, ACC, ACCP)                                                                                           \
		do {                                                                                                                    \
			TILE_STEP_HEAD(KP, CUR, TILE_OF_CHUNK, t_step)                                                                      \
			if (t_prev < dense_end || --flush_in2 <= 0) {                                                                       \
				flush_in2 = p.flush_tiles;                                                                                      \
				/* (a raw ring holds the tile before the previous one, filtered during the previous step) */                    \
				flush_queue<Cfg::QDEPTH, FLUSH_BATCH>(lq0, qcnt[0], seg0, ncand[0], (uint32_t)p.capg, (uint32_t)p.I, tau[0], item0_pp); \
			}                                                                                                                   \
			stagger1_tile<KP, CUR>(aoff8, xb[0], ACC, ACCP, tau_prev, item0_prev, lq0, qcnt[0], J < dense_end || every_tile);   \
			tau_prev = tau[0]; item0_pp = item0_prev; item0_prev = (uint32_t)J * TILE_I + 4 * h;                                \
			TILE_STEP_TAIL(false, )                                                                                             \
			t_prev = J;                                                                                                         \
		} while (0)
		bool last_in_a = false;  // (uniform) which accumulator holds the last tile
		while (t_cur >= 0) {
			STAGGER1_STEP(0, accA, accB);
			last_in_a = true;
			if (t_cur < 0) break;
			STAGGER1_STEP(1, accB, accA);
			last_in_a = false;
		}
#undef STAGGER1_STEP
		flush_queue<Cfg::QDEPTH, FLUSH_BATCH>(lq0, qcnt[0], seg0, ncand[0], (uint32_t)p.capg, (uint32_t)p.I, tau[0], item0_pp);
		if (last_in_a) {  // drain: the last tile (its ring was just drained: the raw path is exact in every split)
#pragma unroll
			for (int e = 0; e < 16; ++e) filter_one<Cfg::QDEPTH>(accA[e], e, tau_prev, item0_prev, lq0, qcnt[0]);
			mark_wrapped_raw<Cfg::QDEPTH>(accA, lq0, qcnt[0]);
		} else {
#pragma unroll
			for (int e = 0; e < 16; ++e) filter_one<Cfg::QDEPTH>(accB[e], e, tau_prev, item0_prev, lq0, qcnt[0]);
			mark_wrapped_raw<Cfg::QDEPTH>(accB, lq0, qcnt[0]);
		}
		last_item0 = item0_prev;
	}

#pragma unroll
	for (int t = 0; t < QT; ++t) {
		flush_queue<Cfg::QDEPTH, FLUSH_BATCH>(lq0 + t * Cfg::QDEPTH * 2048, qcnt[t], seg0 + t * seg_dt, ncand[t], (uint32_t)p.capg, (uint32_t)p.I, tau[t], last_item0);
		if (qv[t] < p.Q) p.seg_cnt[qv[t] * p.nseg + h * p.S + split] = ncand[t];
	}
}
