// Prepass on the sweep's MFMA body (Kp <= 256, the plans that run score16_kernel; included by score_fused.hip behind score16.hpp).
//
// The prepass multiplies an 8 % sample of the item tiles with every query and keeps one maximum per group of 16 items; the threshold kernel
// takes the k-th largest of a query's group maxima as tau0.  Until round 6 it ran score_prepass_kernel<KP, 16>: 32x32x16 MFMAs, compiler-placed
// ds_read with lgkmcnt(0) in front of every k-step, one tile ahead.  This kernel is score16_kernel's tile loop minus everything that serves
// candidates: queries as the resident B operand (four 16-query sub-tiles per wave), the tile image and its XOR swizzle, LDS-DMA staging with
// an SGPR base + M0, the five-quad fragment ring with counted waits, v_mfma_f32_16x16x32_bf16.  No queue, no ladder, no tickets: a workgroup
// keeps its static share [split * st_per_split, + st_per_split) of the n_st sample tiles, leading or strided over n_full_tiles.
//
// One body, one value: every accumulator runs the k-steps 0 .. Kp/32 - 1 in the sweep's order on the sweep's operands, from zero, so a group
// maximum is BIT-EQUAL to the score score16_kernel computes for that item (an MFMA's result does not depend on what is issued between two
// links of its chain).  tau0 is therefore the sweep's own score of some sampled item: the case the select's repair used to catch -- tau0 one
// ulp above the sweep's version of the k-th group maximum, k - 1 candidates left -- cannot occur on these plans any more.
//
// What differs from the sweep, and why:
//  * a fragment feeds FOUR MFMAs (all four query sub-tiles) instead of two: no filter has to hide behind half of the chain, so the tile is
//    one pass of K = Kp / 16 fragments (k-step s >> 1, item half s & 1) and eight accumulators (32 VGPRs), half the sweep's LDS reads per flop;
//  * THREE tile buffers, two tiles in flight.  A workgroup runs about twenty tiles, each a 64 Kp-byte block of its own from HBM (the sample is
//    strided: no neighbour has pulled the tile into L2 the way the sweep's row blocks do for each other), and a tile's MFMAs take well under
//    a microsecond: one tile ahead does not cover the load.  Without the sweep's 16 KB of queues the third buffer is free (48 KB at
//    Kp = 256, two workgroups per CU).  Three workgroups per CU were not an option: the queries alone are 128 VGPRs, with accumulators, ring
//    and addresses the kernel needs more than the 168 a third wave per SIMD would leave.
//    The waits are counted -- at the end of a step vmcnt(PIECES) leaves the youngest tile in flight -- and sit in front of the step's gmax
//    stores, so that nothing but the DMA pieces of the step is younger than what must have landed.  The barrier is a raw s_barrier: every
//    wave has waited for its own pieces and its own LDS reads (the tile's last fragment wait is lgkmcnt(0)).
//  * group maxima in registers.  C/D layout: col = lane & 15 = query, row = 4 (lane >> 4) + reg = item of a 16-item half.  The pinned layout
//    gmax[q * n_groups + 2 j + g] wants the 16 rows r of the 32-item tile with (r >> 2) & 1 == g: lane quarters g and g + 2 of both halves.
//    A lane takes the max over its eight registers of a sub-tile; ONE v_permlane32_swap per PAIR of sub-tiles then brings the partner
//    quarter's value of sub-tile 2 i to lanes 0-31 and of sub-tile 2 i + 1 to lanes 32-63: every lane ends with one finished maximum per
//    pair, two stores per lane and tile with all 64 lanes active.
//  * it zeroes the workspace header (zero_ws_header, sweep_common.hpp) like the other prepass.
#pragma once

template <int KP>
struct Prepass16Cfg {
	static constexpr int NBUF = 3;                   // tile buffers: the tile in the MFMAs + two in flight
	static constexpr int KS32 = KP / 32, K = KP / 16, CPR = KP / 8;
	static constexpr int TILE_BYTES = TILE_I * KP * 2;
	static constexpr int PIECES = TILE_BYTES / 1024 / 4;            // DMA pieces per wave and tile
	static constexpr int LDS_BYTES = NBUF * TILE_BYTES;
	static constexpr int BQ = 256;
	static_assert(PIECES >= 1 && K >= 4, "a tile holds a 1 KB piece per wave and at least four fragments per lane");
	static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
};

template <int N>
__device__ __forceinline__ void vm_wait_all_but() {   // counted vmcnt (N is small: the DMA pieces of one tile)
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}

// One 32-item tile against the wave's 64 queries: acc[item half][query sub-tile].  The sweep's ring (stagger16_tile): AR slots, DIST fragments ahead,
// a slot is rewritten two steps (eight MFMAs) after its use.
template <int KP, int CUR>
__device__ __forceinline__ void prepass16_tile(const uint32_t (&aoff)[Prepass16Cfg<KP>::K], const bf16x8 (&xb)[4][Prepass16Cfg<KP>::KS32], f32x4 (&acc)[2][4]) {
	using C = Prepass16Cfg<KP>;
	constexpr int K = C::K, AR = 5, DIST = 3, OFF = CUR * C::TILE_BYTES;
	u32x4 ring[AR];
#pragma unroll
	for (int i = 0; i < DIST; ++i) lds_read_frag<OFF>(ring[i], aoff[i]);
#pragma unroll
	for (int ih = 0; ih < 2; ++ih)
#pragma unroll
		for (int t = 0; t < 4; ++t) acc[ih][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
	for (int g = 0; g < K; ++g) {
		const int nxt = g + DIST;
		if (nxt < K) lds_read_frag<OFF>(ring[nxt % AR], aoff[nxt]);
#if defined(__HIP_DEVICE_COMPILE__)
		if (g >= 1) asm volatile("" ::"v"(ring[(g - 1) % AR]));
#endif
		const int after = K - 1 - g;
		lds_wait_frag(ring[g % AR], after < DIST ? after : DIST);
		const bf16x8 a = __builtin_bit_cast(bf16x8, ring[g % AR]);
		const int ks = g >> 1, ih = g & 1;
#pragma unroll
		for (int t = 0; t < 4; ++t) acc[ih][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xb[t][ks], acc[ih][t], 0, 0, 0);
	}
	// The eight chains end HERE, in eight live accumulators (see mfma_chain_done in score32.hpp).  Left alone, hipcc sank each chain's last
	// MFMA into the epilogue's maxima and gave it a fresh destination that overlapped a neighbour's: MFMAs three and four issue slots apart
	// whose destinations / accumulator inputs overlap without being one in-place chain -- what scripts/check_mfma_hazards.py refuses.
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("s_nop 7\n\ts_nop 2" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
#endif
}

template <int KP>
__global__ __launch_bounds__(256, 2) void prepass16_kernel(const FusedParams p) {
	using C = Prepass16Cfg<KP>;
	constexpr int K = C::K, KS32 = C::KS32, CPR = C::CPR;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int c16 = lane & 15, g4 = lane >> 4;
	zero_ws_header(p);
	const int wid = xcd_remap(blockIdx.x, p.n_wg);
	const int n_rb = (int)((p.Q + C::BQ - 1) / C::BQ);
	const int split = wid / n_rb, rb = wid - split * n_rb;
	const int wave_u = __builtin_amdgcn_readfirstlane(wave);
	const uint32_t lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr(smem));

	// ---- this workgroup's sample tiles j_begin .. j_end - 1; sample tile j = item tile j (leading) or floor(j * n_full_tiles / n_st) (strided),
	// walked incrementally in fetch order (all uniform): tile += dq, rem += dr, carry
	const int j_begin = split * p.st_per_split, j_end = min(j_begin + p.st_per_split, p.n_st);
	int f_tile, f_rem = 0, dq = 1, dr = 0;
	if (p.sample_leading) f_tile = j_begin;
	else {
		const int64_t x = (int64_t)j_begin * p.n_full_tiles;
		f_tile = (int)(x / p.n_st); f_rem = (int)(x % p.n_st);
		dq = p.n_full_tiles / p.n_st; dr = p.n_full_tiles % p.n_st;
	}
	int j_dma = j_begin;   // the next sample tile to fetch
	uint32_t dma_off[C::PIECES];
	tile_dma_offsets<KP>(dma_off, wave_u, lane);
	auto fetch = [&](int buf) {
		tile_dma_s<KP>(p.Et, f_tile, lds_base + (uint32_t)(buf * C::TILE_BYTES), wave_u, dma_off);
		f_tile += dq; f_rem += dr;
		if (f_rem >= p.n_st) { f_rem -= p.n_st; ++f_tile; }
		++j_dma;
	};
	if (j_dma < j_end) fetch(0);   // in flight beside the query loads

	// ---- this lane's four queries: B operand fragments, resident for the whole kernel.  B[k = 8 (lane >> 4) + j][col = lane & 15]
	bf16x8 xb[4][KS32];
	const int64_t q_wave0 = (int64_t)rb * C::BQ + wave_u * 64;
#pragma unroll
	for (int t = 0; t < 4; ++t) LOAD_QUERIES16(q_wave0 + 16 * t + c16, g4, xb[t]);
	__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the queries and the first tile (see score_sweep_kernel)
	if (j_dma < j_end) fetch(1);
	__builtin_amdgcn_s_barrier();

	// after the maxima's half exchange (below) lane l holds group (l >> 4) & 1 of query sub-tile 2 i + (l >> 5), i = 0, 1
	const int64_t q_st = q_wave0 + 16 * (lane >> 5) + c16;
	const bool st_ok0 = q_st < p.Q, st_ok1 = q_st + 32 < p.Q;
	float *const gdst = p.gmax + (st_ok0 ? q_st : 0) * p.n_groups + (g4 & 1);
	const int64_t gdst_pair = (int64_t)32 * p.n_groups;
	// A fragment of step s = (k-step s >> 1, item half s & 1): row 16 (s & 1) + (lane & 15), 16-byte chunk 4 (s >> 1) + (lane >> 4)
	uint32_t aoff[K];
#pragma unroll
	for (int s = 0; s < K; ++s) {
		const int row = 16 * (s & 1) + c16;
		aoff[s] = lds_addr(smem) + (uint32_t)(row * CPR + swz<CPR>(row, 4 * (s >> 1) + g4)) * 16u;
	}
	__builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): prepass16_tile() counts LDS reads

#define PRE16_STEP(CUR)                                                                                                         \
	do {                                                                                                                        \
		const bool ahead = j_dma < j_end;   /* (uniform) */                                                                     \
		if (ahead) fetch(((CUR) + 2) % C::NBUF);   /* the buffer of the previous step: every wave is past that step's barrier */ \
		f32x4 acc[2][4];                                                                                                        \
		prepass16_tile<KP, CUR>(aoff, xb, acc);                                                                                 \
		float m[4];                                                                                                             \
		_Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                         \
			const f32x4 a0 = acc[0][t], a1 = acc[1][t];                                                                         \
			m[t] = fmaxf(fmaxf(fmaxf(a0[0], a0[1]), fmaxf(a0[2], a0[3])), fmaxf(fmaxf(a1[0], a1[1]), fmaxf(a1[2], a1[3])));     \
		}                                                                                                                       \
		const auto s01 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m[0]), __float_as_uint(m[1]), false, false);          \
		const auto s23 = __builtin_amdgcn_permlane32_swap(__float_as_uint(m[2]), __float_as_uint(m[3]), false, false);          \
		const float v01 = fmaxf(__uint_as_float(s01[0]), __uint_as_float(s01[1]));                                              \
		const float v23 = fmaxf(__uint_as_float(s23[0]), __uint_as_float(s23[1]));                                              \
		/* the next tile has landed (this wave's pieces; the fetch of this step may stay in flight) */                         \
		if (ahead) vm_wait_all_but<C::PIECES>(); else vm_wait_all_but<0>();                                                     \
		if (st_ok0) gdst[2 * (int64_t)j] = v01;                                                                                 \
		if (st_ok1) gdst[gdst_pair + 2 * (int64_t)j] = v23;                                                                     \
		__builtin_amdgcn_s_barrier();                                                                                           \
		++j;                                                                                                                    \
	} while (0)
	ANNCUR_PAD_HERE();
	int j = j_begin;
	while (j < j_end) {
		PRE16_STEP(0);
		if (j >= j_end) break;
		PRE16_STEP(1);
		if (j >= j_end) break;
		PRE16_STEP(2);
	}
#undef PRE16_STEP
}
