// Approximation error on the sweep's 32x32x16 MFMA loop (included by score_fused.hip): error_lds_kernel, error_kernel.
#pragma once

// ------------------------------------------------------------------ a11: approximation error on the same MFMA loop
// err_sq[q] += sum_i (S_hat[q,i] - A[q,i])^2, norm_sq[q] += sum_i A[q,i]^2 over this workgroup's item tiles; S_hat is never
// written.  Same orientation as the sweep: lane = query, so both sums are lane-local accumulators and the exact matrix is read
// as 4 consecutive items (8 or 16 bytes) per lane and accumulator register group; the next tile's exact values are in flight
// during the MFMAs.  One atomicAdd pair per lane at the end (2 S per query).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4n __attribute__((ext_vector_type(4)));
template <typename TA> struct ExactQuad;  // four consecutive items of one row of the exact matrix (native vectors: asm operands)
template <> struct ExactQuad<uint16_t> {
	u32x2 w;
	__device__ __forceinline__ void load(const uint16_t *p) { w = *reinterpret_cast<const u32x2 *>(p); }
	__device__ __forceinline__ float get(int c) const {
		const uint32_t x = (c & 2) ? w[1] : w[0];
		return __uint_as_float((c & 1) ? (x & 0xffff0000u) : (x << 16));
	}
};
template <> struct ExactQuad<float> {
	f32x4n w;
	__device__ __forceinline__ void load(const float *p) { w = *reinterpret_cast<const f32x4n *>(p); }
	__device__ __forceinline__ float get(int c) const { return w[c]; }
};

// The tile's MFMA chains with the A fragments through the counted-wait register ring of the sweep (three k-steps ahead, inline-asm
// ds_read_b128, s_waitcnt lgkmcnt(n)): round 2's loop read two k-steps, waited lgkmcnt(0), issued four MFMAs -- eight exposed LDS
// round trips per tile (0.24 of peak).  Both sub-tiles share the fragment.
template <int KP, int CUR>
__device__ __forceinline__ void error_mfma_tile(const uint32_t (&aoff)[FusedCfg<KP>::NAOFF], const bf16x8 (&xb)[FusedCfg<KP>::QT][FusedCfg<KP>::KSTEPS],
												 f32x16 (&acc)[FusedCfg<KP>::QT]) {
	using Cfg = FusedCfg<KP>;
	constexpr int K = Cfg::KSTEPS, NA = Cfg::NAOFF, QT = Cfg::QT, AR = 5, DIST = 3, OFF = CUR * Cfg::TILE_BYTES;
	static_assert(K > DIST, "at least four k-steps");
	u32x4 ring[AR];
#define ER_READ(slot, s) lds_read_frag_at(ring[slot], aoff[(s) % NA], OFF + ((s) / NA) * 256)
	ER_READ(0, 0); ER_READ(1, 1); ER_READ(2, 2);
#pragma unroll
	for (int t = 0; t < QT; ++t)
#pragma unroll
		for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
	for (int g = 0; g < K; ++g) {
		const int nxt = g + DIST;
		if (nxt < K) ER_READ(nxt % AR, nxt);
#if defined(__HIP_DEVICE_COMPILE__)
		if (g >= 1) asm volatile("" ::"v"(ring[(g - 1) % AR]));
#endif
		const int after = K - 1 - g;
		lds_wait_frag(ring[g % AR], after < DIST ? after : DIST);
		const bf16x8 a = __builtin_bit_cast(bf16x8, ring[g % AR]);
#pragma unroll
		for (int t = 0; t < QT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[t][g], acc[t], 0, 0, 0);
	}
#undef ER_READ
#pragma unroll
	for (int t = 0; t < QT; ++t) mfma_chain_done(acc[t]);
}

// a11 with the exact matrix staged through LDS (bf16 exact matrix, rows 16-byte aligned: lda % 8 == 0).  error_kernel reads the exact
// values with the accumulator's orientation -- lane = query -- i.e. 8 bytes per lane from 32 different rows per load instruction:
// 2.5 TB/s of exact matrix at cfg2 size whatever the MFMA loop does (round 3: the counted-wait fragment ring alone moved 0.84 -> 0.81 ms;
// the time did not scale with Kp either: 0.60 ms at Kp = 128).  Here the workgroup's tile of the exact matrix -- BQ rows x 64 bytes --
// comes in by the same direct-to-LDS loads as the item tile (16 bytes per lane, four lanes per row, 16 rows per instruction), double
// buffered, one tile ahead; the lanes then read their four quads per sub-tile from LDS (ds_read_b64; the 16-byte chunk of a row is
// XOR-swizzled with (row >> 2) & 3 on the DMA's source address: two-way bank conflicts instead of eight-way).
// (The sweep's stagger with the sums in the filter's place -- sub-tile 0's sums in the shadow of sub-tile 1's chain -- was built and
//  measured: no gain at Kp = 128 (0.460 vs 0.459 ms), 16 spilled registers at Kp = 256 (1.28 ms): the epilogue is not what bounds it.)
template <int KP>
__global__ __launch_bounds__(256, 2) void error_lds_kernel(const FusedParams p, const uint16_t *__restrict__ Aex, int64_t lda,
															float *__restrict__ err_sq, float *__restrict__ norm_sq) {
	using Cfg = FusedCfg<KP>;
	constexpr int KSTEPS = Cfg::KSTEPS, QT = Cfg::QT, CPR = Cfg::CPR;
	constexpr int ATILE = Cfg::BQ * 64, PA = ATILE / 4096, AOFF = 2 * Cfg::TILE_BYTES;   // exact tile bytes, DMA pieces per wave, LDS offset
	constexpr int NAB = 2;                                                               // exact-tile buffers
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int r = lane & 31, h = lane >> 5;
	const int wid = xcd_remap(blockIdx.x, p.n_wg);
	const int n_rb = (int)((p.Q + Cfg::BQ - 1) / Cfg::BQ);
	const int split = wid / n_rb, rb = wid - split * n_rb;

	bf16x8 xb[QT][KSTEPS];
	int64_t qv[QT];
	uint32_t aread[QT], asw[QT];  // LDS byte address of this lane's row of the exact tile (+ 8 h) in buffer 0; the row's chunk swizzle
#pragma unroll
	for (int t = 0; t < QT; ++t) {
		const int row = wave * 32 * QT + 32 * t + r;
		qv[t] = (int64_t)rb * Cfg::BQ + row;
		aread[t] = lds_addr(smem) + (uint32_t)(AOFF + row * 64 + 8 * h);
		asw[t] = (uint32_t)((row >> 2) & 3) << 4;
		LOAD_QUERIES32(qv[t], h, xb[t]);
	}
	// exact-tile DMA: piece i of this wave fills LDS chunks (wave * PA + i) * 64 + lane: row = chunk >> 2, position = chunk & 3.
	// Source = the row block's base (uniform) + a 32-bit byte offset per piece (a row block spans at most 256 rows of the matrix)
	const unsigned char *abase = reinterpret_cast<const unsigned char *>(Aex + (int64_t)rb * Cfg::BQ * lda);
	uint32_t asrc[PA];
#pragma unroll
	for (int i = 0; i < PA; ++i) {
		const int ch = (wave * PA + i) * 64 + lane, row = ch >> 2, pos = ch & 3;
		const int64_t last = p.Q - 1 - (int64_t)rb * Cfg::BQ;   // rows past Q re-read the last row (their sums are dropped)
		asrc[i] = (uint32_t)(((int64_t)row < last ? (int64_t)row : last) * lda * 2) + (uint32_t)(16 * (pos ^ ((row >> 2) & 3)));
	}
	// both DMAs hand-placed (tile_dma_s: SGPR base, 32-bit lane offsets, M0 from a scalar): the builtin's per-lane 64-bit pointers and LDS
	// destinations cost ~24 VGPRs, which the staggered Kp = 256 body does not have
	const int wave_u = __builtin_amdgcn_readfirstlane(wave);
	const uint32_t lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr(smem));
	uint32_t dma_off[Cfg::TILE_BYTES / 4096];
	tile_dma_offsets<KP>(dma_off, wave_u, lane);
	const int j_begin = split * p.tiles_per_split, j_end = min(j_begin + p.tiles_per_split, p.n_tiles);
	auto adma = [&](int j, int buf) {
		const unsigned char *src = abase + (int64_t)j * (TILE_I * 2);   // (uniform)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
		for (int i = 0; i < PA; ++i) {
			const uint32_t m0v = lds_base + (uint32_t)(AOFF + buf * ATILE + (wave_u * PA + i) * 1024);
			asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(asrc[i]), "s"(src) : "memory", "m0");
		}
#endif
	};
	__builtin_amdgcn_s_waitcnt(0x0F70);  // see score_sweep_kernel: keeps vmcnt(0) out of the tile loop

	float se[QT], sn[QT];
#pragma unroll
	for (int t = 0; t < QT; ++t) { se[t] = 0.f; sn[t] = 0.f; }
	// (Round 4, measured and dropped: the exact tiles TWO tiles ahead in a ring of three buffers -- 80 KB at Kp = 256 -- with a counted vmcnt at
	//  the end of a step.  Same box, warm, round robin: 0.617 vs 0.615 ms at Kp = 256, 0.472 vs 0.468 at Kp = 128.  What the exact tile costs is
	//  not its round trip: with every DMA re-reading one L2-hot tile the kernel takes 0.505 / 0.32 ms, with the same bytes from contiguous
	//  memory 0.59 / 0.40 -- profiles/r04_error_kernel_modes.txt.)
	if (j_begin < j_end) {
		tile_dma_s<KP>(p.Et, j_begin, lds_base, wave_u, dma_off);
		adma(j_begin, 0);
	}
	__builtin_amdgcn_s_waitcnt(0x0F70);
	__syncthreads();
	uint32_t aoff[Cfg::NAOFF];
#pragma unroll
	for (int s = 0; s < Cfg::NAOFF; ++s) aoff[s] = lds_addr(smem) + (uint32_t)(r * CPR + swz<CPR>(r, 2 * s + h)) * 16u;
	__builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): error_mfma_tile() counts LDS reads
	static_assert(PA <= 15, "vmcnt immediate");
#define ERRL_STEP(ECUR, ACUR, J)                                                                                                \
	do {                                                                                                                        \
		if ((J) + 1 < j_end) tile_dma_s<KP>(p.Et, (J) + 1, lds_base + ((ECUR) ^ 1) * Cfg::TILE_BYTES, wave_u, dma_off);         \
		const bool ahead = (J) + NAB - 1 < j_end;   /* (uniform) */                                                             \
		if (ahead) adma((J) + NAB - 1, ((ACUR) + NAB - 1) % NAB);                                                               \
		f32x16 acc[QT];                                                                                                         \
		error_mfma_tile<KP, ECUR>(aoff, xb, acc);                                                                               \
		ExactQuad<uint16_t> ex[QT][4];  /* items 32 j + 8 g + 4 h + {0..3}, g = 0..3, of the lane's query */                   \
		_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                          \
			_Pragma("unroll") for (int g = 0; g < 4; ++g)                                                                       \
				asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(ex[t][g].w) : "v"(aread[t] + (((uint32_t)g << 4) ^ asw[t])), "n"((ACUR) * ATILE)); \
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                      \
		_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                          \
			_Pragma("unroll") for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(ex[t][g].w));                                  \
		_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                          \
			_Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                    \
				const float x = ex[t][e >> 2].get(e & 3);                                                                       \
				const float d = acc[t][e] - x;                                                                                  \
				se[t] = fmaf(d, d, se[t]);                                                                                      \
				sn[t] = fmaf(x, x, sn[t]);                                                                                      \
			}                                                                                                                   \
		/* this wave's parts of the next item tile and of the next exact tile have landed; the barrier orders LDS only */        \
		if (NAB == 3 && ahead) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PA) : "memory");                                        \
		else __builtin_amdgcn_s_waitcnt(0x0F70);                                                                                \
		asm volatile("" ::: "memory");                                                                                          \
		__builtin_amdgcn_s_barrier();                                                                                           \
		asm volatile("" ::: "memory");                                                                                          \
	} while (0)
	for (int j = j_begin; j < j_end; j += 2) {
		ERRL_STEP(0, 0, j);
		if (j + 1 < j_end) ERRL_STEP(1, 1, j + 1);
	}
#undef ERRL_STEP
#pragma unroll
	for (int t = 0; t < QT; ++t)
		if (qv[t] < p.Q) {
			atomicAdd(&err_sq[qv[t]], se[t]);
			atomicAdd(&norm_sq[qv[t]], sn[t]);
		}
}

// Full 32-item tiles only (p.n_tiles = I / 32): the host adds the last I % 32 columns with the strided kernel of gemm.hip.
template <int KP, typename TA>
__global__ __launch_bounds__(256, 2) void error_kernel(const FusedParams p, const TA *__restrict__ Aex, int64_t lda,
														float *__restrict__ err_sq, float *__restrict__ norm_sq) {
	using Cfg = FusedCfg<KP>;
	constexpr int KSTEPS = Cfg::KSTEPS, QT = Cfg::QT, CPR = Cfg::CPR;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int r = lane & 31, h = lane >> 5;
	const int wid = xcd_remap(blockIdx.x, p.n_wg);
	const int n_rb = (int)((p.Q + Cfg::BQ - 1) / Cfg::BQ);
	const int split = wid / n_rb, rb = wid - split * n_rb;

	bf16x8 xb[QT][KSTEPS];
	int64_t qv[QT];
	const TA *rowp[QT];  // this lane's row of the exact matrix, at its half's first item of a tile
#pragma unroll
	for (int t = 0; t < QT; ++t) {
		qv[t] = (int64_t)rb * Cfg::BQ + wave * 32 * QT + 32 * t + r;
		const bool ok = qv[t] < p.Q;
		rowp[t] = Aex + (ok ? qv[t] : 0) * lda + 4 * h;  // rows past Q read row 0 (their sums are dropped)
		LOAD_QUERIES32(qv[t], h, xb[t]);
	}
	__builtin_amdgcn_s_waitcnt(0x0F70);  // see score_sweep_kernel: keeps vmcnt(0) out of the tile loop

	const int j_begin = split * p.tiles_per_split, j_end = min(j_begin + p.tiles_per_split, p.n_tiles);
	float se[QT], sn[QT];
	ExactQuad<TA> ex[QT][4];  // exact values of the tile whose MFMAs run next: items 32 j + 8 g + 4 h + {0..3}, g = 0..3
#pragma unroll
	for (int t = 0; t < QT; ++t) { se[t] = 0.f; sn[t] = 0.f; }
	if (j_begin < j_end) {
		tile_dma<KP>(p.Et, j_begin, smem, wave, lane);
#pragma unroll
		for (int t = 0; t < QT; ++t)
#pragma unroll
			for (int g = 0; g < 4; ++g) ex[t][g].load(rowp[t] + (int64_t)j_begin * TILE_I + 8 * g);
	}
	__builtin_amdgcn_s_waitcnt(0x0F70);
	__syncthreads();
	uint32_t aoff[Cfg::NAOFF];   // LDS byte address of this lane's A fragment of k-step s (< NAOFF) in tile buffer 0 (see stagger_tile)
#pragma unroll
	for (int s = 0; s < Cfg::NAOFF; ++s) aoff[s] = lds_addr(smem) + (uint32_t)(r * CPR + swz<CPR>(r, 2 * s + h)) * 16u;
	__builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): error_mfma_tile() counts LDS reads
#define ERR_STEP(CUR, J)                                                                                                        \
	do {                                                                                                                        \
		const bool more = (J) + 1 < j_end;                                                                                      \
		if (more) tile_dma<KP>(p.Et, (J) + 1, smem + ((CUR) ^ 1) * Cfg::TILE_BYTES, wave, lane);                                \
		f32x16 acc[QT];                                                                                                         \
		error_mfma_tile<KP, CUR>(aoff, xb, acc);                                                                                \
		/* the exact values are consumed HERE, behind the MFMA chain: hipcc otherwise hoists their unpacking to the top of the */ \
		/* iteration and waits vmcnt(0) there -- for them and for the tile DMA it has just issued */                            \
		_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                          \
			_Pragma("unroll") for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(ex[t][g].w));                                  \
		_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                          \
			_Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                    \
				const float x = ex[t][e >> 2].get(e & 3);                                                                       \
				const float d = acc[t][e] - x;                                                                                  \
				se[t] = fmaf(d, d, se[t]);                                                                                      \
				sn[t] = fmaf(x, x, sn[t]);                                                                                      \
			}                                                                                                                   \
		/* the next tile's exact values are requested now and consumed after the next MFMA chain; the wait below covers the */  \
		/* tile DMA only (loads return in order: the QT*4 quads issued after it may still be in flight) */                      \
		if (more) {                                                                                                             \
			/* the quads must be issued AFTER the tile DMA (the counted wait relies on it) and after the sums above have */      \
			/* consumed the previous ones: otherwise hipcc sinks the sums below the loads and renames the destinations */       \
			if (QT == 2) asm volatile("" : "+v"(se[0]), "+v"(sn[0]), "+v"(se[QT - 1]), "+v"(sn[QT - 1])::"memory");             \
			else asm volatile("" : "+v"(se[0]), "+v"(sn[0])::"memory");                                                         \
			_Pragma("unroll") for (int t = 0; t < QT; ++t)                                                                      \
				_Pragma("unroll") for (int g = 0; g < 4; ++g) ex[t][g].load(rowp[t] + (int64_t)((J) + 1) * TILE_I + 8 * g);     \
			__builtin_amdgcn_s_waitcnt(QT == 2 ? 0x0F78 : 0x0F74);  /* vmcnt(8) / vmcnt(4) */                                   \
		}                                                                                                                       \
		/* raw barrier: __syncthreads() carries a release fence for which hipcc waits vmcnt(0), i.e. for the quads just issued. */ \
		/* What the barrier orders here is LDS only: this wave's fragment reads are complete, its part of the DMA has landed. */ \
		asm volatile("" ::: "memory");                                                                                          \
		__builtin_amdgcn_s_barrier();                                                                                           \
		asm volatile("" ::: "memory");                                                                                          \
	} while (0)
	for (int j = j_begin; j < j_end; j += 2) {
		ERR_STEP(0, j);
		if (j + 1 < j_end) ERR_STEP(1, j + 1);
	}
#undef ERR_STEP
#pragma unroll
	for (int t = 0; t < QT; ++t)
		if (qv[t] < p.Q) {
			atomicAdd(&err_sq[qv[t]], se[t]);
			atomicAdd(&norm_sq[qv[t]], sn[t]);
		}
}
