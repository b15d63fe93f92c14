// What every sweep, prepass and error kernel of score_fused.hip shares: the vector types, the tile and workgroup geometry (FusedCfg), the kernel
// parameters, the tile DMA, the inline-asm LDS accessors, the ticket draw, the fragment ring's reads and waits, the load of the resident query operand.
// Included by score_fused.hip inside its anonymous namespace, in front of the kernel bodies.
#pragma once

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;  // native vector: stays in VGPRs (HIP's uint4 struct did not)

constexpr int TILE_I = 32;
constexpr int CHUNK_TILES = 4;   // dynamic tile schedule: tiles per ticket

template <int KP, int QTV = ((KP <= 256) ? 2 : 1)>
struct FusedCfg {
	static constexpr int KSTEPS = KP / 16;
	static constexpr int QT = QTV;                  // 32-query sub-tiles per wave (default: 2 up to Kp = 256, 1 for Kp = 512)
	static constexpr int BQ = 4 * 32 * QT;          // queries per workgroup (4 waves)
	static constexpr int CPR = KP / 8;              // 16-byte chunks per Et row
	static constexpr int TILE_BYTES = TILE_I * KP * 2;
	static constexpr int PASSES = TILE_BYTES / (256 * 16);
	static constexpr int QDEPTH = 8;                 // lane-private LDS hit queue: entries per (lane, sub-tile)
	static constexpr int QUEUE_BYTES = QT * QDEPTH * 256 * 8;
	static constexpr int QUEUE_OFF = (2 * TILE_BYTES + 16383) / 16384 * 16384;  // rings are 16 KiB aligned (filter_one)
	static constexpr int TICKET_OFF = QUEUE_OFF + QUEUE_BYTES;        // two 32-bit words: the chunk tickets thread 0 hands to its workgroup (dynamic tile schedule)
	// (Kp = 512: two 32 KiB tile buffers + 16 KiB of rings are exactly half a CU's LDS -- 16 bytes more and only ONE workgroup fits per CU
	//  (measured: the sweep of cfg4 20 % slower); that body keeps static tile shares and no ticket words.  Tickets are drawn by the
	//  two-sub-tile body only: the one-sub-tile body at Kp = 128 / 256 (ANNCUR_TOPK_QT1) has the words and leaves them alone)
	static constexpr int LDS_BYTES = TICKET_OFF + (KP >= 512 ? 0 : 16);  // the prepass kernel uses only the tile part
	static constexpr int NAOFF = KSTEPS < 8 ? KSTEPS : 8;             // fragment address registers of the staggered sweep (see stagger_tile)
};

template <int CPR>
__host__ __device__ __forceinline__ constexpr int swz(int row, int c) {   // (constexpr: score16.hpp proves its fragment addresses with static_asserts)
	if (CPR >= 16) return c ^ (row & 15);
	return c ^ ((row >> 1) & 7);  // CPR == 8 (Kp = 64): 128-byte rows, two rows per 256-byte bank line
}

struct FusedParams {
	const uint16_t *X; int64_t ldx;
	const uint16_t *Et;
	int64_t Q, I;
	int n_tiles, n_full_tiles;
	int S, tiles_per_split;           // sweep partition of the item tiles (of the current stage)
	int tile_begin, tile_end;         // item-tile range of the current sweep stage
	int tile_step;                    // 1: split s sweeps the contiguous range [tile_begin + s * tiles_per_split, + tiles_per_split);
	                                  // S: split s sweeps tile_begin + s, + S, + 2 S ... (interleaved: see launch_fused)
	int carry;                        // 1: segment counts continue from the previous stage
	int n_st, S0, st_per_split;       // prepass: sample tiles and their partition
	int sample_leading;               // prepass samples the leading n_st tiles instead of a strided sample (ANNCUR_TOPK_LEADING_SAMPLE)
	float *gmax; int n_groups;        // prepass output [Q x n_groups]
	const float *tau; int tau_stride; // threshold per query: tau[q * tau_stride]
	uint2 *cand; uint32_t *seg_cnt; int capg;
	int nseg;                         // candidate segments per query (2 S: 32x32x16 body, lane halves; S: 16x16x32 body)
	int flush_tiles;                  // wave-cooperative queue flush period (tiles)
	int n_wg;                         // grid size (for the XCD remap)
	// dynamic tile schedule of a sweep stage (chunk_tiles > 0): the workgroups of a query row block draw chunks of `chunk_tiles` consecutive
	// tiles from the row block's ticket counter instead of sweeping a fixed share -- see tile_schedule.hpp
	int chunk_tiles, n_chunks;
	uint32_t *chunk_ctr;              // [n row blocks], zero at launch
	uint8_t *chunk_owner;             // [n row blocks x n_chunks]: which item split swept the chunk (the repair path's map)
	int sliced, chunks_per_slice;     // XCD-sliced tickets: chunk_ctr is [row block][N_SLICES], slice s = chunks [s * chunks_per_slice, + chunks_per_slice)
	// score16_kernel, ladder plans with the leading sample: chunk id c covers the tiles of chunk chunk_pos(c, chunk_rot, n_chunks) -- the sampled
	// tiles [tile_begin, sample_end) come LAST and are not counted for the ladder (score16.hpp).  0 / 0: chunk id = position, no sampled tiles
	int chunk_rot, sample_end;
	// threshold ladder of score16_kernel (score16.hpp): levels [n_rb x BQ][LADDER_LEVELS], counter words [n_rb x BQ][4] (zero at launch),
	// the cell each wave raises to the threshold it ended with (initialised to tau0 by the threshold kernel), k
	int ladder_on; uint32_t ladder_k, ladder_mask;   // ladder_mask = period - 1 (a power of two): tiles between two fetches of a wave's counter words
	const float *ladder; uint32_t *ladder_cnt; float *tau_final;
	uint32_t *nfb;                    // workspace word 0 (zero_ws_header)
	uint32_t zero_bytes;              // prepass kernels: workspace bytes [0, zero_bytes) to clear (a multiple of 16; 0: none) -- see zero_ws_header
};

// Where chunk id c of a ticketed sweep lies among the stage's chunks of consecutive tiles: its tiles are those of position (c + rot) mod n_chunks.
// Chunk ids stay what tickets, the owner map and the repair walk index by; only this map from id to tiles is rotated (rot = 0: identity).
// rot = the chunks that hold the prepass' sampled tiles (the chunk that straddles the sample's end counts as sampled): ids n_chunks - rot ..
// n_chunks - 1, the LAST tickets of a row block, cover them.  0 <= c < n_chunks, 0 <= rot < n_chunks.
__host__ __device__ __forceinline__ constexpr int chunk_pos(int c, int rot, int n_chunks) { return c + rot >= n_chunks ? c + rot - n_chunks : c + rot; }

// Contiguous work ids per XCD (blocks b and b+8 share an XCD's L2): speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int n) {
	const int q = n >> 3, r = n & 7, x = b & 7, l = b >> 3;
	return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + l;
}

// The workspace header -- fallback and hard-list counts (bytes 0..255), the sweep stages' ticket counters, the ladder's counter words: everything
// in front of gmax -- must be zero when the sweep starts.  It used to be a hipMemsetAsync in front of the prepass (a fill kernel and a graph node
// of its own, every call); the prepass workgroups clear it instead, grid-strided, 16 bytes per lane (at cfg2 165 KB over 480 x 256 lanes: at most
// one store each).  Nothing reads the range before the threshold kernel's successors: the prepass writes only gmax, the threshold kernel tau and
// the ladder levels; the counts are first touched by the sweep and the select, all behind the prepass on the same stream.
__device__ __forceinline__ void zero_ws_header(const FusedParams &p) {
	typedef __attribute__((ext_vector_type(4))) unsigned int zvec;
	zvec *const dst = reinterpret_cast<zvec *>(p.nfb);   // (the workspace is 256-byte aligned)
	const uint32_t n = p.zero_bytes >> 4;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = (zvec){0u, 0u, 0u, 0u};
}


// One 32-item tile of E^T (contiguous 64*KP bytes in HBM) -> LDS by direct-to-LDS loads (global_load_lds_dwordx4: 1 KiB per
// wave-instruction, LDS destination = wave-uniform base + lane*16, no staging VGPRs, no ds_write).  The bank-conflict
// swizzle is applied on the per-lane SOURCE address (LDS chunk position p holds source chunk (row, c ^ f(row)));
// readers apply the same involution.
template <int KP>
__device__ __forceinline__ void tile_dma(const uint16_t *__restrict__ Et, int tile, unsigned char *buf, int wave, int lane) {
	constexpr int CPR = FusedCfg<KP>::CPR;
	constexpr int PER_WAVE = FusedCfg<KP>::TILE_BYTES / 1024 / 4;
	const unsigned char *src = reinterpret_cast<const unsigned char *>(Et + (int64_t)tile * TILE_I * KP);
#pragma unroll
	for (int i = 0; i < PER_WAVE; ++i) {
		const int piece = wave * PER_WAVE + i;  // wave-uniform
		const int pch = piece * 64 + lane;
		const int row = pch / CPR, cs = pch % CPR;
		const int c = swz<CPR>(row, cs);
		__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + (row * CPR + c) * 16),
										 (__attribute__((address_space(3))) void *)(buf + piece * 1024), 16, 0, 0);
	}
}

// (Round 3 also issued the next tile's pieces BETWEEN the tile's MFMAs instead of in a burst at the head of the step -- the phase stamps
//  charge the burst with 384 of the 2855 cycles of a step -- : no gain, same box, alternating (0.4802 vs 0.4792 ms per sweep): the partner
//  wave's MFMAs cover the burst already.)
// The same DMA for the staggered sweep, hand-placed: hipcc kept the four per-lane source offsets as 64-bit pairs plus four VGPRs of LDS
// destinations that it then moved to M0 through v_readfirstlane (12 VGPRs and ~20 vector instructions per tile and wave in a kernel
// that sits at the 256-register limit).  Here: one 32-bit offset register per piece (computed once), the tile's base in SGPRs
// (saddr form), M0 from a scalar.  voff[i] = byte offset of this lane's 16 bytes of piece i inside a tile (swizzle on the source).
template <int KP>
__device__ __forceinline__ void tile_dma_offsets(uint32_t (&voff)[FusedCfg<KP>::TILE_BYTES / 4096], int wave_u, int lane) {
	constexpr int CPR = FusedCfg<KP>::CPR, PER_WAVE = FusedCfg<KP>::TILE_BYTES / 4096;
#pragma unroll
	for (int i = 0; i < PER_WAVE; ++i) {
		const int pch = (wave_u * PER_WAVE + i) * 64 + lane;
		const int row = pch / CPR, cs = pch % CPR;
		voff[i] = (uint32_t)(row * CPR + swz<CPR>(row, cs)) * 16u;
	}
}
template <int KP>
__device__ __forceinline__ void tile_dma_s(const uint16_t *__restrict__ Et, int tile, uint32_t lds_buf, int wave_u,
											const uint32_t (&voff)[FusedCfg<KP>::TILE_BYTES / 4096]) {
	constexpr int PER_WAVE = FusedCfg<KP>::TILE_BYTES / 4096;
	const unsigned char *src = reinterpret_cast<const unsigned char *>(Et) + (int64_t)tile * FusedCfg<KP>::TILE_BYTES;  // (uniform)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
	for (int i = 0; i < PER_WAVE; ++i) {
		const uint32_t m0v = lds_buf + (uint32_t)(wave_u * PER_WAVE + i) * 1024u;  // (uniform) LDS destination of the piece: M0 + lane * 16
		asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0v), "v"(voff[i]), "s"(src) : "memory", "m0");
	}
#endif
}

// Threshold filter of one 32x32 accumulator tile: lane = query, register e = item row (e & 3) + 8 (e >> 2) (+ 4 h in item0).
// Survivors go to the lane's private LDS queue (slot i of lane tid at lq[i * 256]: conflict-free, no atomics); the queues
// are drained to the lane's HBM candidate segment by flush_queue() every FLUSH_TILES tiles with ONE store instruction per
// queue slot for the whole wave (a store per hit made the kernel store-issue bound: ~20 sparse stores per tile per wave).
// The queue's LDS accesses are inline asm: with a direct-to-LDS load in flight hipcc cannot prove that an ordinary LDS
// store does not alias the DMA destination and puts s_waitcnt vmcnt(0) in front of EVERY push (measured: it serialised the
// pushes behind the next tile's DMA and the flush stores).  The queue region is disjoint from the tile buffers; LDS
// executes one wave's instructions in order, so a slot written by ds_write_b64 is seen by the later ds_read_b64.
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
	return (uint32_t)(size_t)(__attribute__((address_space(3))) const char *)p;
}
__device__ __forceinline__ void lds_write_u64(uint32_t addr, uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
	const unsigned long long d = ((unsigned long long)hi << 32) | lo;
	asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(d) : "memory");
#endif
}
__device__ __forceinline__ uint2 lds_load_u64(uint32_t addr) {
	unsigned long long d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(d) : "v"(addr) : "memory");
#endif
	return make_uint2((uint32_t)d, (uint32_t)(d >> 32));
}

__device__ __forceinline__ void lds_write_u32(uint32_t addr, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
#endif
}
__device__ __forceinline__ uint32_t lds_load_u32_uniform(uint32_t addr) {  // every lane reads the same word; returned as a scalar
	uint32_t d = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(d) : "v"(addr) : "memory");
#endif
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
}
// Ticket draw of the dynamic tile schedule: a RETURNING atomic add whose result is not waited for where it is issued.  (Written with
// atomicAdd() hipcc's atomic optimiser turns the one-lane add into a wave-aggregated one and waits vmcnt(0) for it on the spot --
// directly behind the next tile's DMA.)  The destination is in flight after the asm statement, like the fragment ring's registers:
// ticket_wait() is the wait, and takes the register as an in/out operand so that nothing that reads it can be scheduled above it.
__device__ __forceinline__ void ticket_draw(uint32_t &ticket, uint32_t *ctr) {
#if defined(__HIP_DEVICE_COMPILE__)
	const uint32_t one = 1u;
	asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(ticket) : "v"(ctr), "v"(one) : "memory");
#endif
}
__device__ __forceinline__ void ticket_wait(uint32_t &ticket) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("s_waitcnt vmcnt(0)" : "+v"(ticket)::"memory");
#endif
}
// Two dwords from two separate VGPRs (no 64-bit register pair has to be assembled in the hit path).
__device__ __forceinline__ void lds_write_2x32(uint32_t addr, uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" ::"v"(addr), "v"(lo), "v"(hi) : "memory");
#endif
}

// ---- A-fragment ring of the staggered sweep.  The LDS reads are inline asm with explicit, COUNTED s_waitcnt lgkmcnt(n):
// hipcc's own wait insertion fell back to lgkmcnt(0) in this loop (every fourth MFMA waited for a fragment requested one
// MFMA earlier).  The compiler does not see that the destination is still in flight after the asm statement; the wait
// statement takes the fragment as an in/out operand so that its consumer cannot be scheduled above the wait.
template <int OFF>
__device__ __forceinline__ void lds_read_frag(u32x4 &dst, uint32_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
#endif
}
__device__ __forceinline__ void lds_read_frag_at(u32x4 &dst, uint32_t addr, int off) {  // `off` folds to an immediate after unrolling
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off));
#endif
}
__device__ __forceinline__ void lds_wait_frag(u32x4 &frag, int pending) {  // `pending` folds to a constant after unrolling
#if defined(__HIP_DEVICE_COMPILE__)
	if (pending >= 3) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(frag));
	else if (pending == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(frag));
	else if (pending == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(frag));
	else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(frag));
#endif
}

// ---- The resident query operand: query q's B fragments of all k-steps, for one sub-tile of the lane, into xb[k-steps] (zeros for a row past Q:
// its scores are dropped by a threshold of +inf and a count of PAD_ROW_COUNT).  Per k-step the lane takes 16 bytes of the row's 32 (32x32x16:
// k = 8 h + j, h = lane >> 5) or of its 64 (16x16x32: k = 8 g4 + j, g4 = lane >> 4).  Expects p (FusedParams) in scope.
// Macros: written as functions the loads compiled to other code (shorter, with a different schedule of the tile loops of the error kernels).
#define LOAD_QUERIES_(q_, part_, xb_, PARTS)                                                                                    \
	do {                                                                                                                        \
		const bool ok = (q_) < p.Q;                                                                                             \
		const u32x4 *src = reinterpret_cast<const u32x4 *>(p.X + (ok ? (q_) : 0) * p.ldx) + (part_);                            \
		_Pragma("unroll") for (int s = 0; s < (int)(sizeof(xb_) / sizeof((xb_)[0])); ++s) {                                     \
			const u32x4 zero = {0u, 0u, 0u, 0u};                                                                                \
			const u32x4 w = ok ? src[(PARTS) * s] : zero;                                                                       \
			(xb_)[s] = __builtin_bit_cast(bf16x8, w);                                                                           \
		}                                                                                                                       \
	} while (0)
#define LOAD_QUERIES32(q_, h_, xb_) LOAD_QUERIES_(q_, h_, xb_, 2)
#define LOAD_QUERIES16(q_, g4_, xb_) LOAD_QUERIES_(q_, g4_, xb_, 4)
