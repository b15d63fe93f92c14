// The tile schedule of the sweep kernels (score_sweep_kernel, score16_kernel, scoreq16_kernel), once: which item tile a workgroup sweeps next.
// Included by score_fused.hip behind sweep_common.hpp.
//
// All of it is wave-uniform scalars.  Static: tiles j_begin, j_begin + step, ... below j_end (a contiguous or an interleaved share).
// Dynamic (p.chunk_tiles > 0; of the 32x32x16 bodies the two-sub-tile one only): the workgroups of a query row block draw chunks of p.chunk_tiles consecutive
// tiles from the row block's ticket counter, one chunk ahead of the one they sweep.  Why: the 480 workgroups of a cfg2 stage do not run at one speed --
// in-kernel stamps (round 2) put the ends of their tile loops between 193 and 271 us (median 234) for equal shares: 32 CUs hold one
// workgroup instead of two, the others differ by XCD / CU placement -- and a launch lasts as long as its slowest workgroup.  With tickets
// a fast workgroup simply sweeps more chunks.  Any assignment is exact: a workgroup's survivors go to its own segments whatever tiles
// it swept; the repair path finds a split's tiles in p.chunk_owner.  Thread 0 draws a ticket when the workgroup starts the chunk
// BEFORE the one the ticket is for (atomic in flight during a whole tile), hands it over through LDS at that tile's barrier.
// The one-sub-tile 32x32x16 bodies run the same step with `dyn` constant-false: static shares, the ticket statements compile out (Kp = 512
// has no LDS left for the ticket words, see FusedCfg).
//
// The statements are macros, not functions over a state struct: as functions they changed the tile loops they were inlined into (register
// allocation behind the first MFMA of scoreq16_kernel<512>); as text they compile to what each kernel had written out.  A kernel uses
//   TILE_SCHEDULE_BEGIN   once, in front of the first tile's DMA: declares the state and, dynamic, draws the first chunk and the look-ahead;
//   TILE_STEP_HEAD / TILE_STEP_TAIL   around the drain and the tile function of every step, inside one scope.
// They expect in scope: p (FusedParams), tid, rb, split, j_begin, j_end and -- for the DMA of the next tile -- lds_base, wave_u, dma_off
// (tile_dma_offsets).  What differs between the bodies is an argument:
//   CHUNK_TILE(c)  first tile of chunk id c: TILE_OF_CHUNK, or TILE_OF_CHUNK_ROT where the sampled chunks come last (score16.hpp);
//   SLICED         whether the tickets are XCD-sliced (below): p.sliced, or a literal false for the 32x32x16 body;
//   T_STEP         distance between two tiles of a static share (the interleaved shares of the 32x32x16 body; 1 once tickets are drawn);
//   ON_CROSSED     a statement for the step in which the next chunk is opened (score16_kernel: the first sampled chunk), or nothing.
// The counter a ticket is drawn from is ctr_rb + slice: the row block's counter, or its counter of the slice this workgroup draws from.
#pragma once

// ---- XCD-sliced tickets (round 4).  Under round 3's schedule a row block's workgroups -- spread over all eight XCDs -- drew their chunks from
// ONE counter per row block: every XCD ended up reading every tile of the stage (cfg4's per-GPU shape: 8.9 GB of L2 -> fabric traffic per
// launch against 1.0 GB of E^T, 5.3 TB/s).  Now the stage's chunks are cut into eight contiguous slices, one per XCD, each with its own
// counter per row block: a workgroup draws from the slice of the XCD it RUNS on (s_getreg XCC_ID -- measured, never assumed: placement is
// speed only) and, once that slice is exhausted, steals from the following ones.  All the row blocks resident on an XCD walk the same
// slice at about the same pace, so a tile crosses the fabric about once (plus the steals) instead of once per XCD, and the schedule
// stays dynamic: a slow workgroup still draws fewer chunks, a fast one moves on to help its neighbours.  Any assignment is exact
// (chunk ids stay global: the owner map and the repair path are unchanged).
constexpr int N_SLICES = 8;
__device__ __forceinline__ uint32_t slice_len(int n_chunks, int cps, int s) {
	const int b = s * cps, e = min(b + cps, n_chunks);
	return e > b ? (uint32_t)(e - b) : 0u;
}
// local ticket `l` drawn from slice `slice` of this row block -> global chunk id, or n_chunks when every slice is exhausted.  Steals (a
// blocking atomic per exhausted slice, at most seven per workgroup and stage) happen here; `tried` = slices this workgroup found exhausted.
__device__ __forceinline__ uint32_t slice_resolve(uint32_t l, uint32_t *ctr_rb, int n_chunks, int cps, int &slice, int &tried) {
	for (;;) {
		if (l < slice_len(n_chunks, cps, slice)) return (uint32_t)(slice * cps) + l;
		if (++tried >= N_SLICES) return (uint32_t)n_chunks;
		slice = (slice + 1) & (N_SLICES - 1);
		l = atomicAdd(ctr_rb + slice, 1u);
	}
}
__device__ __forceinline__ int xcc_id() {
	uint32_t x = 0;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
#endif
	return (int)(x & (N_SLICES - 1));
}

// first tile of chunk id c (uniform): chunk id = position, or rotated so that the sampled chunks are the last ids (chunk_pos)
#define TILE_OF_CHUNK(c) (p.tile_begin + (int)(c) * p.chunk_tiles)
#define TILE_OF_CHUNK_ROT(c) (p.tile_begin + chunk_pos((int)(c), p.chunk_rot, p.n_chunks) * p.chunk_tiles)

// State, and the ticket prologue: thread 0 draws the first chunk and the look-ahead and hands both to the workgroup through LDS.
// TICKET_WORDS: LDS byte address of the body's four ticket words (16-byte aligned).  The first two are used in turn by the steps: a ticket is
// published at the end of one step and read at the head of the next, and nothing but program order separates that read from the NEXT
// publication (possible one step later when a chunk is a single tile).
#define TILE_SCHEDULE_BEGIN(DYN, SLICED, TICKET_WORDS, CHUNK_TILE)                                                              \
	int t_cur = j_begin < j_end ? j_begin : -1, t_cend = j_end, t_next_chunk = -1;                                              \
	bool ticket_pending = false;                                                                                                \
	const bool dyn = (DYN);                                                                                                     \
	uint32_t ticket_slot = (TICKET_WORDS);                                                                                      \
	/* thread 0's slice state; unsliced = one counter per row block as in round 3 */                                            \
	uint32_t *const ctr_rb = p.chunk_ctr + ((SLICED) ? (size_t)rb * N_SLICES : (size_t)rb);                                     \
	int slice = (SLICED) ? xcc_id() : 0, tried = 0;                                                                             \
	if (dyn) {                                                                                                                  \
		if (tid == 0) {                                                                                                         \
			uint32_t c0, c1;                                                                                                    \
			if (SLICED) {                                                                                                       \
				c0 = slice_resolve(atomicAdd(ctr_rb + slice, 1u), ctr_rb, p.n_chunks, p.chunks_per_slice, slice, tried);        \
				c1 = c0 < (uint32_t)p.n_chunks ? slice_resolve(atomicAdd(ctr_rb + slice, 1u), ctr_rb, p.n_chunks, p.chunks_per_slice, slice, tried) : (uint32_t)p.n_chunks; \
			} else {                                                                                                            \
				c0 = atomicAdd(ctr_rb, 2u); c1 = c0 + 1u;                                                                       \
			}                                                                                                                   \
			if (p.chunk_owner) {                                                                                                \
				if (c0 < (uint32_t)p.n_chunks) p.chunk_owner[(int64_t)rb * p.n_chunks + c0] = (uint8_t)split;                   \
				if (c1 < (uint32_t)p.n_chunks) p.chunk_owner[(int64_t)rb * p.n_chunks + c1] = (uint8_t)split;                   \
			}                                                                                                                   \
			lds_write_u32(ticket_slot + 8u, c0);   /* (the prologue's pair sits in the third and fourth ticket word) */         \
			lds_write_u32(ticket_slot + 12u, c1);                                                                               \
			__builtin_amdgcn_s_waitcnt(0xC07F);  /* lgkmcnt(0): the words are in LDS before this wave reaches the barrier */    \
		}                                                                                                                       \
		__syncthreads();                                                                                                        \
		const uint32_t c = lds_load_u32_uniform(ticket_slot + 8u), c1 = lds_load_u32_uniform(ticket_slot + 12u);                \
		t_cur = c < (uint32_t)p.n_chunks ? CHUNK_TILE(c) : -1;                                                                  \
		t_cend = min(t_cur + p.chunk_tiles, p.tile_end);                                                                        \
		t_next_chunk = c1 < (uint32_t)p.n_chunks ? CHUNK_TILE(c1) : -1;                                                         \
	}

// One step of the schedule, around a body's drain and tile function: (head) read the pending ticket, pick the next tile, issue its DMA into
// the other buffer, draw the ticket of the chunk after the one that tile opens; (tail) wait, publish the ticket, barrier, advance.
// Declares J (this step's tile), nx (the next one, -1: none), crossed, ticket.
#define TILE_STEP_HEAD(KP, CUR, CHUNK_TILE, T_STEP)                                                                             \
	const int J = t_cur;                                                                                                        \
	if (ticket_pending) {  /* (uniform) the ticket thread 0 drew during the previous step */                                    \
		const uint32_t c = lds_load_u32_uniform(ticket_slot);                                                                   \
		t_next_chunk = c < (uint32_t)p.n_chunks ? CHUNK_TILE(c) : -1;                                                           \
		ticket_pending = false;                                                                                                 \
		ticket_slot ^= 4u;  /* (the ticket words are 16-byte aligned) */                                                        \
	}                                                                                                                           \
	int nx = J + (T_STEP);                                                                                                      \
	bool crossed = false;  /* (uniform) the next tile opens the look-ahead chunk: draw the ticket of the one after it */        \
	if (nx >= t_cend) { nx = t_next_chunk; crossed = dyn && nx >= 0; }                                                          \
	if (nx >= 0) tile_dma_s<KP>(p.Et, nx, lds_base + ((CUR) ^ 1) * FusedCfg<KP>::TILE_BYTES, wave_u, dma_off);                  \
	uint32_t ticket = 0;                                                                                                        \
	if (crossed && tid == 0) ticket_draw(ticket, ctr_rb + slice);  /* in flight until ticket_wait() below */
#define TILE_STEP_TAIL(SLICED, ON_CROSSED)                                                                                      \
	ticket_wait(ticket);  /* vmcnt(0): the DMA of the next tile, the queue stores issued with it and the ticket have landed */  \
	if (crossed) {                                                                                                              \
		if (tid == 0) {                                                                                                         \
			if (SLICED) ticket = slice_resolve(ticket, ctr_rb, p.n_chunks, p.chunks_per_slice, slice, tried);                   \
			lds_write_u32(ticket_slot, ticket);                                                                                 \
			if (p.chunk_owner && ticket < (uint32_t)p.n_chunks) p.chunk_owner[(int64_t)rb * p.n_chunks + ticket] = (uint8_t)split; \
			__builtin_amdgcn_s_waitcnt(0xC07F);                                                                                 \
		}                                                                                                                       \
		ticket_pending = true;                                                                                                  \
		t_cend = min(nx + p.chunk_tiles, p.tile_end);                                                                           \
		ON_CROSSED                                                                                                              \
	}                                                                                                                           \
	__syncthreads();                                                                                                            \
	t_cur = nx;
