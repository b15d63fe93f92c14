// Fused S_hat = X . E  +  per-query top-k for gfx950; S_hat is never written to HBM.
//
// Orientation: the MFMA computes S_hat^T tiles, D[item][query] = sum_k Et[item][k] * X[query][k]
// (v_mfma_f32_32x32x16_bf16, A operand = 32 item rows of E^T from LDS, B operand = the wave's
// queries, resident in registers for the whole kernel).  In the C/D layout the query sits on the
// LANE (col = lane & 31) and the 16 accumulator registers are 16 items, so a query's threshold is
// one lane-local VGPR and the filter is one v_cmp per output element.
//
// Data layout in HBM
//   X   [Q  x Kp] bf16 row-major   queries' scores against the anchor items (C_q), K zero-padded to Kp
//   Et  [Ip x Kp] bf16 row-major   item embeddings E^T (= (U R)^T), Ip = 32-multiple, zero rows past I
//   one 32-item tile of Et is ONE contiguous 64*Kp-byte block -> 16-byte coalesced loads.
// LDS: the tile is stored row-major with the 16-byte chunk index XOR-swizzled by the row so the
// per-k-step ds_read_b128 (32 rows x one chunk column) is bank-conflict free.
//
// Launches (all on the caller's stream):
//   1. prepass   : group maxima of S_hat over a strided sample of item tiles  -> gmax[Q x G]
//   2. threshold : tau[q] = k-th largest group maximum (wave-per-query radix select) -> a lower bound on the
//                  k-th best score of the query (k distinct groups each hold an element >= tau)
//   3. sweep     : all tiles, in 1-3 stages (plan_fused picks the split); every S_hat[q,i] >= tau[q] goes through the
//                  lane's private LDS ring to the lane's private candidate segment in HBM (no atomics); between stages
//                  a wave-per-query kernel raises tau[q] to the k-th best candidate collected so far
//   4. select    : per query, exact top-k of its candidates (wave-level selector; workgroup-level kernel for k > 128).
//                  A segment that overflowed or whose ring wrapped is repaired by recomputing only the item tiles its
//                  split swept; nothing leaves the call inexact.
// Algorithmic work: 2*Q*Kp*I flops in (3) (+ sample fraction in (1)).
#include <stdlib.h>
#include <math.h>
#include <type_traits>
// scripts/placement_sweep.sh builds the library with ANNCUR_PLACEMENT_PAD = 1..n: that many extra instructions in front of every
// sweep loop move the loops through all alignments relative to the instruction-fetch lines.  A result that changes with the pad is a
// missing wait state somewhere (DESIGN.md 4.1 'A latent hazard'); the shipped build has no pad.
#ifdef ANNCUR_PLACEMENT_PAD
#define ANNCUR_PAD_HERE() asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(ANNCUR_PLACEMENT_PAD) : "memory")
#else
#define ANNCUR_PAD_HERE() do { } while (0)
#endif
#include "select.hpp"
#include "wave_select.hpp"
#include "select_stream.hpp"

using namespace anncur;

namespace {

// The kernels, one header per body, in the order their definitions have always had in this translation unit.  This file keeps the plan,
// the launchers and the C entry points.
#include "sweep_common.hpp"    // types, FusedCfg, FusedParams, tile DMA, LDS accessors, fragment ring, query operand load
#include "tile_schedule.hpp"   // the dynamic tile schedule (tickets, XCD slices), once for the three sweep kernels
#include "score32.hpp"         // 32x32x16 bodies: per-lane rings, score_prepass_kernel, score_sweep_kernel
#include "score16.hpp"         // 16x16x32 sweep (Kp <= 256): WaveQueue, threshold ladder, score16_kernel
#include "prepass16.hpp"       // prepass on that body
#include "score_q16.hpp"       // 16x16x32 sweep at Kp = 512
#include "score_error.hpp"     // approximation-error kernels
#include "score_evalf.hpp"     // error sums and candidates in one sweep
#include "fused_select.hpp"    // select and threshold refinement

}  // namespace
namespace {
#include "score_wide.hpp"
}
namespace {

// ------------------------------------------------------------------ host-side plan
struct FusedPlan {
	bool ok;
	bool wide;    // the plan of wide_kernel (Kp > 512, score_wide.hpp): n_tiles, stage_end, tiles_per_split count block tiles of 256 items, not tiles of 32
	int QT, BQ, n_rb, n_tiles, n_full, S, tiles_per_split, group, n_st, S0, st_per_split, n_groups, capg, kmax, flush_tiles;
	int n_stages, stage_end[3], stage_tps[3], stage_flush[3], stage_pred[3];
	int leading;
	int lg;   // candidate segments per query and item split: 2 (32x32x16 sweep: lane halves), 1 (16x16x32 sweep: wave-level queue),
	          // 4 (wide kernel: lane half x wave item half)
	int nseg;     // candidate segments per query: lg S
	bool body16;  // the sweep stages run score16_kernel
	bool bodyef;  // the sweep stages run evalf_kernel (anncur_eval_fused: candidates + error sums in one pass; 32x32x16, wave queue, static shares)
	bool bodyq16; // the sweep stages run scoreq16_kernel (Kp = 512: wave-level queue and tickets on 16x16x32 MFMAs)
	int chunk;  // dynamic tile schedule of the sweep stages: tiles per ticket (0: static shares)
	bool ladder;  // score16_kernel moves its thresholds up a ladder of levels inside ONE sweep launch (score16.hpp): no stages, no refinement launches
	int ladder_k2; // rank (in the prepass sample's group maxima) of the ladder's top level
	int sample_last;  // ladder plans with the leading sample, prepass on the sweep's body: the chunks that hold the sampled tiles; the sweep meets them last
	                  // and starts its counters from the prepass (score16.hpp 'SAMPLED TILES LAST').  0: item order, counters from zero
	size_t off_lcnt, off_lvl, off_tau2;
	size_t off_gmax, off_tval, off_tidx, off_segcnt, off_cand, off_tau, off_hard, off_ctr, off_owner, total;
};

int num_cu() { return anncur_num_cu(); }

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// Sweep stages: between stages the threshold is raised to the k-th best candidate seen so far, which cuts the survivors of the
// remaining tiles from H0 to ~1.2 k / (fraction seen).  Any split is exact; the split is picked by a small cost model with
// constants measured on MI355X (cfg2, round 1): ~2.4e-11 s of chip time per survivor, ~25 us + 3 ns per query per extra stage
// (threshold kernel + launch ramp) with the wave-level refinement kernel (k <= 128, <= 64 segments), ~1.4e-11 s per candidate
// read with the workgroup-level one.  `unit_items` = items per tile unit of P.n_tiles (32, or 256 for the wide kernel).
void plan_stages(FusedPlan &P, int64_t Q, int k, double exp_hits, bool staged, double fmin, int unit_items) {
	double frac[3] = {1.0, 1.0, 1.0};
	P.n_stages = 1;
	if (staged) {
		const double H0 = exp_hits, c_hit = 2.4e-11 * (double)Q;
		const double c_stage = k <= WSEL_K ? 25e-6 + 3e-9 * (double)Q : (k <= WQ_K2 ? 25e-6 + 1.2e-8 * (double)Q : 25e-6 + 1.4e-11 * (double)Q * 0.3 * H0);
		auto later = [&](double f) { const double h = 1.2 * k / f; return h < H0 ? h : H0; };
		double best = H0 * c_hit;
		static const double grid[] = {0.02, 0.03, 0.04, 0.06, 0.08, 0.10, 0.12, 0.15, 0.18, 0.22, 0.26, 0.30, 0.35, 0.40, 0.50};
		const int ng = (int)(sizeof(grid) / sizeof(grid[0]));
		for (int i = 0; i < ng; ++i) {
			const double f1 = grid[i];
			if (f1 < fmin) continue;
			const double c2 = (f1 * H0 + (1 - f1) * later(f1)) * c_hit + c_stage;
			if (c2 < best) { best = c2; P.n_stages = 2; frac[0] = f1; frac[1] = 1.0; }
			for (int j = i + 1; j < ng; ++j) {
				const double f2 = grid[j];
				if (f2 - f1 < fmin) continue;
				const double c3 = (f1 * H0 + (f2 - f1) * later(f1) + (1 - f2) * later(f2)) * c_hit + 2 * c_stage;
				if (c3 < best) { best = c3; P.n_stages = 3; frac[0] = f1; frac[1] = f2; }
			}
		}
	}
	// The hit-count model above knows nothing of what a first stage costs beyond its survivors: it runs against the loosest threshold
	// (dense rings, exec-mask filter) and every candidate it collects is read again by the refinement.  Measured at cfg2 size on MI355X
	// (round 3, one box, alternating): k = 100 -- the model's 0.35 stays (0.245: + 2 % sweep time on the bench matrices, level on random
	// operands); k = 500 -- the model's 0.35: 1.18 ms per call, 0.30 1.12, 0.22 1.11, 0.15 1.15 -> above k = 128 a two-stage plan
	// takes 0.6 of the model's first fraction.  The 16x16x32 body (k <= 128) gains more from a tight threshold than it loses to a
	// loose one (higher clock on sparse tiles, costlier pushes on dense ones): cfg2 sweep launches 0.458 ms at 0.35, 0.455 at 0.30,
	// 0.453 at 0.26, 0.450 at 0.22, 0.453 at 0.18, 0.461 at 0.14 -> 0.63 of the model's fraction.
	if (P.n_stages == 2) {
		const double shrink = P.body16 ? 0.63 : (k <= WSEL_K ? 1.0 : 0.6);
		const double f1 = frac[0] * shrink;
		frac[0] = f1 > fmin ? f1 : (fmin < frac[0] ? fmin : frac[0]);
	}
	double rate = exp_hits / ((double)P.n_tiles * 2.0);  // expected hits per (query half, tile) in the first stage
	int prev = 0;
	for (int i = 0; i < P.n_stages; ++i) {
		int end = (int)(frac[i] * P.n_tiles + 0.5);
		if (i == P.n_stages - 1 || end > P.n_tiles) end = P.n_tiles;
		if (end <= prev) end = prev + 1 < P.n_tiles ? prev + 1 : P.n_tiles;
		P.stage_end[i] = end;
		P.stage_tps[i] = (end - prev + P.S - 1) / P.S;
		// ring window: expected hits per (lane, sub-tile) ring and window <= 0.35, so that 8 slots wrap with p ~ 1.5e-10 per window
		// (cfg2: 3.1e7 windows per call -> one repaired query per ~200 calls; at 0.5 it was one per ~10 calls)
		int ft = (int)(0.35 / (rate > 1e-9 ? rate : 1e-9));
		P.stage_flush[i] = ft < 1 ? 1 : (ft > 8 ? 8 : ft);
		// Filter variant of the stage: `rate` survivors per (lane, sub-tile, tile) = rate / 16 per element, so a compare finds a survivor
		// in one of its 64 lanes with P = 1 - exp(-4 rate).  The ballot variant pays for that with a wave-level branch out and back, the
		// exec variant (filter_one<.., true>) with two more scalar instructions on EVERY compare and a shorter survivor block.  Measured
		// (MI355X, one process, alternating): cfg2 k = 100 (P ~ 0.3-0.5) exec 0.535 vs ballot 0.551 ms per sweep; k = 500 (P ~ 0.9)
		// 0.84 vs 0.88; I = 10^6, Kp = 256 (P ~ 0.2 over most of the sweep) 2.80 vs 2.76 -> exec above P = 0.25.
		// (staggered Kp <= 256 loop only: launch_fused ignores it elsewhere)
		P.stage_pred[i] = (1.0 - exp(-4.0 * rate)) > 0.25 ? 1 : 0;
		// next stage: threshold = k-th best of the fraction seen so far
		rate = (double)k / ((double)end * unit_items) * 16.0 * 1.2;
		prev = end;
	}
}

// ---- what plan_fused and plan_wide share: one plan structure in two tile units (32 items; block tiles of 256 items).  Where the two differ,
// it shows as an argument here or stays in the planner.
// `slack`: items the last tile may reach past I while indices stay below 2^31
bool plan_shape_ok(int64_t Q, int64_t I, int k, int slack) {
	return k >= 1 && k <= ANNCUR_MAX_TOPK && Q >= 1 && I >= 1 && I < (int64_t)0x7fffffff - slack && k <= I;
}
// Prepass sample: enough groups that the k-th largest group maximum is a tight bound.  A sampled tile gives `gpt16` groups of 16 items or
// 4 gpt16 groups of 4, and stands for at least `min_sweep` full tiles.  False: the problem is too small for the fused path (dense GEMM + scan).
bool plan_sample(FusedPlan &P, int k, int gpt16, int min_sweep) {
	const int target = (4 * k > 512) ? 4 * k : 512;
	const int n16 = (target + gpt16 - 1) / gpt16;
	if ((int64_t)n16 * 8 <= P.n_full) { P.group = 16; P.n_st = n16; }
	else { P.group = 4; P.n_st = (target + 4 * gpt16 - 1) / (4 * gpt16); }
	if ((int64_t)P.n_st * min_sweep > P.n_full) return false;
	P.n_groups = P.n_st * (P.group == 16 ? gpt16 : 4 * gpt16);
	return P.n_groups >= k;
}
// item splits of the prepass over the sample tiles
void plan_prepass_splits(FusedPlan &P, int slots) {
	int S0 = slots / P.n_rb;
	if (S0 < 1) S0 = 1;
	if (S0 > P.n_st) S0 = P.n_st;
	P.st_per_split = (P.n_st + S0 - 1) / S0;
	P.S0 = (P.n_st + P.st_per_split - 1) / P.st_per_split;
}
// Candidate segments (P.lg and P.S are set): capacity for the expected survivors per query ~ 1.3 k * (tiles / sample tiles), spread over the
// lg S segments of a query.  Returns the survivors the stage plan should expect.
// (segment capacity -- hence the workspace size -- is planned for the strided sample whatever the hint; with item rows ordered
//  by descending norm the leading sample's threshold lets ~40 % fewer elements through: measured on the synthetic protocol)
double plan_segments(FusedPlan &P, int k, bool leading) {
	P.nseg = P.lg * P.S;
	const double exp_hits_cap = 1.3 * k * ((double)P.n_tiles / P.n_st);
	const double per_seg = exp_hits_cap / (double)P.nseg;
	int capg = next_pow2((int)(4.0 * per_seg) + 32);
	if (capg < 64) capg = 64;
	if (capg > 16384) capg = 16384;
	P.capg = capg;
	return (leading ? 0.65 : 1.0) * exp_hits_cap;
}
// The workspace: 256-byte aligned regions behind the 256-byte header.  A region the plan does not have (the ladder's; the wide plan's ticket
// counters and owner map) has size 0 and leaves the offset where it was.  Last step of a plan: sets kmax and ok.
void plan_workspace(FusedPlan &P, int64_t Q, int k, size_t ctr_bytes, size_t owner_bytes) {
	P.kmax = k <= 128 ? 128 : (k <= 512 ? 512 : 2048);
	const size_t ladder_rows = P.ladder ? (size_t)P.n_rb * P.BQ : 0;
	size_t off = 256;
	auto region = [&off](size_t bytes) { const size_t at = off; off = align256(off + bytes); return at; };
	P.off_ctr = region(ctr_bytes);                            // ticket counters [stage][row block][slice]: zeroed with the header by the prepass (zero_ws_header)
	P.off_lcnt = region(ladder_rows * 16);                    // ladder counter words: zeroed with the header too
	P.off_gmax = region((size_t)Q * P.n_groups * 4);
	P.off_tval = region((size_t)Q * k * 4);
	P.off_tidx = region((size_t)Q * k * 4);
	P.off_segcnt = region((size_t)Q * P.nseg * 4);
	P.off_tau = region((size_t)Q * 4);
	P.off_hard = region((size_t)Q * 4);
	P.off_owner = region(owner_bytes);                        // chunk owners
	P.off_lvl = region(ladder_rows * 4 * LADDER_LEVELS);
	P.off_tau2 = region(P.ladder ? (size_t)Q * 4 : 0);
	P.off_cand = region((size_t)Q * P.nseg * (size_t)P.capg * 8);   // (lanes past Q never store: PAD_ROW_COUNT in csrc/common.hpp)
	P.total = off;
	P.ok = true;
}

// What a caller asks of the plan: the flags word of the C entry points (plan_opts_of_flags below: ANNCUR_TOPK_LEADING_SAMPLE, _MFMA16, _QT1,
// _MFMA32, _STAGED = no_ladder), or anncur_eval_fused (evalf: the sweep stages run evalf_kernel)
struct PlanOpts { bool leading = false, mfma16 = false, qt1 = false, mfma32 = false, evalf = false, no_ladder = false; };
PlanOpts evalf_opts() { PlanOpts o; o.evalf = true; return o; }

FusedPlan plan_fused(int64_t Q, int64_t I, int KP, int k, const PlanOpts &opts) {
	FusedPlan P{};
	if (!(KP == 64 || KP == 128 || KP == 256 || KP == 512) || !plan_shape_ok(Q, I, k, 64)) return P;
	const bool evalf = opts.evalf;
	if (evalf && !(KP <= 256 && I < (int64_t)(1 << 26))) return P;   // anncur_eval_fused: Kp <= 256 (two workgroups per CU), queue entries carry the query
	// (anncur_eval_fused has one body and samples in item order: the variants and the hint do not apply)
	const bool leading = opts.leading && !evalf, mfma16 = opts.mfma16 && !evalf, qt1 = opts.qt1 && !evalf, mfma32 = opts.mfma32 && !evalf, no_ladder = opts.no_ladder;
	P.leading = leading ? 1 : 0;
	P.bodyef = evalf;
	// qt1 (ANNCUR_TOPK_QT1, Kp = 128 / 256): one 32-query sub-tile per wave with the cross-tile pipeline of the Kp = 512 sweep,
	// 3 workgroups per CU (<= 168 VGPRs) instead of two sub-tiles staggered inside a wave at 2 workgroups per CU
	P.QT = (KP <= 256 && !(qt1 && KP >= 128)) ? 2 : 1;
	P.BQ = 128 * P.QT;
	P.n_rb = (int)ceil_div64(Q, P.BQ);
	P.n_tiles = (int)ceil_div64(I, TILE_I);
	P.n_full = (int)(I / TILE_I);
	if (!plan_sample(P, k, 2, 4)) return P;   // two groups of 16 per sampled tile (the sub-tile rows with bit 2 clear / set)
	int slots = ((P.QT == 1 && KP <= 256) ? 3 : 2) * num_cu();
	// Dynamic tile schedule (staggered 32x32x16 sweep, Kp <= 256): tickets of CHUNK_TILES tiles per query row block instead of fixed shares
	// (score_sweep_kernel).  Workgroups per row block: enough to fill every slot (rounded UP -- a workgroup that finds no ticket left ends at
	// once), at most 32 so that the 2 S segments of a query fit the wave-level select.
	// Kp = 512: the body with the wave-level queue (score_q16.hpp: queue + counters + ticket words fit the 16 KB the rings took) unless
	// ANNCUR_TOPK_MFMA32 asks for the per-lane-ring body (static shares: no LDS left for its ticket words) or I >= 2^26.  (16x16x32 MFMAs
	// against the same body on 32x32x16, cfg4 per-GPU shape, one box, alternating: sweep launches 5.21 -> 5.02 ms, step 7.19 -> 7.00)
	P.bodyq16 = KP == 512 && !mfma32 && I < (int64_t)(1 << 26);
	const bool ticketed = (P.QT == 2 || P.bodyq16) && !evalf;   // the bodies with the ticket schedule
	P.chunk = ticketed ? CHUNK_TILES : 0;
	// Body of the sweep stages
	const bool can16 = KP <= 256 && P.QT == 2 && I < (int64_t)(1 << 26);
	// (default up to k = 384 since late round 4: same process, warm, round robin at cfg2 size -- k = 150: 0.733 vs 0.738 ms for the 32x32x16 body,
	//  200: 0.779 vs 0.827, 256: 0.829 vs 0.878, 300: 0.909 vs 0.942, 384: 0.951 vs 0.968; level from 500 on: 1.04 / 1.04, 1000: 1.50 / 1.50)
	// Round 5: with the in-flight threshold ladder (score16.hpp; needs the wave-level threshold kernel, i.e. <= 4096 group maxima: k <= 1024) the
	// 16x16x32 body wins up to k = 1024 -- one process, alternating, cfg2 size: k = 500 0.984 ms against 1.055-1.072 for the staged 32x32x16 body
	// (1970 against 2606 candidates per query, select 0.144 against 0.19), k = 1000 1.38 against 1.53; without the ladder (ANNCUR_TOPK_STAGED) the
	// round-4 limit stands
	constexpr int BODY16_MAX_K = 384, BODY16_MAX_K_LADDER = 1024;
	int S = P.chunk > 0 ? (slots + P.n_rb - 1) / P.n_rb : slots / P.n_rb;
	if (P.chunk > 0 && k <= WQ_K2 && S > WAVE / 2) S = WAVE / 2;
	if (S < 1) S = 1;
	if (S > 255) S = P.chunk > 0 ? 255 : (S > 256 ? 256 : S);   // (the owner map holds a split in a byte, 255 = none)
	if (S > P.n_tiles) S = P.n_tiles;
	P.tiles_per_split = (P.n_tiles + S - 1) / S;
	P.S = (P.n_tiles + P.tiles_per_split - 1) / P.tiles_per_split;
	// The ladder's counters are 16-bit fields, two per word: a wrap in a low half (levels 1, 3, 5, 7) would carry +1 into the next level's count,
	// and a move on that count could drop the true k-th item.  Bound on a field (score16.hpp): the S waves that serve a query (one per item split)
	// add to level j's field only while their own threshold is below level j.  Once k candidates at or above level j have been counted (time T:
	// the field holds <= k then), a wave adds to it only what it drains before its next refresh, which raises its threshold to j:
	//   - one fetch period: the first fetch issued after T comes at most LADDER_PERIOD tiles later;
	//   - the lag tile: its words are consumed at the head of the NEXT tile (and T may fall inside a tile whose pushes are drained later), and
	//     the last tile's sub-tiles {2,3} are filtered and drained after the tile loop: one tile each, <= TILE_I candidates per query and tile;
	//   - the entries still queued ahead of a drain: a head drain waits for DRAIN_AT entries, so fewer than DRAIN_AT of the query's candidates
	//     may sit in the queue at T.
	// (The cold drains inside a tile do not count.)  So a field never exceeds k + S ((LADDER_PERIOD + 2) TILE_I + DRAIN_AT), and the ladder runs
	// only while that stays below half a field (or while I itself is below a field's range: a field counts distinct items).  With S <= WAVE / 2
	// (k <= WQ_K2) and LADDER_PERIOD = 16 this is 1024 + 32 x 768 = 25 600 <= 32 768: the gate does not bind today; it keeps a later change of
	// WQ_K2, the cap on S, LADDER_PERIOD or the tile size from bringing the carry back unnoticed (tests/test_cpu_host.py checks it on a grid).
	constexpr int64_t LADDER_WAVE_SLACK = (int64_t)(LADDER_PERIOD + 2) * TILE_I + Fused16Cfg<256>::DRAIN_AT;   // (DRAIN_AT: the same for every Kp)
	const bool ladder_fits = I < 65536 || (int64_t)k + (int64_t)P.S * LADDER_WAVE_SLACK <= 32768;
	const bool ladder_possible = !no_ladder && ticketed && P.n_groups <= 4096 && ladder_fits;
	P.body16 = can16 && !mfma32 && !evalf && (mfma16 || k <= (ladder_possible ? BODY16_MAX_K_LADDER : BODY16_MAX_K));
	// Body of the sweep stages (Kp <= 256, two sub-tiles per wave): 16x16x32 MFMAs with one candidate queue per wave (score16.hpp; its queue
	// entries carry the query beside the item: I < 2^26) for k <= 128, 32x32x16 with per-lane rings above (at k = 500 half of the leading
	// tiles' elements pass the first threshold: the rings' raw-tile hand-over is built for that).  ANNCUR_TOPK_MFMA16 / _MFMA32 force one.
	// Measured at cfg2, MI355X, same box, alternating (round 3): sweep launches 0.457 ms (16x16x32) vs 0.479 (32x32x16) at equal stage
	// split, 0.450 with the split below; a mixed plan (first stage 32x32x16, later stages 16x16x32) was level with 16x16x32 throughout.
	plan_prepass_splits(P, slots);
	// candidate segments per (query, item split): two (lane halves) in the 32x32x16 sweep, ONE in the 16x16x32 sweep (wave-level queue)
	P.lg = (P.body16 || P.bodyq16 || P.bodyef) ? 1 : 2;
	const double exp_hits = plan_segments(P, k, leading);
	// queue window: keep the expected hits per (lane, sub-tile) window near 0.5 so that 8 slots overflow with p ~ 1e-9
	const double per_lane_tile = exp_hits / ((double)P.n_tiles * 2.0);  // hits per query-half per tile
	int ft = (int)(0.35 / (per_lane_tile > 1e-9 ? per_lane_tile : 1e-9));
	P.flush_tiles = ft < 1 ? 1 : (ft > 8 ? 8 : ft);
	// Threshold ladder (score16.hpp, round 5): the default 16x16x32 body raises its thresholds inside ONE launch from counts of what it keeps, so it
	// runs unstaged.  The ladder's top level = the sample's group maximum of rank k2 ~ where the k-th best of ALL items is expected to fall among
	// the sample's (k x sample items / I; the norm-ordered leading sample holds about twice its share of the high scorers), at least 3, at most k / 2.
	P.ladder = P.body16 && ladder_possible;
	{
		double r = (double)k * ((double)P.n_st * TILE_I / (double)I) * (leading ? 2.0 : 1.25);
		int k2 = (int)(r + 0.5);
		if (k2 > k / 2) k2 = k / 2;
		if (k2 < 3) k2 = 3;
		if (k2 > k) k2 = k;
		P.ladder_k2 = k2;
	}
	// Sampled tiles last + pre-credited counters (score16.hpp): the sample must be the leading tiles, and a group maximum must be bit-equal to the
	// sweep's score of its item -- prepass16_kernel (groups of 16), not score_prepass_kernel's 32x32x16 chain.  The ladder runs in one stage.
	P.sample_last = 0;
	if (P.ladder && leading && P.group == 16 && P.chunk > 0) {
		const int r = (P.n_st + P.chunk - 1) / P.chunk, n_chunks = (P.n_tiles + P.chunk - 1) / P.chunk;
		if (r < n_chunks) P.sample_last = r;
	}
	plan_stages(P, Q, k, exp_hits, !P.ladder && (k <= WQ_K2 ? P.nseg <= WAVE : true) && P.n_tiles >= 24 * P.S, 4.0 * P.S / P.n_tiles, TILE_I);
	plan_workspace(P, Q, k, (size_t)P.n_rb * 3 * 4 * N_SLICES, (size_t)3 * P.n_rb * (size_t)(P.n_tiles / (P.chunk > 0 ? P.chunk : P.n_tiles) + 2));
	return P;
}

// Threshold refinement between two sweep stages: tau[q] = max(tau[q], k-th best candidate collected so far).
int launch_tau_refine(const uint2 *cand, const uint32_t *seg_cnt, int nseg, int capg, int64_t Q, int k, int kmax, float *tau, int tau_stride,
					  int prefilter, hipStream_t st) {
	int rc;
	if (k <= WQ_K2 && nseg <= WAVE) {
		if (k <= WSEL_K) {
			constexpr int lds = 4 * WaveSelLayout<WqCfg<128>::CAP>::BYTES;
			if ((rc = anncur_ensure_dyn_lds((const void *)select_wave_kernel<true, 128>, lds)) != ANNCUR_OK) return rc;
			hipLaunchKernelGGL((select_wave_kernel<true, 128>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), lds, st, cand, seg_cnt, nseg, capg, Q,
							   (uint32_t)k, (float *)nullptr, (int32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, tau, tau_stride, prefilter, (const int32_t *)nullptr);
		} else {  // streaming radix select (select_stream.hpp): 1 KB of LDS per wave
			constexpr int lds = 4 * StreamSelLayout::BYTES;
			hipLaunchKernelGGL((select_stream_kernel<true, 2>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), lds, st, cand, seg_cnt, nseg, capg, Q,
							   (uint32_t)k, (float *)nullptr, (int32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, tau, tau_stride, prefilter, (const int32_t *)nullptr);
		}
	} else {
#define LAUNCH_TAU(KM)                                                                                                        \
		do {                                                                                                                  \
			if ((rc = anncur_ensure_dyn_lds((const void *)tau_block_kernel<KM>, (int)SelCfg<KM>::LDS_BYTES)) != ANNCUR_OK) return rc; \
			hipLaunchKernelGGL((tau_block_kernel<KM>), dim3((unsigned)Q), dim3(SEL_THREADS), SelCfg<KM>::LDS_BYTES, st, cand, seg_cnt, \
							   nseg, capg, (uint32_t)k, tau, tau_stride, prefilter);                                           \
		} while (0)
		if (kmax == 128) LAUNCH_TAU(128); else if (kmax == 512) LAUNCH_TAU(512); else LAUNCH_TAU(2048);
#undef LAUNCH_TAU
	}
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

// Per-query exact top-k of the collected candidates.  Fast path: one wave per query (k <= 128, <= 64 segments); what it cannot
// take (overflowed segment, fewer than k candidates) lands in hard_list for the workgroup-level kernel, which repairs it exactly.
int launch_select(const FusedPlan &P, const SweepStages &stages, const uint2 *cand, const uint32_t *seg_cnt, const uint16_t *X, int64_t ldx,
				  const uint16_t *Et, int64_t Q, int64_t I, int KP, int k, float *out_val, int32_t *out_idx, unsigned char *ws, const float *tau,
				  int tau_stride, hipStream_t st, const int32_t *remap = nullptr) {
	int rc;
#define LAUNCH_SELECT(KM)                                                                                              \
	do {                                                                                                               \
		const size_t lds = SelCfg<KM>::LDS_BYTES + (size_t)KP * 4 + 32;                                                \
		if ((rc = anncur_ensure_dyn_lds((const void *)select_candidates_kernel<KM>, (int)lds)) != ANNCUR_OK) return rc; \
		hipLaunchKernelGGL((select_candidates_kernel<KM>), dim3(sel_grid), dim3(SEL_THREADS), lds, st, cand, seg_cnt, P.nseg, \
						   P.S, stages, P.capg, X, ldx, Et, I, KP, (uint32_t)k, out_val, out_idx, (uint32_t *)ws, hard_list, hard_cnt,      \
						   (P.n_stages > 1 || P.ladder) ? tau : (const float *)nullptr, tau_stride, remap);                              \
	} while (0)
	const int32_t *hard_list = nullptr;
	const uint32_t *hard_cnt = nullptr;
	unsigned sel_grid = (unsigned)Q;
	if (k <= WQ_K2 && P.nseg <= WAVE) {
		int32_t *hl = (int32_t *)(ws + P.off_hard);
		uint32_t *hc = (uint32_t *)(ws + 4);
#define LAUNCH_WSEL(KW)                                                                                                           \
		do {                                                                                                                      \
			constexpr int lds = 4 * WaveSelLayout<WqCfg<KW>::CAP>::BYTES;                                                         \
			if ((rc = anncur_ensure_dyn_lds((const void *)select_wave_kernel<false, KW>, lds)) != ANNCUR_OK) return rc;           \
			hipLaunchKernelGGL((select_wave_kernel<false, KW>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), lds, st, cand, seg_cnt, P.nseg, P.capg, Q, \
							   (uint32_t)k, out_val, out_idx, hc, hl, const_cast<float *>(tau), tau_stride, (P.n_stages > 1 || P.ladder) ? 1 : 0, remap); \
		} while (0)
#define LAUNCH_SSEL(EE)                                                                                                           \
		do {                                                                                                                      \
			constexpr int lds = 4 * StreamSelLayout::BYTES;                                                                       \
			hipLaunchKernelGGL((select_stream_kernel<false, EE>), dim3((unsigned)ceil_div64(Q, 4)), dim3(256), lds, st, cand, seg_cnt, P.nseg, P.capg, Q, \
							   (uint32_t)k, out_val, out_idx, hc, hl, const_cast<float *>(tau), tau_stride, (P.n_stages > 1 || P.ladder) ? 1 : 0, remap); \
		} while (0)
		if (k <= WSEL_K) LAUNCH_WSEL(128);
		else if (k <= 256) LAUNCH_SSEL(4);
		else if (k <= 512) LAUNCH_SSEL(8);
		else LAUNCH_SSEL(16);
#undef LAUNCH_SSEL
#undef LAUNCH_WSEL
		ANNCUR_LAUNCH_OK();
		hard_list = hl; hard_cnt = hc;
		sel_grid = (unsigned)(Q < 1024 ? Q : 1024);
	}
	if (P.kmax == 128) LAUNCH_SELECT(128); else if (P.kmax == 512) LAUNCH_SELECT(512); else LAUNCH_SELECT(2048);
#undef LAUNCH_SELECT
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

// tau = k-th largest group maximum of the prepass (a valid lower bound on the query's k-th best score)
int launch_threshold(const FusedPlan &P, const float *gmax, int64_t Q, int k, unsigned char *ws, const float *&tau, int &tau_stride, hipStream_t st) {
	if (P.n_groups <= 4096) {  // one wave per query, keys in LDS (kth_value_wave_kernel)
		float *t = (float *)(ws + P.off_tau);
		const int rc = P.ladder ? anncur_internal_kth_value(gmax, Q, P.n_groups, P.n_groups, k, t, 1, st, /*coarse=*/1, (float *)(ws + P.off_lvl), P.ladder_k2, (float *)(ws + P.off_tau2),
														 P.sample_last > 0 ? (uint32_t *)(ws + P.off_lcnt) : (uint32_t *)nullptr)   // (pre-credit: score16.hpp)
								: anncur_internal_kth_value(gmax, Q, P.n_groups, P.n_groups, k, t, 1, st, /*coarse=*/1);   // (any lower bound on the k-th best will do)
		tau = t; tau_stride = 1;
		return rc;
	}
	float *tval = (float *)(ws + P.off_tval);
	tau = tval + (k - 1); tau_stride = k;
	return anncur_rowwise_topk(gmax, ANNCUR_F32, Q, P.n_groups, P.n_groups, k, tval, (int32_t *)(ws + P.off_tidx), st);
}


// ------------------------------------------------------------------ a8: the exact scan co-scheduled with the retrieval (anncur_eval_topk)
// The retrieval is a chain of MFMA-bound sweep launches with latency-bound launches in between (threshold, refinement, select): one
// wave per query on a few KB each, most of the chip idle.  The exact top-k scan of A is HBM-bound and independent of all of them.
// Both kinds want every CU to themselves (the sweep fills the register file and the LDS; a scan that arrives first occupies the CUs
// the sweep is waiting for), so they are not left to race on two streams: the scan is cut into row chunks, and chunk i is launched on
// the auxiliary stream exactly beside the i-th latency-bound launch -- fork after the launch in front of it, join before the next
// sweep -- where it finds the chip free and hides that launch.  Chunks are whole rounds of the scan (rows in flight on the chip) so
// that none ends on a mostly empty round; the last takes the remainder.
struct CoScan {
	hipStream_t aux;
	hipEvent_t *ev;            // [2 * slots]: fork / join pairs
	const void *A; int a_dtype; int64_t lda, Q, I; int32_t k;
	float *val; int32_t *idx;
	int slots, next;           // chunks planned / launched so far
	int64_t row_end[8];        // chunk i = rows [row_end[i-1], row_end[i])
};

int co_plan(CoScan &co, int slots) {
	if (slots > 8) slots = 8;
	if (slots < 1) slots = 1;
	const int64_t round = anncur_internal_scan_rows_in_flight(co.a_dtype);
	const int64_t rounds = co.Q / round;                      // whole rounds available
	int64_t per = rounds / slots;                             // whole rounds per chunk (the last chunk takes what is left)
	if (per < 1) {                                            // fewer rounds than slots: one round per chunk while they last
		per = 1;
		slots = rounds >= 1 ? (int)rounds : 1;
	}
	int64_t r = 0;
	for (int i = 0; i < slots; ++i) { r = (i == slots - 1) ? co.Q : r + per * round; co.row_end[i] = r < co.Q ? r : co.Q; }
	co.slots = slots;
	co.next = 0;
	return anncur_event_pool(&co.ev, 2 * slots);
}
// launch the next chunk on the auxiliary stream behind everything enqueued on `st` so far
int co_fork(CoScan *co, hipStream_t st) {
	if (!co || co->next >= co->slots) return ANNCUR_OK;
	const int i = co->next++;
	const int64_t r0 = i ? co->row_end[i - 1] : 0, r1 = co->row_end[i];
	if (r1 <= r0) return ANNCUR_OK;
	ANNCUR_HIP_OK(hipEventRecord(co->ev[2 * i], st));
	ANNCUR_HIP_OK(hipStreamWaitEvent(co->aux, co->ev[2 * i], 0));
	const char *a = (const char *)co->A + (size_t)r0 * (size_t)co->lda * dtype_size(co->a_dtype);
	const int rc = anncur_rowwise_topk(a, co->a_dtype, r1 - r0, co->I, co->lda, co->k, co->val + r0 * co->k, co->idx + r0 * co->k, co->aux);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_HIP_OK(hipEventRecord(co->ev[2 * i + 1], co->aux));
	return ANNCUR_OK;
}
// `st` waits for the chunks launched so far
int co_join(CoScan *co, hipStream_t st) {
	if (!co || co->next < 1) return ANNCUR_OK;
	const int i = co->next - 1;
	if (co->row_end[i] > (i ? co->row_end[i - 1] : 0)) ANNCUR_HIP_OK(hipStreamWaitEvent(st, co->ev[2 * i + 1], 0));
	return ANNCUR_OK;
}
// whatever the plan left unlaunched (fewer latency-bound launches than chunks), then the final join
int co_finish(CoScan *co, hipStream_t st) {
	if (!co) return ANNCUR_OK;
	int rc;
	while (co->next < co->slots) {
		if ((rc = co_fork(co, st)) != ANNCUR_OK) return rc;
		if ((rc = co_join(co, st)) != ANNCUR_OK) return rc;
	}
	return co_join(co, st);
}

// A launch failed after chunks of the exact scan were forked onto the auxiliary stream: the launch stream still waits for every chunk
// issued so far, so that no work is left running into the caller's buffers behind its back and a stream capture stays joined.  (The
// exact result is then incomplete: outputs are undefined whenever a call returns an error.)
void co_abort(CoScan *co, hipStream_t st) {
	if (!co) return;
	for (int i = 0; i < co->next; ++i)
		if (co->row_end[i] > (i ? co->row_end[i - 1] : 0)) (void)hipStreamWaitEvent(st, co->ev[2 * i + 1], 0);
}

// error_lds_kernel / evalf_kernel address the workgroup's tile of the exact matrix as a uniform 64-bit base + a 32-bit byte offset per lane,
// (row within the row block) x pitch x 2 + chunk: the routes that use them are taken only while the last row's offset stays below 2^32
// (bq = 256 rows: pitch <= 8 421 504 elements).  ADVICE r4: unchecked, a longer pitch read the wrong rows silently.
bool exact_tile_offsets_fit(int64_t lda, int bq) { return lda >= 0 && (uint64_t)(bq - 1) * (uint64_t)lda * 2u + 64u < ((uint64_t)1 << 32); }
// wide_kernel (score_wide.hpp) addresses its query rows the same way: rows of the 256-query block x ldx x 2 + chunk in 32 bits.
bool wide_query_offsets_fit(int64_t ldx) { return exact_tile_offsets_fit(ldx, WBN); }

// anncur_eval_fused: the exact matrix and the two per-row sums the sweep stages also produce (evalf_kernel)
struct EvalArgs { const uint16_t *A; int64_t lda; float *err_sq, *norm_sq; const uint16_t *Et_hint; };   // Et_hint: see anncur_eval_fused_ex (may be null)

// one fused top-k call as the launchers see it (score_topk_impl has checked the arguments against the plan)
struct TopkCall {
	const void *X; int64_t ldx; const void *Et; int64_t Q, I; int KP, k; float *out_val; int32_t *out_idx; unsigned char *ws; hipStream_t st;
	hipEvent_t *ev;             // anncur_score_topk_timed: its 11 events (null otherwise)
	CoScan *co;                 // anncur_eval_topk: the exact scan to co-schedule (null otherwise)
	const int32_t *item_ids;    // may be null
	const EvalArgs *ea;         // anncur_eval_fused (null otherwise)
};

// The launch sequence of every route: prepass, threshold, sweep in stages (between two stages the thresholds are raised from the candidates
// collected so far), select.  A route supplies its two MFMA-bound launches -- launch_prepass(), launch_stage(stg, first tile): both return an
// error code --, where the threshold goes (tau, tau_stride of its parameter struct, set before the first stage) and what the select's repair
// path needs of it (`stages`; the stage ranges are filled in here, `unit` 32-item tiles per tile of the plan).  Owned here, once: the event
// points of anncur_score_topk_timed (0..4 the boundaries, 5 + 2 stg / 6 + 2 stg around each sweep launch) and the co-scan protocol (CoScan).
template <typename Prepass, typename Stage>
int run_pipeline(const FusedPlan &P, const TopkCall &c, SweepStages stages, int unit, const float *&tau, int &tau_stride, Prepass launch_prepass, Stage launch_stage) {
#define EV(i) do { if (c.ev) ANNCUR_HIP_OK(hipEventRecord(c.ev[i], st)); } while (0)
	unsigned char *const ws = c.ws; const hipStream_t st = c.st;
	const uint2 *cand = (const uint2 *)(ws + P.off_cand);
	const uint32_t *seg_cnt = (const uint32_t *)(ws + P.off_segcnt);
	int rc;
	EV(0);
	// 1. prepass
	if ((rc = launch_prepass()) != ANNCUR_OK) return rc;
	ANNCUR_LAUNCH_OK();
	EV(1);
	// 2. tau = k-th largest group maximum (beside it: the first chunk of the exact scan, anncur_eval_topk only)
	if ((rc = co_fork(c.co, st)) != ANNCUR_OK) return rc;
	if ((rc = launch_threshold(P, (const float *)(ws + P.off_gmax), c.Q, c.k, ws, tau, tau_stride, st)) != ANNCUR_OK) return rc;
	if ((rc = co_join(c.co, st)) != ANNCUR_OK) return rc;
	EV(2);
	// 3. sweep, in stages; between stages the thresholds are raised from the candidates collected so far
	for (int stg = 0, prev = 0; stg < P.n_stages; prev = P.stage_end[stg], ++stg) {
		EV(5 + 2 * stg);
		if ((rc = launch_stage(stg, prev)) != ANNCUR_OK) return rc;
		ANNCUR_LAUNCH_OK();
		EV(6 + 2 * stg);
		if (stg + 1 < P.n_stages) {
			if ((rc = co_fork(c.co, st)) != ANNCUR_OK) return rc;
			if ((rc = launch_tau_refine(cand, seg_cnt, P.nseg, P.capg, c.Q, c.k, P.kmax, const_cast<float *>(tau), tau_stride, stg > 0 ? 1 : 0, st)) != ANNCUR_OK)
				return rc;
			if ((rc = co_join(c.co, st)) != ANNCUR_OK) return rc;
		}
	}
	EV(3);
	// 4. select (beside it: the last chunk of the exact scan; the caller joins)
	if ((rc = co_fork(c.co, st)) != ANNCUR_OK) return rc;
	stages.n = P.n_stages;
	const int n_tiles32 = (int)ceil_div64(c.I, TILE_I);
	for (int g = 0, prev = 0; g < P.n_stages; prev = P.stage_end[g], ++g) {
		stages.begin[g] = prev * unit;
		stages.end[g] = P.stage_end[g] * unit < n_tiles32 ? P.stage_end[g] * unit : n_tiles32;
		stages.tps[g] = P.stage_tps[g] * unit;
	}
	// (ladder: the prefilter is the highest threshold a workgroup ended the sweep with -- k candidates at or above it were counted)
	if ((rc = launch_select(P, stages, cand, seg_cnt, (const uint16_t *)c.X, c.ldx, (const uint16_t *)c.Et, c.Q, c.I, c.KP, c.k, c.out_val, c.out_idx, ws,
							P.ladder ? (const float *)(ws + P.off_tau2) : tau, P.ladder ? 1 : tau_stride, st, c.item_ids)) != ANNCUR_OK) return rc;
	EV(4);
	return ANNCUR_OK;
#undef EV
}

template <int KP, int QTV = FusedCfg<KP>::QT>
int launch_fused(const FusedPlan &P, const TopkCall &c) {
	using Cfg = FusedCfg<KP, QTV>;
	unsigned char *const ws = c.ws; const hipStream_t st = c.st; const EvalArgs *const ea = c.ea;
	FusedParams p{};
	p.X = (const uint16_t *)c.X; p.ldx = c.ldx; p.Et = (const uint16_t *)c.Et; p.Q = c.Q; p.I = c.I;
	p.n_tiles = P.n_tiles; p.n_full_tiles = P.n_full; p.S = P.S; p.tiles_per_split = P.tiles_per_split;
	p.tile_begin = 0; p.tile_end = P.n_tiles; p.carry = 0; p.tile_step = 1;
	p.n_st = P.n_st; p.S0 = P.S0; p.st_per_split = P.st_per_split; p.sample_leading = P.leading;
	p.gmax = (float *)(ws + P.off_gmax); p.n_groups = P.n_groups;
	p.cand = (uint2 *)(ws + P.off_cand); p.seg_cnt = (uint32_t *)(ws + P.off_segcnt); p.capg = P.capg; p.flush_tiles = P.flush_tiles;
	p.nfb = (uint32_t *)ws; p.nseg = P.nseg;
	p.ladder_on = P.ladder ? 1 : 0; p.ladder_k = (uint32_t)c.k; p.ladder_mask = (uint32_t)(LADDER_PERIOD - 1);
	p.ladder = (const float *)(ws + P.off_lvl); p.ladder_cnt = (uint32_t *)(ws + P.off_lcnt); p.tau_final = (float *)(ws + P.off_tau2);

	const int chunk = (P.chunk > 0 && (Cfg::QT == 2 || P.bodyq16)) ? P.chunk : 0;   // (the one-sub-tile bodies with per-lane rings keep static shares)
	const int owner_stride = P.n_rb * (P.n_tiles / (chunk > 0 ? chunk : P.n_tiles) + 2);
	// Item split s of a stage sweeps the tiles begin + s, begin + s + S, ... (interleaved), not a contiguous range: with norm-ordered rows
	// the survivors crowd into the leading tiles, all the workgroups of a stage run at once, and with contiguous ranges the stage took
	// as long as its FIRST split (cfg2: the first stage, 22 % of the tiles, 0.236 ms against 0.306 ms for the other 78 %).
	// (score16_kernel keeps contiguous ranges)
	const int tile_step = (!P.body16 && !P.bodyq16 && !P.bodyef && P.S > 1 && chunk == 0) ? P.S : 1;
	SweepStages stages{};
	stages.stride = tile_step; stages.chunk = chunk; stages.bq = P.BQ; stages.rot = chunk > 0 ? P.sample_last : 0;
	for (int g = 0, prev = 0; g < P.n_stages; prev = P.stage_end[g], ++g) {
		stages.n_chunks[g] = chunk > 0 ? (P.stage_end[g] - prev + chunk - 1) / chunk : 0;
		stages.owner[g] = (const uint8_t *)(ws + P.off_owner) + (size_t)g * owner_stride;
	}

	// prepass; its workgroups also clear the header (+ the stages' ticket counters, the ladder's counter words): zero_ws_header -- no memset launch
	auto launch_prepass = [&]() -> int {
		p.n_wg = P.n_rb * P.S0;
		// anncur_eval_fused_ex's hint: the prepass samples the LEADING tiles of the norm-ordered copy (the likeliest high scorers: a tighter first
		// threshold), the sweep keeps the item order the exact tiles need.  Any subset of the items gives a valid threshold.
		FusedParams pp = p;
		pp.zero_bytes = (uint32_t)((chunk > 0 || P.ladder) ? P.off_gmax : 256);
		if (ea && ea->Et_hint) { pp.Et = ea->Et_hint; pp.sample_leading = 1; }
		if constexpr (KP <= 256 && QTV == 2) {   // the plans that sweep with score16_kernel: the prepass on the same body (prepass16.hpp)
			if (P.body16 && P.group == 16) {
				if (const int rcl = anncur_ensure_dyn_lds((const void *)prepass16_kernel<KP>, Prepass16Cfg<KP>::LDS_BYTES)) return rcl;
				hipLaunchKernelGGL((prepass16_kernel<KP>), dim3(p.n_wg), dim3(256), Prepass16Cfg<KP>::LDS_BYTES, st, pp);
				return ANNCUR_OK;
			}
		}
		if (P.group == 16)
			hipLaunchKernelGGL((score_prepass_kernel<KP, 16, QTV>), dim3(p.n_wg), dim3(256), 2 * Cfg::TILE_BYTES, st, pp);
		else
			hipLaunchKernelGGL((score_prepass_kernel<KP, 4, QTV>), dim3(p.n_wg), dim3(256), 2 * Cfg::TILE_BYTES, st, pp);
		return ANNCUR_OK;
	};
	auto launch_stage = [&](int stg, int prev) -> int {
		p.n_wg = P.n_rb * P.S;
		p.tile_begin = prev; p.tile_end = P.stage_end[stg]; p.tiles_per_split = P.stage_tps[stg];
		p.flush_tiles = P.stage_flush[stg]; p.carry = stg > 0;
		p.tile_step = tile_step;
		if (chunk > 0) {
			// (work ids are split-major in every kernel: split = wid / n_rb.  Row-block-major ids -- the workgroups of a row block on ONE XCD -- were
			//  measured for the ticket schedule, round 3, one box: cfg4 shape sweep 5.13 -> 6.28 ms and L2-miss traffic 9.0 -> 13.0 GB per launch,
			//  cfg2 0.451 -> 0.480 ms)
			p.chunk_tiles = chunk; p.n_chunks = (p.tile_end - p.tile_begin + chunk - 1) / chunk;
			// XCD-sliced tickets: the wave-queue bodies (Kp = 512: the shape whose sweep was close to the fabric's bandwidth; Kp <= 256: traffic only); [row block][slice] counters
			// (Kp <= 256: measured at cfg2, one process, interleaved -- sweep launches 0.5030 ms sliced vs 0.4914 unsliced, bare loops level:
			//  there the fabric is nowhere near its limit and the steals' blocking atomics cost more than the traffic they save (328 -> 180 MB
			//  per launch); the score16 body keeps the code path but runs unsliced)
			p.sliced = P.bodyq16 ? 1 : 0;
			p.chunks_per_slice = (p.n_chunks + N_SLICES - 1) / N_SLICES;
			p.chunk_ctr = (uint32_t *)(ws + P.off_ctr) + (size_t)stg * P.n_rb * N_SLICES;
			p.chunk_owner = (uint8_t *)(ws + P.off_owner) + (size_t)stg * owner_stride;
			// sampled tiles last (one-stage ladder plans only; read by score16_kernel)
			p.chunk_rot = P.sample_last; p.sample_end = P.sample_last * chunk < p.tile_end ? P.sample_last * chunk : p.tile_end;
		}
		// the first body that applies (`if constexpr`: a body is instantiated only for the KP / QTV it exists for)
		auto launch = [&](auto kernel, int lds, auto... more) -> int {
			if (const int rcl = anncur_ensure_dyn_lds((const void *)kernel, lds)) return rcl;
			hipLaunchKernelGGL(kernel, dim3(p.n_wg), dim3(256), lds, st, p, more...);
			return ANNCUR_OK;
		};
		if constexpr (KP <= 256 && QTV == 2) {  // anncur_eval_fused: candidates + error sums in one pass (score_evalf.hpp)
			if (P.bodyef && !ea) { anncur_set_error("launch_fused: evalf plan without the exact matrix"); return ANNCUR_E_INVALID; }
			if (P.bodyef) return launch(evalf_kernel<KP>, EvalFCfg<KP>::LDS_BYTES, ea->A, ea->lda, ea->err_sq, ea->norm_sq);
		}
		if constexpr (KP == 512) {  // Kp = 512 with the wave-level queue and tickets (score_q16.hpp)
			if (P.bodyq16) return launch(scoreq16_kernel<KP>, FusedQ16Cfg<KP>::LDS_BYTES);
		}
		if constexpr (KP <= 256 && QTV == 2) {  // 16x16x32 sweep (score16.hpp): one segment per (query, item split)
			if (P.body16) return launch(score16_kernel<KP>, Fused16Cfg<KP>::LDS_BYTES);
		}
		if constexpr (Cfg::QT == 2) {  // the exec-mask filter (the branch-free filter lives in the staggered path)
			if (P.stage_pred[stg]) return launch(score_sweep_kernel<KP, true, QTV>, Cfg::LDS_BYTES);
		}
		return launch(score_sweep_kernel<KP, false, QTV>, Cfg::LDS_BYTES);
	};
	return run_pipeline(P, c, stages, 1, p.tau, p.tau_stride, launch_prepass, launch_stage);
}

// ------------------------------------------------------------------ wide inner dimension (Kp > 512): score_wide.hpp
constexpr int WIDE_KP_MAX = 4096;
bool wide_kp(int KP) { return KP > 512 && KP <= WIDE_KP_MAX && (KP % 128) == 0; }

// Same plan structure in units of 256-item block tiles (P.n_tiles, stage_end, tiles_per_split); candidate segments per query:
// 4 S = lane half x wave item half x item split.
FusedPlan plan_wide(int64_t Q, int64_t I, int KP, int k, bool leading) {
	FusedPlan P{};
	P.wide = true;
	P.leading = leading ? 1 : 0;
	if (!wide_kp(KP) || !plan_shape_ok(Q, I, k, 512)) return P;
	P.QT = 2; P.BQ = WBN;
	P.n_rb = (int)ceil_div64(Q, WBN);
	P.n_tiles = (int)ceil_div64(I, WBM);
	P.n_full = (int)(I / WBM);
	if (!plan_sample(P, k, 16, 2)) return P;           // 16 groups of 16 items per sampled block tile
	const int slots = num_cu();                        // one 512-thread workgroup (128 KiB of LDS) per CU
	int S = slots / P.n_rb;
	if (S < 1) S = 1;
	if (S > 64) S = 64;
	if (k <= WQ_K2 && S > 16) S = 16;                  // 4 S <= 64 segments: wave-level refinement / select kernels
	if (S > P.n_tiles) S = P.n_tiles;
	P.tiles_per_split = (P.n_tiles + S - 1) / S;
	P.S = (P.n_tiles + P.tiles_per_split - 1) / P.tiles_per_split;
	plan_prepass_splits(P, slots);
	P.lg = 4;
	const double exp_hits = plan_segments(P, k, leading);
	while (P.capg > 64 && (int64_t)P.capg * P.nseg >= (1 << 21)) P.capg >>= 1;  // a workgroup's 256 x 4 S segments span < 4 GiB (32-bit store offsets)
	P.flush_tiles = 1;
	plan_stages(P, Q, k, exp_hits, (k <= WQ_K2 ? P.nseg <= WAVE : true) && P.n_tiles >= 4 * P.S, 1.0 * P.S / P.n_tiles, WBM);
	plan_workspace(P, Q, k, 0, 0);   // (no ticket counters, no owner map, no ladder)
	return P;
}

int launch_wide(const FusedPlan &P, const TopkCall &c) {
	unsigned char *const ws = c.ws; const hipStream_t st = c.st;
	WideParams p{};
	p.X = (const uint16_t *)c.X; p.ldx = c.ldx; p.Et = (const uint16_t *)c.Et; p.et_rows = ceil_div64(c.I, TILE_I) * TILE_I; p.Q = c.Q; p.I = c.I; p.Kp = c.KP;
	p.n_rb = P.n_rb; p.S = P.S;
	p.n_st = P.n_st; p.S0 = P.S0; p.st_per_split = P.st_per_split; p.sample_leading = P.leading; p.n_bt_full = P.n_full;
	p.gmax = (float *)(ws + P.off_gmax); p.n_groups = P.n_groups;
	p.cand = (uint2 *)(ws + P.off_cand); p.seg_cnt = (uint32_t *)(ws + P.off_segcnt); p.capg = P.capg;
	if (const int rc = anncur_ensure_dyn_lds((const void *)wide_kernel<1, 16>, W_LDS_TOTAL)) return rc;
	ANNCUR_HIP_OK(hipMemsetAsync(ws, 0, 256, st));   // (the wide prepass does not clear the header)
	// prepass over the sampled block tiles
	auto launch_prepass = [&]() -> int {
		p.n_wg = P.n_rb * P.S0;
		if (const int rcl = anncur_ensure_dyn_lds(P.group == 16 ? (const void *)wide_kernel<0, 16> : (const void *)wide_kernel<0, 4>, W_LDS_TOTAL)) return rcl;
		if (P.group == 16) hipLaunchKernelGGL((wide_kernel<0, 16>), dim3(p.n_wg), dim3(512), W_LDS_TOTAL, st, p);
		else hipLaunchKernelGGL((wide_kernel<0, 4>), dim3(p.n_wg), dim3(512), W_LDS_TOTAL, st, p);
		return ANNCUR_OK;
	};
	auto launch_stage = [&](int stg, int prev) -> int {
		p.n_wg = P.n_rb * P.S;
		p.bt_begin = prev; p.bt_end = P.stage_end[stg]; p.bt_per_split = P.stage_tps[stg]; p.carry = stg > 0;
		hipLaunchKernelGGL((wide_kernel<1, 16>), dim3(p.n_wg), dim3(512), W_LDS_TOTAL, st, p);
		return ANNCUR_OK;
	};
	return run_pipeline(P, c, SweepStages{}, WBM / TILE_I, p.tau, p.tau_stride, launch_prepass, launch_stage);
}

constexpr int TOPK_FLAGS = ANNCUR_TOPK_LEADING_SAMPLE | ANNCUR_TOPK_MFMA16 | ANNCUR_TOPK_QT1 | ANNCUR_TOPK_MFMA32 | ANNCUR_TOPK_RING | ANNCUR_TOPK_STAGED;

// The one reading of a flags word (`who`: the entry point, for the error text): unknown bits and the retired ring body are refused,
// ANNCUR_TOPK_MFMA16 yields to ANNCUR_TOPK_QT1
int plan_opts_of_flags(const char *who, int flags, PlanOpts &opts) {
	ANNCUR_REQUIRE((flags & ~TOPK_FLAGS) == 0, ANNCUR_E_INVALID, "%s: unknown flags 0x%x", who, flags);
	ANNCUR_REQUIRE((flags & ANNCUR_TOPK_RING) == 0, ANNCUR_E_UNSUPPORTED, "%s: ANNCUR_TOPK_RING (the tile-ring sweep body) is retired: measured slower than the default body", who);
	opts = PlanOpts{};
	opts.leading = (flags & ANNCUR_TOPK_LEADING_SAMPLE) != 0; opts.qt1 = (flags & ANNCUR_TOPK_QT1) != 0; opts.mfma32 = (flags & ANNCUR_TOPK_MFMA32) != 0;
	opts.mfma16 = (flags & ANNCUR_TOPK_MFMA16) != 0 && !opts.qt1; opts.no_ladder = (flags & ANNCUR_TOPK_STAGED) != 0;
	return ANNCUR_OK;
}

FusedPlan plan_any(int64_t Q, int64_t I, int KP, int k, const PlanOpts &opts = PlanOpts{}) {
	return wide_kp(KP) ? plan_wide(Q, I, KP, k, opts.leading) : plan_fused(Q, I, KP, k, opts);
}

}  // namespace

extern "C" size_t anncur_score_topk_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k) {
	const FusedPlan P = plan_any(Q, I, Kp, k);
	if (!P.ok) return 0;
	size_t t = P.total;
	PlanOpts variant[4];   // (whatever variant flag the call will carry)
	variant[0].mfma16 = variant[1].mfma32 = variant[2].qt1 = variant[3].no_ladder = true;
	for (const PlanOpts &o : variant) {
		const FusedPlan V = plan_any(Q, I, Kp, k, o);
		if (V.ok && V.total > t) t = V.total;
	}
	return t;
}

extern "C" int anncur_score_topk_supported(int64_t Q, int64_t I, int32_t Kp, int32_t k) {
	return plan_any(Q, I, Kp, k).ok ? 1 : 0;
}

// (item_ids: the select kernels report item_ids[row of Et] -- the map is applied where the indices are written, not by a launch of its own;
//  a row index is always < I there: it comes out of a candidate the sweep wrote or a recomputed item)
static int score_topk_impl(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp,
						   int32_t k, float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes,
						   void *stream, hipEvent_t *ev, int32_t flags = 0, const int32_t *item_ids = nullptr, CoScan *co = nullptr, const EvalArgs *ea = nullptr) {
	PlanOpts opts;
	int rc;
	if ((rc = plan_opts_of_flags("score_topk", flags, opts)) != ANNCUR_OK) return rc;
	const FusedPlan P = ea ? plan_fused(Q, I, Kp, k, evalf_opts()) : plan_any(Q, I, Kp, k, opts);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED,
				   "score_topk: (Q=%lld, I=%lld, Kp=%d, k=%d) is outside the fused path (Kp in {64,128,256,512} or a multiple of 128 up to %d, "
				   "1<=k<=%d, I large enough for a sampled threshold); use anncur_gemm + anncur_rowwise_topk",
				   (long long)Q, (long long)I, Kp, k, WIDE_KP_MAX, ANNCUR_MAX_TOPK);
	ANNCUR_REQUIRE(X && Et && out_val && out_idx, ANNCUR_E_INVALID, "score_topk: null pointer");
	ANNCUR_REQUIRE(lde == Kp, ANNCUR_E_INVALID, "score_topk: Et must be packed (lde == Kp), got lde=%lld", (long long)lde);
	ANNCUR_REQUIRE(ldx >= Kp && (ldx % 8) == 0, ANNCUR_E_INVALID, "score_topk: ldx must be >= Kp and a multiple of 8");
	ANNCUR_REQUIRE(!P.wide || wide_query_offsets_fit(ldx), ANNCUR_E_UNSUPPORTED,
				   "score_topk: query pitch ldx = %lld is too long for the wide kernel's 32-bit row offsets (Kp = %d > 512: 255 rows x ldx x 2 bytes must stay below 2^32, "
				   "ldx <= 8421504): pass a compact copy of X", (long long)ldx, Kp);
	ANNCUR_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)Et % 16) == 0, ANNCUR_E_INVALID, "score_topk: X and Et must be 16-byte aligned");
	ANNCUR_REQUIRE(workspace && workspace_bytes >= P.total && ((uintptr_t)workspace % 256) == 0, ANNCUR_E_WORKSPACE,
				   "score_topk: workspace of %zu bytes (256-byte aligned) required, got %zu", P.total, workspace_bytes);
	hipStream_t st = (hipStream_t)stream;
	const TopkCall c{X, ldx, Et, Q, I, Kp, k, out_val, out_idx, (unsigned char *)workspace, st, ev, co, item_ids, ea};
	if (co && (rc = co_plan(*co, P.n_stages + 1)) != ANNCUR_OK) return rc;   // one chunk per latency-bound launch: threshold, refinements, select
	if (P.wide) rc = launch_wide(P, c);
	else switch (Kp) {
		case 64: rc = launch_fused<64>(P, c); break;
		case 128: rc = P.QT == 1 ? launch_fused<128, 1>(P, c) : launch_fused<128>(P, c); break;
		case 256: rc = P.QT == 1 ? launch_fused<256, 1>(P, c) : launch_fused<256>(P, c); break;
		default: rc = launch_fused<512>(P, c); break;
	}
	if (rc == ANNCUR_OK) rc = co_finish(co, st);
	if (rc != ANNCUR_OK) co_abort(co, st);   // (never return with forked chunks unjoined)
	return rc;
}

extern "C" int anncur_score_topk_ex(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp,
									int32_t k, float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes,
									int32_t flags, const int32_t *item_ids, void *stream) {
	return score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k, out_val, out_idx, workspace, workspace_bytes, stream, nullptr, flags, item_ids);
}

extern "C" int anncur_score_topk(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp,
								 int32_t k, float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes,
								 void *stream) {
	return score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k, out_val, out_idx, workspace, workspace_bytes, stream, nullptr);
}

/* a8: exact top-k of the stored scores AND the fused approximate retrieval in one call, the scan's row chunks co-scheduled with the
 * retrieval's latency-bound launches (CoScan above).  Results are those of anncur_rowwise_topk + anncur_score_topk_ex. */
extern "C" int anncur_eval_topk(const void *A, int a_dtype, int64_t lda, int32_t k_exact, float *exact_val, int32_t *exact_idx,
								const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp, int32_t k_retvr,
								float *approx_val, int32_t *approx_idx, void *workspace, size_t workspace_bytes, int32_t flags,
								const int32_t *item_ids, void *stream, void *aux_stream) {
	ANNCUR_REQUIRE(dtype_ok(a_dtype) && A && exact_val && exact_idx && lda >= I && k_exact >= 1 && k_exact <= I && k_exact <= ANNCUR_MAX_TOPK,
				   ANNCUR_E_INVALID, "eval_topk: bad exact-scan arguments");
	if (Q == 0) return ANNCUR_OK;
	if (!aux_stream || aux_stream == stream) {   // no second stream: the two parts one after the other
		const int rc = anncur_rowwise_topk(A, a_dtype, Q, I, lda, k_exact, exact_val, exact_idx, stream);
		if (rc != ANNCUR_OK) return rc;
		return score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k_retvr, approx_val, approx_idx, workspace, workspace_bytes, stream, nullptr, flags, item_ids);
	}
	CoScan co{};
	co.aux = (hipStream_t)aux_stream;
	co.A = A; co.a_dtype = a_dtype; co.lda = lda; co.Q = Q; co.I = I; co.k = k_exact; co.val = exact_val; co.idx = exact_idx;
	return score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k_retvr, approx_val, approx_idx, workspace, workspace_bytes, stream, nullptr, flags, item_ids, &co);
}

/* a8 + a11 of one grid cell of entry point A in ONE sweep: top-k_retvr of S_hat = X . E AND err_sq[q] = sum_i (S_hat - A)^2,
 * norm_sq[q] = sum_i A^2 (score_evalf.hpp).  Operands as anncur_score_topk (Et in ITEM order) + the exact matrix as
 * anncur_approx_error_packed's lds route takes it (bf16, 16-byte aligned rows). */
extern "C" size_t anncur_eval_fused_workspace_bytes(int64_t Q, int64_t I, int32_t Kp, int32_t k) {
	const FusedPlan P = plan_fused(Q, I, Kp, k, evalf_opts());
	return P.ok ? P.total : 0;
}

extern "C" int anncur_eval_fused(const void *X, int64_t ldx, const void *Et, int64_t lde, const void *A, int a_dtype, int64_t lda,
								 int64_t Q, int64_t I, int32_t Kp, int32_t k, float *out_val, int32_t *out_idx, float *err_sq, float *norm_sq,
								 void *workspace, size_t workspace_bytes, void *stream) {
	return anncur_eval_fused_ex(X, ldx, Et, lde, nullptr, A, a_dtype, lda, Q, I, Kp, k, out_val, out_idx, err_sq, norm_sq, workspace, workspace_bytes, stream);
}
extern "C" int anncur_eval_fused_ex(const void *X, int64_t ldx, const void *Et, int64_t lde, const void *Et_hint, const void *A, int a_dtype, int64_t lda,
									int64_t Q, int64_t I, int32_t Kp, int32_t k, float *out_val, int32_t *out_idx, float *err_sq, float *norm_sq,
									void *workspace, size_t workspace_bytes, void *stream) {
	ANNCUR_REQUIRE(Kp == 64 || Kp == 128 || Kp == 256, ANNCUR_E_UNSUPPORTED, "eval_fused: Kp must be 64, 128 or 256 (got %d): use anncur_score_topk + anncur_approx_error_packed", Kp);
	ANNCUR_REQUIRE(a_dtype == ANNCUR_BF16 && A && (lda % 8) == 0 && ((uintptr_t)A % 16) == 0 && lda >= I, ANNCUR_E_UNSUPPORTED,
				   "eval_fused: the exact matrix must be bf16 with 16-byte aligned rows (lda a multiple of 8): use anncur_score_topk + anncur_approx_error(_packed) otherwise");
	ANNCUR_REQUIRE(err_sq && norm_sq, ANNCUR_E_INVALID, "eval_fused: null pointer");
	ANNCUR_REQUIRE(exact_tile_offsets_fit(lda, 256), ANNCUR_E_UNSUPPORTED,
				   "eval_fused: row pitch %lld of the exact matrix is too long for the kernel's 32-bit tile offsets (255 rows x pitch x 2 bytes must stay below 2^32): use anncur_score_topk + anncur_approx_error_packed",
				   (long long)lda);
	ANNCUR_REQUIRE(anncur_eval_fused_workspace_bytes(Q, I, Kp, k) > 0, ANNCUR_E_UNSUPPORTED, "eval_fused: shape (Q=%lld, I=%lld, Kp=%d, k=%d) is outside the fused path",
				   (long long)Q, (long long)I, Kp, k);
	if (Q == 0) return ANNCUR_OK;
	hipStream_t st = (hipStream_t)stream;
	ANNCUR_TRY(anncur_fill_words_async(err_sq, 0u, (size_t)Q, st));
	ANNCUR_TRY(anncur_fill_words_async(norm_sq, 0u, (size_t)Q, st));
	const int64_t I_full = I / TILE_I * TILE_I;
	if (I_full < I) {  // the last I % 32 columns' error terms: strided kernel of gemm.hip, accumulating into the same sums
		const int rc = anncur_internal_approx_error_acc((const uint16_t *)X, ANNCUR_BF16, ldx, (const uint16_t *)Et + I_full * lde, ANNCUR_BF16, lde,
														(const void *)((const uint16_t *)A + I_full), a_dtype, lda, Q, I - I_full, Kp, err_sq, norm_sq, stream);
		if (rc != ANNCUR_OK) return rc;
	}
	const EvalArgs ea{(const uint16_t *)A, lda, err_sq, norm_sq, (const uint16_t *)Et_hint};
	return score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k, out_val, out_idx, workspace, workspace_bytes, stream, nullptr, 0, nullptr, nullptr, &ea);
}

extern "C" int anncur_score_topk_timed(const void *X, int64_t ldx, const void *Et, int64_t lde, int64_t Q, int64_t I, int32_t Kp,
									   int32_t k, float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes,
									   int32_t flags, const int32_t *item_ids, void *stream, float *stage_ms) {
	ANNCUR_REQUIRE(stage_ms, ANNCUR_E_INVALID, "score_topk_timed: stage_ms is null");
	PlanOpts opts;
	int rc;
	if ((rc = plan_opts_of_flags("score_topk_timed", flags, opts)) != ANNCUR_OK) return rc;
	constexpr int NEV = 11;  // 0..4 stage boundaries, 5..10 begin/end of up to three sweep launches (run_pipeline)
	hipEvent_t ev[NEV];
	for (int i = 0; i < NEV; ++i) ANNCUR_HIP_OK(hipEventCreate(&ev[i]));
	const FusedPlan P = plan_any(Q, I, Kp, k, opts);
	rc = score_topk_impl(X, ldx, Et, lde, Q, I, Kp, k, out_val, out_idx, workspace, workspace_bytes, stream, ev, flags, item_ids);
	if (rc == ANNCUR_OK) {
		hipError_t e = hipEventSynchronize(ev[4]);
		if (e != hipSuccess) { anncur_set_error("hipEventSynchronize: %s", hipGetErrorString(e)); rc = ANNCUR_E_HIP; }
		for (int i = 0; i < 4 && rc == ANNCUR_OK; ++i)
			if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) { anncur_set_error("hipEventElapsedTime failed"); rc = ANNCUR_E_HIP; }
		stage_ms[4] = 0.f;
		stage_ms[6] = stage_ms[7] = stage_ms[8] = 0.f;
		for (int g = 0; g < P.n_stages && rc == ANNCUR_OK; ++g) {
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, ev[5 + 2 * g], ev[6 + 2 * g]) != hipSuccess) { anncur_set_error("hipEventElapsedTime failed"); rc = ANNCUR_E_HIP; }
			stage_ms[4] += ms;
			stage_ms[6 + g] = ms;
		}
		stage_ms[5] = (float)P.n_stages;
	}
	for (int i = 0; i < NEV; ++i) (void)hipEventDestroy(ev[i]);
	return rc;
}


/* plan introspection for benchmarks / DESIGN.md: n_sample_tiles, n_tiles, S, capg, group (tiles of 32 items, or of 256 for Kp > 512) */
extern "C" int anncur_score_topk_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out5) {
	const FusedPlan P = plan_any(Q, I, Kp, k);
	ANNCUR_REQUIRE(P.ok && out5, ANNCUR_E_UNSUPPORTED, "score_topk_plan: unsupported shape");
	out5[0] = P.n_st; out5[1] = P.n_tiles; out5[2] = P.S; out5[3] = P.capg; out5[4] = P.group;
	return ANNCUR_OK;
}

/* the same for the flags of anncur_score_topk_ex, in words: what a test needs to see that a variant flag was honoured, and to read the group
 * maxima back.  The positions are listed in include/anncur_hip.h and named again in ops.py (_plan_words). */
enum PlanWord {
	PW_N_ST, PW_N_TILES, PW_S, PW_CAPG, PW_GROUP,   // sample tiles, item tiles, item splits, segment capacity, group
	PW_LG,                   // segments per query and item split (2: 32x32x16 sweep, 1: 16x16x32 sweep, 4: wide kernel)
	PW_QT, PW_N_STAGES,      // 32-query sub-tiles per wave, sweep stages
	PW_STAGE_END = 8,        // [3]
	PW_STAGE_BODY = 11,      // [3] 0: 32x32x16 with the ballot filter, 1: with the exec-mask filter, 2: 16x16x32, 4: Kp = 512 with the wave-level queue on 16x16x32 MFMAs, 6: evalf_kernel
	PW_STAGE_FLUSH = 14,     // [3] ring drain period
	PW_LADDER = 17, PW_LADDER_K2, PW_LADDER_PERIOD,   // threshold ladder (1: the sweep raises its thresholds in-launch, score16.hpp; 0: staged), rank of its top level, LADDER_PERIOD
	PW_GMAX_OFF256, PW_N_GROUPS,   // workspace offset of the prepass' group maxima in 256-byte units, group maxima per query (row pitch of that array)
	PW_PREPASS16, PW_S0,     // prepass kernel (1: prepass16_kernel, the sweep's 16x16x32 body; 0: score_prepass_kernel<KP, ..>), prepass item splits
	PW_N_EX = 24,            // anncur_score_topk_plan_ex returns the words up to here
	PW_STAGE_TPS = 24,       // [3] tiles per item split of each stage: anncur_eval_fused_plan returns them too
	PW_N = 27
};
static void describe_plan(const FusedPlan &P, int32_t *out, int n_out, int n_max) {
	int32_t v[PW_N] = {};
	v[PW_N_ST] = P.n_st; v[PW_N_TILES] = P.n_tiles; v[PW_S] = P.S; v[PW_CAPG] = P.capg; v[PW_GROUP] = P.group; v[PW_LG] = P.lg; v[PW_QT] = P.QT;
	v[PW_N_STAGES] = P.n_stages;
	v[PW_LADDER] = P.ladder ? 1 : 0; v[PW_LADDER_K2] = P.ladder ? P.ladder_k2 : 0; v[PW_LADDER_PERIOD] = LADDER_PERIOD;
	v[PW_GMAX_OFF256] = (int32_t)(P.off_gmax / 256); v[PW_N_GROUPS] = P.n_groups; v[PW_PREPASS16] = (P.body16 && P.group == 16) ? 1 : 0; v[PW_S0] = P.S0;
	for (int g = 0; g < P.n_stages; ++g) {
		v[PW_STAGE_END + g] = P.stage_end[g]; v[PW_STAGE_FLUSH + g] = P.stage_flush[g]; v[PW_STAGE_TPS + g] = P.stage_tps[g];
		v[PW_STAGE_BODY + g] = P.bodyef ? 6 : P.body16 ? 2 : P.bodyq16 ? 4 : P.stage_pred[g];
	}
	for (int i = 0; i < n_out && i < n_max; ++i) out[i] = v[i];
}

extern "C" int anncur_score_topk_plan_ex(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, int32_t *out, int32_t n_out) {
	PlanOpts opts;
	if (const int rc = plan_opts_of_flags("score_topk_plan_ex", flags, opts)) return rc;
	const FusedPlan P = plan_any(Q, I, Kp, k, opts);
	ANNCUR_REQUIRE(P.ok && out && n_out >= 0, ANNCUR_E_UNSUPPORTED, "score_topk_plan_ex: unsupported shape");
	describe_plan(P, out, n_out, PW_N_EX);
	return ANNCUR_OK;
}

/* the plan anncur_eval_fused(_ex) runs for the cell (plan_fused(..., evalf = true): item order, static contiguous tile shares, evalf_kernel in
 * every stage -- body 6): the 24 words of anncur_score_topk_plan_ex, then the tiles per item split of each stage [3].  Host code only. */
extern "C" int anncur_eval_fused_plan(int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t *out, int32_t n_out) {
	ANNCUR_REQUIRE(Kp == 64 || Kp == 128 || Kp == 256, ANNCUR_E_UNSUPPORTED, "eval_fused_plan: Kp must be 64, 128 or 256 (got %d)", Kp);
	const FusedPlan P = plan_fused(Q, I, Kp, k, evalf_opts());
	ANNCUR_REQUIRE(P.ok && out && n_out >= 0, ANNCUR_E_UNSUPPORTED, "eval_fused_plan: shape (Q=%lld, I=%lld, Kp=%d, k=%d) is outside the fused path",
				   (long long)Q, (long long)I, Kp, k);
	describe_plan(P, out, n_out, PW_N);
	return ANNCUR_OK;
}

/* diagnostics: candidates the sweep of the LAST call on this workspace kept, per query on average (the segment counts it left behind;
 * synchronises the stream).  What a threshold plan is judged by: k ln(I / k) is what an online threshold can reach. */
extern "C" int anncur_score_topk_survivors(const void *workspace, int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, double *mean_per_query,
										   void *stream) {
	ANNCUR_REQUIRE(workspace && mean_per_query, ANNCUR_E_INVALID, "score_topk_survivors: bad arguments");
	PlanOpts opts;
	if (const int rc = plan_opts_of_flags("score_topk_survivors", flags, opts)) return rc;
	const FusedPlan P = plan_any(Q, I, Kp, k, opts);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "score_topk_survivors: unsupported shape");
	const size_t n = (size_t)Q * P.nseg;
	std::vector<uint32_t> h(n);
	ANNCUR_HIP_OK(hipMemcpyAsync(h.data(), (const unsigned char *)workspace + P.off_segcnt, n * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
	ANNCUR_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
	double tot = 0.0;
	for (size_t i = 0; i < n; ++i) tot += (h[i] & 0x80000000u) ? 0.0 : (double)h[i];   // (a poisoned count marks a repaired split)
	*mean_per_query = tot / (double)Q;
	return ANNCUR_OK;
}

/* diagnostics: the threshold ladder the sweep of the LAST call on this workspace left behind (synchronises the stream).  The plan's arrays
 * are laid out per row block (n_rb x BQ rows); the first Q rows are returned, the counter words decoded into one count per level
 * (levels[q][j - 1] <-> counts[q][j - 1]: the candidates counted with level j as the highest they reach). */
extern "C" int anncur_score_topk_ladder_state(const void *workspace, int64_t Q, int64_t I, int32_t Kp, int32_t k, int32_t flags, float *levels,
											  uint32_t *counts, float *tau_final, float *tau0, void *stream) {
	ANNCUR_REQUIRE(workspace && levels && counts && tau_final, ANNCUR_E_INVALID, "score_topk_ladder_state: bad arguments");
	PlanOpts opts;
	if (const int rc = plan_opts_of_flags("score_topk_ladder_state", flags, opts)) return rc;
	const FusedPlan P = plan_any(Q, I, Kp, k, opts);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "score_topk_ladder_state: unsupported shape");
	ANNCUR_REQUIRE(P.ladder, ANNCUR_E_UNSUPPORTED, "score_topk_ladder_state: the plan of (Q=%lld, I=%lld, Kp=%d, k=%d, flags 0x%x) has no threshold ladder",
				   (long long)Q, (long long)I, Kp, k, flags);
	const unsigned char *ws = (const unsigned char *)workspace;
	hipStream_t st = (hipStream_t)stream;
	std::vector<uint32_t> words((size_t)Q * 4);
	ANNCUR_HIP_OK(hipMemcpyAsync(levels, ws + P.off_lvl, (size_t)Q * LADDER_LEVELS * 4, hipMemcpyDeviceToHost, st));
	ANNCUR_HIP_OK(hipMemcpyAsync(words.data(), ws + P.off_lcnt, (size_t)Q * 16, hipMemcpyDeviceToHost, st));
	ANNCUR_HIP_OK(hipMemcpyAsync(tau_final, ws + P.off_tau2, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
	if (tau0) ANNCUR_HIP_OK(hipMemcpyAsync(tau0, ws + P.off_tau, (size_t)Q * 4, hipMemcpyDeviceToHost, st));   // (ladder plans: <= 4096 group maxima, tau_stride 1)
	ANNCUR_HIP_OK(hipStreamSynchronize(st));
	for (int64_t q = 0; q < Q; ++q)
		for (int j = 0; j < LADDER_LEVELS; ++j) counts[q * LADDER_LEVELS + j] = (words[(size_t)q * 4 + (j >> 1)] >> (16 * (j & 1))) & 0xffffu;
	return ANNCUR_OK;
}

/* a11 on packed bf16 operands (the layout of anncur_score_topk): err_sq[q] = sum_i (X[q,:].Et[i,:] - A[q,i])^2, norm_sq[q] = sum_i A[q,i]^2 */
extern "C" int anncur_approx_error_packed(const void *X, int64_t ldx, const void *Et, int64_t lde, const void *A, int a_dtype, int64_t lda,
										  int64_t Q, int64_t I, int32_t Kp, float *err_sq, float *norm_sq, void *stream) {
	ANNCUR_REQUIRE(Kp == 64 || Kp == 128 || Kp == 256 || Kp == 512, ANNCUR_E_UNSUPPORTED, "approx_error_packed: Kp must be 64, 128, 256 or 512 (got %d)", Kp);
	ANNCUR_REQUIRE(dtype_ok(a_dtype), ANNCUR_E_INVALID, "approx_error_packed: bad dtype");
	ANNCUR_REQUIRE(Q >= 0 && I >= 1 && I < (int64_t)0x7fffffff - 64 && lda >= I, ANNCUR_E_INVALID, "approx_error_packed: bad shape");
	ANNCUR_REQUIRE(X && Et && A && err_sq && norm_sq, ANNCUR_E_INVALID, "approx_error_packed: null pointer");
	ANNCUR_REQUIRE(lde == Kp && ldx >= Kp && (ldx % 8) == 0 && ((uintptr_t)X % 16) == 0 && ((uintptr_t)Et % 16) == 0, ANNCUR_E_INVALID,
				   "approx_error_packed: X / Et must be packed bf16 (lde == Kp, ldx multiple of 8, 16-byte aligned)");
	ANNCUR_REQUIRE((lda % 4) == 0 && ((uintptr_t)A % 16) == 0, ANNCUR_E_UNSUPPORTED,
				   "approx_error_packed: the exact matrix must be 16-byte aligned with lda a multiple of 4 (use anncur_approx_error otherwise)");
	if (Q == 0) return ANNCUR_OK;
	hipStream_t st = (hipStream_t)stream;
	ANNCUR_TRY(anncur_fill_words_async(err_sq, 0u, (size_t)Q, st));
	ANNCUR_TRY(anncur_fill_words_async(norm_sq, 0u, (size_t)Q, st));
	const int64_t I_full = I / TILE_I * TILE_I;
	if (I_full < I) {  // the last I % 32 columns: strided kernel of gemm.hip, accumulating into the same sums
		const int rc = anncur_internal_approx_error_acc((const uint16_t *)X, ANNCUR_BF16, ldx, (const uint16_t *)Et + I_full * lde, ANNCUR_BF16, lde,
														a_dtype == ANNCUR_F32 ? (const void *)((const float *)A + I_full) : (const void *)((const uint16_t *)A + I_full),
														a_dtype, lda, Q, I - I_full, Kp, err_sq, norm_sq, stream);
		if (rc != ANNCUR_OK) return rc;
	}
	if (I_full == 0) return ANNCUR_OK;
	FusedParams p{};
	p.X = (const uint16_t *)X; p.ldx = ldx; p.Et = (const uint16_t *)Et; p.Q = Q; p.I = I_full;
	const int QT = (Kp <= 256) ? 2 : 1, BQ = 128 * QT;
	const int n_rb = (int)ceil_div64(Q, BQ);
	p.n_tiles = (int)(I_full / TILE_I);
	int S = 2 * num_cu() / n_rb;
	if (S < 1) S = 1;
	if (S > p.n_tiles) S = p.n_tiles;
	p.tiles_per_split = (p.n_tiles + S - 1) / S;
	S = (p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
	p.n_wg = n_rb * S;
#define LAUNCH_ERR(KPV, TA)                                                                                                   \
	hipLaunchKernelGGL((error_kernel<KPV, TA>), dim3(p.n_wg), dim3(256), 2 * FusedCfg<KPV>::TILE_BYTES, st, p, (const TA *)A, lda, err_sq, norm_sq)
#define LAUNCH_ERR_K(TA)                                                                                                      \
	do {                                                                                                                      \
		switch (Kp) {                                                                                                         \
			case 64: LAUNCH_ERR(64, TA); break;                                                                               \
			case 128: LAUNCH_ERR(128, TA); break;                                                                             \
			case 256: LAUNCH_ERR(256, TA); break;                                                                             \
			default: LAUNCH_ERR(512, TA); break;                                                                              \
		}                                                                                                                     \
	} while (0)
	// bf16 exact matrix with 16-byte aligned rows: the kernel that stages the exact tile through LDS
	// (and a row pitch whose 32-bit tile offsets cannot wrap: exact_tile_offsets_fit; longer pitches take error_kernel's 64-bit row pointers)
	const bool lds_exact = a_dtype == ANNCUR_BF16 && (lda % 8) == 0 && ((uintptr_t)A % 16) == 0 && exact_tile_offsets_fit(lda, Kp <= 256 ? 256 : 128);
	if (lds_exact) {
#define LAUNCH_ERRL(KPV)                                                                                                      \
		do {                                                                                                                  \
			const int lds_ = 2 * FusedCfg<KPV>::TILE_BYTES + 2 * FusedCfg<KPV>::BQ * 64;                                      \
			{ const int rc_ = anncur_ensure_dyn_lds((const void *)error_lds_kernel<KPV>, lds_); if (rc_ != ANNCUR_OK) return rc_; } \
			hipLaunchKernelGGL((error_lds_kernel<KPV>), dim3(p.n_wg), dim3(256), lds_, st, p, (const uint16_t *)A, lda, err_sq, norm_sq); \
		} while (0)
		switch (Kp) {
			case 64: LAUNCH_ERRL(64); break;
			case 128: LAUNCH_ERRL(128); break;
			case 256: LAUNCH_ERRL(256); break;
			default: LAUNCH_ERRL(512); break;
		}
#undef LAUNCH_ERRL
	} else if (a_dtype == ANNCUR_F32) LAUNCH_ERR_K(float); else LAUNCH_ERR_K(uint16_t);
#undef LAUNCH_ERR_K
#undef LAUNCH_ERR
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
