// Batched per-query least squares on the fp64 matrix cores: the weights of the adaptive multi-round search.
//
//   w_q = argmin_w || w R_S - c ||^2 + lambda ||w||^2,   R_S = the columns Rt[ids[q, j], :]^T of query q's scored items, kq x n_q
//
// by normal equations on the smaller side, in fp64, by Cholesky (include/anncur_hip.h has the contract and the pivot rule).  Three kernels:
//   lstsq_gram_kernel    G_q = R_S^T R_S (item side, n x n) or R_S R_S^T (query side, kq x kq): 64 x 64 tiles of the lower triangle, the rows
//                        of Rt gathered by ids[q, .], widened to fp64 and accumulated on v_mfma_f64_16x16x4_f64 (fragment maps: gemm64.hip);
//   lstsq_matvec_kernel  out[a] = sum_j Rt[ids[q, j], a] v[j]: the right-hand side R_S c^T of the query side (before the factorisation) and
//                        the result w = R_S y of the item side (after it; rounded to fp32 once, at the store);
//   lstsq_factor_kernel  one workgroup per query: left-looking Cholesky by 16-column panels in place in the workspace, then the back
//                        substitution.  The right-hand side is carried as ONE EXTRA ROW of the matrix (row gp): the panel update and the
//                        triangular solve that every row below the diagonal block gets are, for that row, exactly the forward substitution.
// Workspace of one query: (gp + 1) x gp doubles, gp = ceil16(g): rows 0..gp-1 hold G, then L (lower triangle), row gp the right-hand
// side, then z = L^-1 rhs, then (item side) y.  Every cell that is read is written here first: the caller pre-fills nothing.
//
// anncur_lstsq_extend (item side) runs the SAME three kernels on a per-query state that persists from call to call: the matrix rows
// at the pitch capp = ceil16(cap), z and y in rows of their own and a header (lstsq_state_stride below).  The kernels take the row
// pitch, the places of z and y and the first row / panel to compute as runtime arguments; anncur_lstsq_rows passes "pitch gp, z and
// y in row gp, start at 0", the extension restarts at panel p0 = n_old / 16.  Every entry of G, L, z and y goes through the same
// machine code and the same chain of fp64 operations on either way, so the two results are equal bit for bit.
//
// anncur_lstsq_seed_shared starts such a state from a prefix of ids that every query shares (the adaptive search's anchor items): the
// Gram and factor kernels run ONCE, for one query, into slot 0 -- without a right-hand side, L does not depend on one --, and
// lstsq_seed_broadcast_kernel copies L and the header to the other slots.  z is the one per-query part of the prefix; the first
// extension computes it inside the factor kernel (the HDR_ZROWS rule there), so the result stays bit-equal.
#include "common.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GT = 64, GK = 32;   // Gram tile: 64 x 64 outputs, 32-deep steps of the summed index
constexpr int GPITCH = 80;        // doubles per LDS row (gemm64.hip: the four k-rows of a fragment read do not collide)
constexpr int PB = 16;            // panel width of the factorisation = the MFMA tile
constexpr int PPITCH = 17;        // doubles per row of the LDS panel: a thread per row walks its 16 entries without bank conflicts
constexpr int MAXBLK = 9;         // row blocks per wave and panel: ceil((512 / 16 + 1) / 4)
// header of a persistent state (doubles): the largest Gram diagonal so far, the smallest accepted pivot so far, the sticky status,
// the number of leading entries of z that are valid (0 after anncur_lstsq_seed_shared, n_new after a successful factor call)
constexpr int HDR_DMAX = 0, HDR_PMIN = 1, HDR_STATUS = 2, HDR_ZROWS = 3, HDR_DOUBLES = 16;

__device__ __forceinline__ float nan_f32() { return __uint_as_float(0x7fc00000u); }

// SIDE 0 (item side): index space of G = positions j of the id list, summed index = the kq anchor queries.
// SIDE 1 (query side): index space of G = the kq anchor queries, summed index = positions j of the id list.
// A hole (id < 0 or >= m_items), a row at or beyond g and a summed index beyond its range all read as zero: the pitch pad of Rt and rows
// that no id names never enter a sum.
template <int SIDE>
__global__ __launch_bounds__(256) void lstsq_gram_kernel(const float *__restrict__ Rt, int64_t ldr, int64_t m_items, const int32_t *__restrict__ ids,
															  int64_t ld_ids, int n, int kq, int gp, int pitch, int r0, int t0, int ntp,
															  double *__restrict__ ws, int64_t ws_stride, int64_t hdr_off) {
	__shared__ double As[GK][GPITCH], Bs[GK][GPITCH];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
	const int64_t q = blockIdx.x / ntp;
	if (hdr_off >= 0 && ws[q * ws_stride + hdr_off + HDR_STATUS] != 0.0) return;   // a failed state stays as it is (workgroup-uniform)
	int t = t0 + (int)(blockIdx.x % ntp), ti = 0;   // the tiles of the rows from r0 on: t0 = the tiles of the row tiles above them
	while (t > ti) { t -= ti + 1; ++ti; }   // tile pair (ti >= tj) of the lower triangle
	const int tj = t;
	const int32_t *qi = ids + q * ld_ids;
	const int Kd = SIDE == 0 ? kq : n;
	auto fetch = [&](int row, int k) -> double {
		if (SIDE == 0) {
			if (row >= n || k >= kq) return 0.0;
			const int64_t id = qi[row];
			return (id >= 0 && id < m_items) ? (double)Rt[id * ldr + k] : 0.0;
		}
		if (row >= kq || k >= n) return 0.0;
		const int64_t id = qi[k];
		return (id >= 0 && id < m_items) ? (double)Rt[id * ldr + row] : 0.0;
	};
	f64x4 acc[2][2];
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
	constexpr int PER = GT * GK / 256;
	double ra[PER], rb[PER];
	// consecutive threads run along the index that is contiguous in Rt: k on the item side (one item's kq values), the row on the query side
	auto load = [&](int k0) {
#pragma unroll
		for (int i = 0; i < PER; ++i) {
			const int e = tid + 256 * i;
			const int r = SIDE == 0 ? e / GK : e % GT, k = SIDE == 0 ? e % GK : e / GT;
			ra[i] = fetch(ti * GT + r, k0 + k);
			rb[i] = fetch(tj * GT + r, k0 + k);
		}
	};
	auto stash = [&]() {
#pragma unroll
		for (int i = 0; i < PER; ++i) {
			const int e = tid + 256 * i;
			const int r = SIDE == 0 ? e / GK : e % GT, k = SIDE == 0 ? e % GK : e / GT;
			As[k][r] = ra[i];
			Bs[k][r] = rb[i];
		}
	};
	load(0);
	for (int k0 = 0; k0 < Kd; k0 += GK) {
		stash();
		__syncthreads();
		if (k0 + GK < Kd) load(k0 + GK);   // in flight during the MFMAs below
#pragma unroll
		for (int ks = 0; ks < GK / 4; ++ks) {
			double a[2], b[2];
#pragma unroll
			for (int i = 0; i < 2; ++i) a[i] = As[ks * 4 + (lane >> 4)][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
			for (int j = 0; j < 2; ++j) b[j] = Bs[ks * 4 + (lane >> 4)][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
		}
		__syncthreads();
	}
	double *G = ws + q * ws_stride;
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int row = ti * GT + wm * 32 + i * 16 + (lane >> 4) + 4 * r, col = tj * GT + wn * 32 + j * 16 + (lane & 15);
				if (row >= r0 && row < gp && col < gp) G[(int64_t)row * pitch + col] = acc[i][j][r];   // (rows above r0 hold L)
			}
}

// out[a] = sum_j Rt[ids[q, j], a] v[j] over the non-hole entries, in fp64, in a fixed order: a workgroup = 64 values of a (one per lane:
// a coalesced read of each gathered row), its four waves take every fourth j and their sums are added in wave order.
// SIDE 0: v = y (at v_off of the query's workspace) -> W[q, a] as fp32, NaN for a query whose factorisation failed.
// SIDE 1: v = C[q, .] -> the right-hand side b at v_off of the query's workspace, zero for kq <= a < gp.
template <int SIDE>
__global__ __launch_bounds__(256) void lstsq_matvec_kernel(const float *__restrict__ Rt, int64_t ldr, int64_t m_items, const int32_t *__restrict__ ids,
																int64_t ld_ids, const float *__restrict__ C, int64_t ldc, int n, int kq, int gp, int nchunk,
																double *ws, int64_t ws_stride, int64_t v_off, float *__restrict__ W, int64_t ldw,
																const int32_t *__restrict__ status) {
	__shared__ double part[4][64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t q = blockIdx.x / nchunk;
	const int a = (int)(blockIdx.x % nchunk) * 64 + lane;
	if (SIDE == 0 && status[q] != 0) {
		if (wave == 0 && a < kq) W[q * ldw + a] = nan_f32();
		return;
	}
	const int32_t *qi = ids + q * ld_ids;
	double *row = ws + q * ws_stride + v_off;
	double acc = 0.0;
#pragma unroll 4
	for (int j = wave; j < n; j += 4) {
		const int64_t id = qi[j];
		if (id < 0 || id >= m_items) continue;   // (wave-uniform)
		const double v = SIDE == 0 ? row[j] : (double)C[q * ldc + j];
		if (a < kq) acc += (double)Rt[id * ldr + a] * v;
	}
	part[wave][lane] = acc;
	__syncthreads();
	if (wave != 0) return;
	const double s = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
	if (SIDE == 0) {
		if (a < kq) W[q * ldw + a] = (float)s;   // the one rounding to fp32
	} else if (a < gp) {
		row[a] = a < kq ? s : 0.0;
	}
}

// One workgroup per query.  G (rows 0..gp-1 of the query's workspace, lower triangle) is overwritten by its Cholesky factor L, panel by
// panel: for panel p (columns c0 = 16 p ...) every 16-row block b >= p -- and the block that holds the right-hand-side row gp -- becomes
//   P_b = G[b][p] - sum_{k < p} L[b][k] L[p][k]^T          (MFMA, the earlier panels read back from the workspace: L2)
// in LDS; the 16 x 16 diagonal block is factored there (16 steps, one barrier each), and a thread per row solves x L_pp^T = P_row.
// Each entry of L is written once.  Index i is "padding" if it is a hole of the id list (item side) or lies in [g, gp): its row and column
// of G are zero, its diagonal is set to 1 and its right-hand side to 0, so it decouples.  lambda is added to the other diagonals as the
// panel is formed; the pivot threshold 2^-40 max_i G_ii is taken from the diagonal as the Gram kernel wrote it, before lambda.
// Runtime layout: matrix rows at `pitch`, the right-hand-side row at z_off, y written to y_off (anncur_lstsq_rows: gp, gp gp, gp gp).
// A persistent state (hdr_off >= 0) restarts at panel p0 = n_old / 16, whose rows the Gram kernel has just re-formed from r0 = 16 p0
// down.  Panels p < p0 keep their diagonal factor and their rows above r0: for them only the row blocks from p0 down are formed (the
// same left-looking sum over k < p) and solved against the STORED diagonal block; z keeps its entries below r0.  From p0 on the loop
// is the full one.  The header carries what the overwritten rows no longer show: the largest diagonal of G (the threshold only
// grows, so the smallest accepted pivot so far is tested against the new one) and the status, which is sticky.
// A SEEDED state (anncur_lstsq_seed_shared) holds L of the shared prefix but no z: its header says HDR_ZROWS = 0.  A restart that finds
// fewer valid entries of z than r0 (`zfull`, the same header word in every thread) carries the right-hand side through the old panels
// as well: rhs is initialised from C at EVERY position, the old panels' block range includes the right-hand-side block (b1 = nb) and
// their per-row solve against the stored diagonal block includes the right-hand-side row.  For that row this is the chain of the fresh
// path, instruction for instruction: the same MFMA accumulation over k < c0, then the same thread-per-row solve against the same Ld
// values (stored doubles instead of the ones just factored: equal bits).  It is this one kernel, not a copy of its source, so no
// second compilation can contract the s -= x L chain differently, and z -- hence W -- equals anncur_lstsq_rows' bit for bit.
// C == nullptr (item side; the seed's own call, Q = 1): no right-hand side at all.  L does not depend on one, so the right-hand-side
// block, row and the back substitution are left out (wave-uniformly), z, y, W and status are not touched and HDR_ZROWS becomes 0.
template <int SIDE>
__global__ __launch_bounds__(256) void lstsq_factor_kernel(const int32_t *__restrict__ ids, int64_t ld_ids, int64_t m_items, const float *__restrict__ C,
																int64_t ldc, int n, int kq, int g, int gp, int pitch, int p0, int n_old, double ridge, double *ws,
																int64_t ws_stride, int64_t z_off, int64_t y_off, int64_t hdr_off, float *__restrict__ W,
																int64_t ldw, int32_t *__restrict__ status) {
	extern __shared__ __attribute__((aligned(16))) double sm[];
	double *Pn = sm;                          // [(gp + 1) x PPITCH]: the panel, rows c0 .. gp (local row = row - c0)
	double *Ld = Pn + (gp + 1) * PPITCH;      // [16 x PPITCH]: the factored diagonal block
	double *yv = Ld + PB * PPITCH;            // [gp]: the solution of the back substitution
	double *red = yv + gp;                    // [256]
	int *padf = (int *)(red + 256);           // [gp]
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t q = blockIdx.x;
	double *G = ws + q * ws_stride;
	double *rhs = G + z_off;
	double *hdr = hdr_off >= 0 ? G + hdr_off : nullptr;
	const int nb = gp / PB, r0 = p0 * PB;
	auto at = [&](int row) -> double * { return row < gp ? G + (int64_t)row * pitch : rhs; };   // row gp = the right-hand side

	const bool norhs = SIDE == 0 && C == nullptr;
	bool zfull = false;
	double dmax = 0.0, pmin = INFINITY;
	if (hdr && n_old > 0) {   // (n_old = 0 initialises the state: nothing of it is read)
		if (hdr[HDR_STATUS] != 0.0) {   // (the same word in every thread: a uniform exit)
			if (tid == 0) status[q] = 1;
			return;
		}
		dmax = hdr[HDR_DMAX];
		pmin = hdr[HDR_PMIN];
		zfull = hdr[HDR_ZROWS] < (double)r0;   // z is not valid below r0: a seeded state
	}
	for (int i = tid; i < gp; i += 256) {
		bool pad = i >= g;
		if (SIDE == 0 && !pad) {
			const int64_t id = ids[q * ld_ids + i];
			pad = id < 0 || id >= m_items;
		}
		padf[i] = pad ? 1 : 0;
		if (SIDE == 0 && !norhs && (i >= r0 || zfull)) rhs[i] = pad ? 0.0 : (double)C[q * ldc + i];
		if (i < r0) continue;   // (L's diagonal, and z unless zfull: kept)
		if (!pad) dmax = fmax(dmax, G[(int64_t)i * pitch + i]);   // (fmax drops a NaN: the pivot test below catches it)
	}
	red[tid] = dmax;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
		__syncthreads();
	}
	const double dtot = red[0], thr = dtot * 0x1p-40;
	__syncthreads();

	bool bad = p0 > 0 && !(pmin > thr);   // an old pivot under the grown threshold
	for (int p = 0; p < nb && !bad; ++p) {
		const int c0 = p * PB;
		const bool old = p < p0;
		const bool with_rhs = !norhs && (!old || zfull);       // (the right-hand side, block nb, restarts at p0 unless zfull)
		const int b0 = old ? p0 : p, b1 = with_rhs ? nb : nb - 1;
		f64x4 acc[MAXBLK];
#pragma unroll
		for (int i = 0; i < MAXBLK; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
		for (int k = 0; k < c0; k += 4) {
			const int col = k + (lane >> 4);
			const double bf = G[(int64_t)(c0 + (lane & 15)) * pitch + col];
#pragma unroll
			for (int i = 0; i < MAXBLK; ++i) {
				const int b = b0 + wave + 4 * i;   // (wave-uniform)
				if (b <= b1) {
					const int row = b * PB + (lane & 15);
					const double af = row <= gp ? at(row)[col] : 0.0;
					acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc[i], 0, 0, 0);
				}
			}
		}
#pragma unroll
		for (int i = 0; i < MAXBLK; ++i) {
			const int b = b0 + wave + 4 * i;
			if (b <= b1) {
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const int row = b * PB + (lane >> 4) + 4 * r, col = lane & 15;
					if (row <= gp) {
						double v = at(row)[c0 + col] - acc[i][r];
						if (row == c0 + col) v = padf[row] ? 1.0 : v + ridge;
						Pn[(row - c0) * PPITCH + col] = v;
					}
				}
			}
		}
		if (old) {   // the diagonal block as an earlier call factored it
			const int i = tid >> 4, k = tid & 15;
			if (i >= k) Ld[i * PPITCH + k] = G[(int64_t)(c0 + i) * pitch + c0 + k];
		}
		__syncthreads();
		if (!old) {   // the diagonal block: right-looking, thread (i, k) owns entry (i, k) of the lower triangle
			const int i = tid >> 4, k = tid & 15;
			for (int j = 0; j < PB; ++j) {
				const double d = Pn[j * PPITCH + j];
				if (!padf[c0 + j]) {
					if (!(d > thr)) { bad = true; break; }   // (the same d in every thread: a uniform exit)
					pmin = fmin(pmin, d);
				}
				const double l = sqrt(d);
				if (k == j && i >= j) Ld[i * PPITCH + j] = i == j ? l : Pn[i * PPITCH + j] / l;
				if (k > j && i >= k) Pn[i * PPITCH + k] -= (Pn[i * PPITCH + j] / l) * (Pn[k * PPITCH + j] / l);
				__syncthreads();
			}
		}
		if (bad) break;
		if (!old) {
			const int i = tid >> 4, k = tid & 15;
			if (i >= k) G[(int64_t)(c0 + i) * pitch + c0 + k] = Ld[i * PPITCH + k];
		}
		// rows below the block, the right-hand-side row (il = gp - c0) the last; under an old panel the rows from r0 down, without it unless zfull
		for (int il = (old ? r0 - c0 : PB) + tid; il <= (with_rhs ? gp - c0 : gp - 1 - c0); il += 256) {
			double x[PB];
#pragma unroll
			for (int j = 0; j < PB; ++j) {
				double s = Pn[il * PPITCH + j];
#pragma unroll
				for (int u = 0; u < j; ++u) s -= x[u] * Ld[j * PPITCH + u];
				x[j] = s / Ld[j * PPITCH + j];
			}
#pragma unroll
			for (int j = 0; j < PB; ++j) at(c0 + il)[c0 + j] = x[j];
		}
		__syncthreads();   // L's new panel is visible to the whole workgroup, and Pn / Ld are free again
	}
	if (bad) {
		if (tid == 0) {
			if (!norhs) status[q] = 1;
			if (hdr) hdr[HDR_STATUS] = 1.0;
		}
		if (SIDE == 1)
			for (int a = tid; a < kq; a += 256) W[q * ldw + a] = nan_f32();
		return;
	}

	if (norhs) {   // the seed: L and the header, nothing else
		if (tid == 0 && hdr) {
			hdr[HDR_DMAX] = dtot;
			hdr[HDR_PMIN] = pmin;
			hdr[HDR_STATUS] = 0.0;
			hdr[HDR_ZROWS] = 0.0;
		}
		return;
	}
	// back substitution L^T y = z (z = row gp), panel by panel from the last
	for (int p = nb - 1; p >= 0; --p) {
		const int c0 = p * PB;
		{
			const int j = tid & 15, part = tid >> 4;
			double s = 0.0;
			for (int i = c0 + PB + part; i < gp; i += 16) s += G[(int64_t)i * pitch + c0 + j] * yv[i];
			red[part * 16 + j] = s;
			Ld[part * PPITCH + j] = G[(int64_t)(c0 + part) * pitch + c0 + j];   // (only the lower triangle of the block is used)
		}
		__syncthreads();
		if (wave == 0) {   // the 16 x 16 triangle: lane j holds column j of L_pp and its own partial right-hand side
			const int j = lane & 15;
			double s = rhs[c0 + j];
			for (int part = 0; part < 16; ++part) s -= red[part * 16 + j];
			double colj[PB];
#pragma unroll
			for (int u = 0; u < PB; ++u) colj[u] = Ld[u * PPITCH + j];
#pragma unroll
			for (int u = PB - 1; u >= 0; --u) {
				const double yu = __shfl(s / colj[u], u);   // lane u holds L[u][u] in colj[u]
				if (j < u) s -= colj[u] * yu;
				if (lane == u) yv[c0 + u] = yu;
			}
		}
		__syncthreads();
	}
	if (SIDE == 1) {
		for (int a = tid; a < kq; a += 256) W[q * ldw + a] = (float)yv[a];   // the one rounding to fp32
	} else {
		for (int i = tid; i < gp; i += 256) G[y_off + i] = yv[i];
	}
	if (tid == 0) {
		status[q] = 0;
		if (hdr) {
			hdr[HDR_DMAX] = dtot;
			hdr[HDR_PMIN] = pmin;
			hdr[HDR_STATUS] = 0.0;
			hdr[HDR_ZROWS] = (double)n;
		}
	}
}

// anncur_lstsq_seed_shared, second step: the factor of the shared prefix, which slot 0 of the state holds, goes to the slots 1 .. Q-1.
// Workgroup (q, rb) copies the 16-row block rb of slot 0 up to and including its diagonal block -- rows [16 rb, 16 rb + 16), columns
// [0, 16 rb + 16): the lower block triangle is all that the factor kernel reads of stored rows -- and, for rb = 0, the four header
// words that are in use.  16-byte vectors (rows start on 128-byte boundaries, a block row is a whole number of vectors), the tail of
// the loop by predication; no LDS, no barrier, and no workgroup waits on another.  nrb = ceil16(n_sh) / 16 row blocks per query.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void lstsq_seed_broadcast_kernel(double *ws, int64_t ws_stride, int64_t hdr_off, int pitch, int nrb) {
	const int tid = threadIdx.x;
	const int64_t q = 1 + blockIdx.x / nrb;
	const int rb = (int)(blockIdx.x % nrb);
	const double *src = ws;
	double *dst = ws + q * ws_stride;
	const int vpr = (rb + 1) * (PB / 2), nvec = PB * vpr;   // vectors per row of this block, and in all
#pragma unroll 4
	for (int v = tid; v < nvec; v += 256) {
		const int64_t off = (int64_t)(rb * PB + v / vpr) * pitch + 2 * (v % vpr);
		*(u32x4 *)(dst + off) = *(const u32x4 *)(src + off);
	}
	if (rb == 0 && tid < 2) *(u32x4 *)(dst + hdr_off + 2 * tid) = *(const u32x4 *)(src + hdr_off + 2 * tid);
}

// The four HIP events of a _timed call: destroyed on every way out of the caller, an error return included.
struct TimingEvents {
	hipEvent_t e[4];
	int n = 0;
	~TimingEvents() {
		while (n > 0) (void)hipEventDestroy(e[--n]);
	}
	int create() {
		for (; n < 4; ++n) ANNCUR_HIP_OK(hipEventCreate(&e[n]));
		return ANNCUR_OK;
	}
	int elapsed(float *ms3) {   // synchronises
		ANNCUR_HIP_OK(hipEventSynchronize(e[3]));
		for (int i = 0; i < 3; ++i) ANNCUR_HIP_OK(hipEventElapsedTime(&ms3[i], e[i], e[i + 1]));
		return ANNCUR_OK;
	}
};

int lstsq_gp(int n, int kq) { const int g = n < kq ? n : kq; return (g + PB - 1) / PB * PB; }
size_t lstsq_factor_lds(int gp) { return (size_t)((gp + 1) * PPITCH + PB * PPITCH + gp + 256) * sizeof(double) + (size_t)gp * sizeof(int); }

bool lstsq_shape_ok(int64_t Q, int64_t n, int64_t kq) {
	return Q >= 0 && n >= 1 && n <= ANNCUR_MAX_TOPK && kq >= 1 && kq <= ANNCUR_LSTSQ_MAX_KQ && (n < kq ? n : kq) <= ANNCUR_LSTSQ_MAX_G;
}

template <int SIDE>
int lstsq_launch(const float *Rt, int64_t ldr, int64_t m_items, int kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc, int64_t Q, int n,
				 double ridge, float *W, int64_t ldw, int32_t *status, double *ws, hipStream_t st, hipEvent_t *ev) {
	const int g = n < kq ? n : kq, gp = lstsq_gp(n, kq);
	const int64_t stride = (int64_t)(gp + 1) * gp;
	const int nt = (gp + GT - 1) / GT, ntp = nt * (nt + 1) / 2;
	const size_t lds = lstsq_factor_lds(gp);
	const int rc = anncur_ensure_dyn_lds((const void *)lstsq_factor_kernel<SIDE>, (int)lds);
	if (rc != ANNCUR_OK) return rc;
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[0], st));
	const int64_t v_off = (int64_t)gp * gp;   // the right-hand side, then z, then y: row gp
	hipLaunchKernelGGL((lstsq_gram_kernel<SIDE>), dim3((unsigned)(Q * ntp)), dim3(256), 0, st, Rt, ldr, m_items, ids, ld_ids, n, kq, gp, gp, 0, 0, ntp, ws, stride,
					   (int64_t)-1);
	if (SIDE == 1) {
		const int nchunk = (gp + 63) / 64;
		hipLaunchKernelGGL((lstsq_matvec_kernel<1>), dim3((unsigned)(Q * nchunk)), dim3(256), 0, st, Rt, ldr, m_items, ids, ld_ids, C, ldc, n, kq, gp, nchunk, ws,
						   stride, v_off, W, ldw, (const int32_t *)status);
	}
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[1], st));
	hipLaunchKernelGGL((lstsq_factor_kernel<SIDE>), dim3((unsigned)Q), dim3(256), lds, st, ids, ld_ids, m_items, C, ldc, n, kq, g, gp, gp, 0, 0, ridge, ws, stride,
					   v_off, v_off, (int64_t)-1, W, ldw, status);
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[2], st));
	if (SIDE == 0) {
		const int nchunk = (kq + 63) / 64;
		hipLaunchKernelGGL((lstsq_matvec_kernel<0>), dim3((unsigned)(Q * nchunk)), dim3(256), 0, st, Rt, ldr, m_items, ids, ld_ids, C, ldc, n, kq, gp, nchunk, ws,
						   stride, v_off, W, ldw, (const int32_t *)status);
	}
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[3], st));
	return ANNCUR_OK;
}

int lstsq_rows(const float *Rt, int64_t ldr, int64_t m_items, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc, int64_t Q, int32_t n,
			   double ridge, float *W, int64_t ldw, int32_t *status, void *workspace, size_t workspace_bytes, void *stream, float *ms3) {
	ANNCUR_REQUIRE(lstsq_shape_ok(Q, n, kq), ANNCUR_E_INVALID,
				   "lstsq_rows: need Q >= 0, 1 <= n <= %d, 1 <= kq <= %d and min(n, kq) <= %d (got Q = %lld, n = %d, kq = %d)", ANNCUR_MAX_TOPK,
				   ANNCUR_LSTSQ_MAX_KQ, ANNCUR_LSTSQ_MAX_G, (long long)Q, (int)n, (int)kq);
	ANNCUR_REQUIRE(ridge >= 0.0, ANNCUR_E_INVALID, "lstsq_rows: need ridge >= 0 (got %g)", ridge);   // (a NaN fails too)
	ANNCUR_REQUIRE(m_items >= 1 && ldr >= kq && ld_ids >= n && ldc >= n && ldw >= kq, ANNCUR_E_INVALID,
				   "lstsq_rows: need m >= 1 and row pitches ldr >= kq, ld_ids >= n, ldc >= n, ldw >= kq");
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(Rt && ids && C && W && status, ANNCUR_E_INVALID, "lstsq_rows: null pointer");
	const size_t need = anncur_lstsq_rows_workspace_bytes(Q, n, kq);
	ANNCUR_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 255) == 0, ANNCUR_E_WORKSPACE,
				   "lstsq_rows: workspace missing, misaligned (256 bytes) or too small (%zu < %zu bytes)", workspace_bytes, need);
	const int gp = lstsq_gp(n, kq), nt = (gp + GT - 1) / GT;
	ANNCUR_REQUIRE(Q * (nt * (nt + 1) / 2) < (int64_t)0x7fffffff && Q * ((kq + 63) / 64 + 1) < (int64_t)0x7fffffff, ANNCUR_E_INVALID,
				   "lstsq_rows: Q = %lld is too many queries for one launch at this size: split them", (long long)Q);
	hipStream_t st = (hipStream_t)stream;
	TimingEvents evs;
	hipEvent_t *ev = nullptr;
	if (ms3) {
		const int rce = evs.create();
		if (rce != ANNCUR_OK) return rce;
		ev = evs.e;
	}
	const int rc = n <= kq ? lstsq_launch<0>(Rt, ldr, m_items, kq, ids, ld_ids, C, ldc, Q, n, ridge, W, ldw, status, (double *)workspace, st, ev)
						   : lstsq_launch<1>(Rt, ldr, m_items, kq, ids, ld_ids, C, ldc, Q, n, ridge, W, ldw, status, (double *)workspace, st, ev);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_LAUNCH_OK();
	return ms3 ? evs.elapsed(ms3) : ANNCUR_OK;
}

// One query's persistent state, in doubles: capp rows of capp (G, then L), the row of z, the row of y, the header.
int64_t lstsq_state_stride(int capp) { return (int64_t)(capp + 2) * capp + HDR_DOUBLES; }
bool lstsq_state_ok(int64_t Q, int64_t cap) { return Q >= 0 && cap >= 1 && cap <= ANNCUR_LSTSQ_MAX_G; }

int lstsq_extend(const float *Rt, int64_t ldr, int64_t m_items, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc, int64_t Q,
				 int32_t n_old, int32_t n_new, int32_t cap, double ridge, float *W, int64_t ldw, int32_t *status, void *state, size_t state_bytes, void *stream,
				 float *ms3) {
	ANNCUR_REQUIRE(lstsq_state_ok(Q, cap) && kq >= 1 && kq <= ANNCUR_LSTSQ_MAX_KQ, ANNCUR_E_INVALID,
				   "lstsq_extend: need Q >= 0, 1 <= cap <= %d and 1 <= kq <= %d (got Q = %lld, cap = %d, kq = %d)", ANNCUR_LSTSQ_MAX_G, ANNCUR_LSTSQ_MAX_KQ,
				   (long long)Q, (int)cap, (int)kq);
	ANNCUR_REQUIRE(n_new <= kq, ANNCUR_E_INVALID,
				   "lstsq_extend: n_new = %d scored items above kq = %d: the query side has no incremental form (anncur_lstsq_rows solves it)", (int)n_new, (int)kq);
	ANNCUR_REQUIRE(n_old >= 0 && n_old < n_new && n_new <= cap, ANNCUR_E_INVALID, "lstsq_extend: need 0 <= n_old < n_new <= cap (got n_old = %d, n_new = %d, cap = %d)",
				   (int)n_old, (int)n_new, (int)cap);
	ANNCUR_REQUIRE(ridge >= 0.0, ANNCUR_E_INVALID, "lstsq_extend: need ridge >= 0 (got %g)", ridge);   // (a NaN fails too)
	ANNCUR_REQUIRE(m_items >= 1 && ldr >= kq && ld_ids >= n_new && ldc >= n_new && ldw >= kq, ANNCUR_E_INVALID,
				   "lstsq_extend: need m >= 1 and row pitches ldr >= kq, ld_ids >= n_new, ldc >= n_new, ldw >= kq");
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(Rt && ids && C && W && status, ANNCUR_E_INVALID, "lstsq_extend: null pointer");
	const size_t need = anncur_lstsq_state_bytes(Q, cap);
	ANNCUR_REQUIRE(state && state_bytes >= need && ((uintptr_t)state & 255) == 0, ANNCUR_E_WORKSPACE,
				   "lstsq_extend: state missing, misaligned (256 bytes) or too small (%zu < %zu bytes)", state_bytes, need);
	const int capp = (cap + PB - 1) / PB * PB, gp = (n_new + PB - 1) / PB * PB, p0 = n_old / PB, r0 = p0 * PB;
	const int nt = (gp + GT - 1) / GT, ti0 = r0 / GT, t0 = ti0 * (ti0 + 1) / 2, ntp = nt * (nt + 1) / 2 - t0;   // the tiles of the row tiles from ti0 on
	const int nchunk = (kq + 63) / 64;
	ANNCUR_REQUIRE(Q * ntp < (int64_t)0x7fffffff && Q * nchunk < (int64_t)0x7fffffff, ANNCUR_E_INVALID,
				   "lstsq_extend: Q = %lld is too many queries for one launch at this size: split them", (long long)Q);
	const int64_t stride = lstsq_state_stride(capp), z_off = (int64_t)capp * capp, y_off = z_off + capp, hdr_off = y_off + capp;
	const size_t lds = lstsq_factor_lds(gp);
	const int rc = anncur_ensure_dyn_lds((const void *)lstsq_factor_kernel<0>, (int)lds);
	if (rc != ANNCUR_OK) return rc;
	hipStream_t st = (hipStream_t)stream;
	TimingEvents evs;
	hipEvent_t *ev = nullptr;
	if (ms3) {
		const int rce = evs.create();
		if (rce != ANNCUR_OK) return rce;
		ev = evs.e;
	}
	double *ws = (double *)state;
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[0], st));
	hipLaunchKernelGGL((lstsq_gram_kernel<0>), dim3((unsigned)(Q * ntp)), dim3(256), 0, st, Rt, ldr, m_items, ids, ld_ids, (int)n_new, (int)kq, gp, capp, r0, t0, ntp, ws,
					   stride, n_old > 0 ? hdr_off : (int64_t)-1);
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[1], st));
	hipLaunchKernelGGL((lstsq_factor_kernel<0>), dim3((unsigned)Q), dim3(256), lds, st, ids, ld_ids, m_items, C, ldc, (int)n_new, (int)kq, (int)n_new, gp, capp, p0,
					   (int)n_old, ridge, ws, stride, z_off, y_off, hdr_off, W, ldw, status);
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[2], st));
	hipLaunchKernelGGL((lstsq_matvec_kernel<0>), dim3((unsigned)(Q * nchunk)), dim3(256), 0, st, Rt, ldr, m_items, ids, ld_ids, C, ldc, (int)n_new, (int)kq, gp, nchunk,
					   ws, stride, y_off, W, ldw, (const int32_t *)status);
	if (ev) ANNCUR_HIP_OK(hipEventRecord(ev[3], st));
	ANNCUR_LAUNCH_OK();
	return ms3 ? evs.elapsed(ms3) : ANNCUR_OK;
}

// The shared prefix factored ONCE (the Gram and factor kernels of every other call, Q = 1, on shared_ids as the one id row, into slot 0,
// without a right-hand side), then copied to every other slot.
int lstsq_seed_shared(const float *Rt, int64_t ldr, int64_t m_items, int32_t kq, const int32_t *shared_ids, int32_t n_sh, int64_t Q, int32_t cap, double ridge,
					  void *state, size_t state_bytes, void *stream) {
	ANNCUR_REQUIRE(lstsq_state_ok(Q, cap) && kq >= 1 && kq <= ANNCUR_LSTSQ_MAX_KQ, ANNCUR_E_INVALID,
				   "lstsq_seed_shared: need Q >= 0, 1 <= cap <= %d and 1 <= kq <= %d (got Q = %lld, cap = %d, kq = %d)", ANNCUR_LSTSQ_MAX_G, ANNCUR_LSTSQ_MAX_KQ,
				   (long long)Q, (int)cap, (int)kq);
	ANNCUR_REQUIRE(n_sh >= 1 && n_sh <= cap && n_sh <= kq, ANNCUR_E_INVALID, "lstsq_seed_shared: need 1 <= n_sh <= min(cap, kq) (got n_sh = %d, cap = %d, kq = %d)",
				   (int)n_sh, (int)cap, (int)kq);
	ANNCUR_REQUIRE(ridge >= 0.0, ANNCUR_E_INVALID, "lstsq_seed_shared: need ridge >= 0 (got %g)", ridge);   // (a NaN fails too)
	ANNCUR_REQUIRE(m_items >= 1 && ldr >= kq, ANNCUR_E_INVALID, "lstsq_seed_shared: need m >= 1 and the row pitch ldr >= kq");
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(Rt && shared_ids, ANNCUR_E_INVALID, "lstsq_seed_shared: null pointer");
	const size_t need = anncur_lstsq_state_bytes(Q, cap);
	ANNCUR_REQUIRE(state && state_bytes >= need && ((uintptr_t)state & 255) == 0, ANNCUR_E_WORKSPACE,
				   "lstsq_seed_shared: state missing, misaligned (256 bytes) or too small (%zu < %zu bytes)", state_bytes, need);
	const int capp = (cap + PB - 1) / PB * PB, gp = (n_sh + PB - 1) / PB * PB, nrb = gp / PB;
	const int nt = (gp + GT - 1) / GT, ntp = nt * (nt + 1) / 2;
	ANNCUR_REQUIRE((Q - 1) * nrb < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "lstsq_seed_shared: Q = %lld is too many queries for one launch at this size: split them",
				   (long long)Q);
	const int64_t stride = lstsq_state_stride(capp), z_off = (int64_t)capp * capp, y_off = z_off + capp, hdr_off = y_off + capp;
	const size_t lds = lstsq_factor_lds(gp);
	const int rc = anncur_ensure_dyn_lds((const void *)lstsq_factor_kernel<0>, (int)lds);
	if (rc != ANNCUR_OK) return rc;
	hipStream_t st = (hipStream_t)stream;
	double *ws = (double *)state;
	hipLaunchKernelGGL((lstsq_gram_kernel<0>), dim3((unsigned)ntp), dim3(256), 0, st, Rt, ldr, m_items, shared_ids, (int64_t)n_sh, (int)n_sh, (int)kq, gp, capp, 0, 0, ntp,
					   ws, stride, (int64_t)-1);
	hipLaunchKernelGGL((lstsq_factor_kernel<0>), dim3(1), dim3(256), lds, st, shared_ids, (int64_t)n_sh, m_items, (const float *)nullptr, (int64_t)0, (int)n_sh, (int)kq,
					   (int)n_sh, gp, capp, 0, 0, ridge, ws, stride, z_off, y_off, hdr_off, (float *)nullptr, (int64_t)0, (int32_t *)nullptr);
	if (Q > 1)
		hipLaunchKernelGGL(lstsq_seed_broadcast_kernel, dim3((unsigned)((Q - 1) * nrb)), dim3(256), 0, st, ws, stride, hdr_off, capp, nrb);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

}  // namespace

extern "C" int anncur_lstsq_seed_shared(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *shared_ids, int32_t n_sh, int64_t Q, int32_t cap,
										 double ridge, void *state, size_t state_bytes, void *stream) {
	return lstsq_seed_shared(Rt, ldr, m, kq, shared_ids, n_sh, Q, cap, ridge, state, state_bytes, stream);
}

extern "C" size_t anncur_lstsq_state_bytes(int64_t Q, int32_t cap) {
	if (!lstsq_state_ok(Q, cap)) return 0;
	return (size_t)Q * (size_t)lstsq_state_stride((cap + PB - 1) / PB * PB) * sizeof(double);
}

extern "C" int anncur_lstsq_extend(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc, int64_t Q,
								   int32_t n_old, int32_t n_new, int32_t cap, double ridge, float *W, int64_t ldw, int32_t *status, void *state, size_t state_bytes,
								   void *stream) {
	return lstsq_extend(Rt, ldr, m, kq, ids, ld_ids, C, ldc, Q, n_old, n_new, cap, ridge, W, ldw, status, state, state_bytes, stream, nullptr);
}

extern "C" int anncur_lstsq_extend_timed(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc,
										 int64_t Q, int32_t n_old, int32_t n_new, int32_t cap, double ridge, float *W, int64_t ldw, int32_t *status, void *state,
										 size_t state_bytes, void *stream, float *ms3) {
	ANNCUR_REQUIRE(ms3, ANNCUR_E_INVALID, "lstsq_extend_timed: ms3 is NULL");
	return lstsq_extend(Rt, ldr, m, kq, ids, ld_ids, C, ldc, Q, n_old, n_new, cap, ridge, W, ldw, status, state, state_bytes, stream, ms3);
}

extern "C" size_t anncur_lstsq_rows_workspace_bytes(int64_t Q, int32_t n, int32_t kq) {
	if (!lstsq_shape_ok(Q, n, kq)) return 0;
	const int64_t gp = lstsq_gp(n, kq);
	return (size_t)Q * (size_t)((gp + 1) * gp) * sizeof(double);
}

extern "C" int anncur_lstsq_rows(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc, int64_t Q,
								 int32_t n, double ridge, float *W, int64_t ldw, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
	return lstsq_rows(Rt, ldr, m, kq, ids, ld_ids, C, ldc, Q, n, ridge, W, ldw, status, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int anncur_lstsq_rows_timed(const float *Rt, int64_t ldr, int64_t m, int32_t kq, const int32_t *ids, int64_t ld_ids, const float *C, int64_t ldc,
									   int64_t Q, int32_t n, double ridge, float *W, int64_t ldw, int32_t *status, void *workspace, size_t workspace_bytes,
									   void *stream, float *ms3) {
	ANNCUR_REQUIRE(ms3, ANNCUR_E_INVALID, "lstsq_rows_timed: ms3 is NULL");
	return lstsq_rows(Rt, ldr, m, kq, ids, ld_ids, C, ldc, Q, n, ridge, W, ldw, status, workspace, workspace_bytes, stream, ms3);
}
