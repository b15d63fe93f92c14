// Anchor item selection by column-pivoted QR: the k items whose score columns R[:, i] (R [kq x m], the anchor rows of the
// index) span the most, taken greedily -- always the item with the largest component outside the span of those taken so far.
// include/anncur_hip.h has the contract (the sums' order, the tie rule, the stop rule).  All state is fp64 in the caller's workspace:
//   header   d_first (the first pivot's value) and the stop flag
//   d[m]     squared norm of every column's component outside the span; a TAKEN item's entry is NaN, so it is never a candidate again
//   basis    [k x kq]: row t = q_t, the orthonormal direction step t added
//   parts    one (value, id) maximum per workgroup of the step kernel
// Two launches per step, the kernel boundary their only synchronisation (no workgroup waits for another inside a launch):
//   pivot_step_kernel  over item slices.  INIT: d_i = sum_a R[a,i]^2.  Otherwise q_t in LDS, c_i = sum_a R[a,i] q_t[a], d_i <- d_i - c_i^2.
//                      A thread owns 16 bytes of consecutive items (4 fp32, 8 bf16) and walks the kq rows, eight loads in flight; it
//                      keeps the largest finite d_i it wrote (strictly larger only: the smaller id stays on a tie), the wave reduces them.
//   pivot_pick_kernel  one workgroup: the maximum of the parts, the stop rule, column p orthogonalised against the basis twice
//                      (classical Gram-Schmidt: all coefficients from the same vector, then one subtraction), normalised -> q_t, ids[t],
//                      gain[t], n_sel.  After a stop both kernels read the flag and return (the pick kernel writes the (-1, 0.0) tail).
// Every sum has a fixed order that depends on kq and the constants below alone, never on m, the grid or the dispatch order.
#include "common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int PV_THREADS = 64;      // step kernel: one wave per workgroup (at m = 100 000 that is 391 / 196 workgroups: every CU gets one)
constexpr int PV_ROWS = 8;          // rows of R a thread has in flight
constexpr int PV_MAX_WG = 2048;     // workgroups of the step kernel (256 CUs x 8): beyond, a workgroup takes every gridDim-th slice
constexpr int PK_THREADS = 1024;    // pick kernel: 16 waves
constexpr int PV_HDR_BYTES = 256;

struct PvHeader {
	double d_first;
	int32_t stopped, pad;
};
struct PvMax {
	double v;
	int32_t id, pad;
};

template <typename T>
struct PvVec;
template <>
struct PvVec<float> {
	static constexpr int N = 4;
	typedef f32x4 V;
	static __device__ __forceinline__ float get(const V &x, int e) { return x[e]; }
};
template <>
struct PvVec<uint16_t> {   // bf16: element e is half (e & 1) of dword e / 2
	static constexpr int N = 8;
	typedef u32x4 V;
	static __device__ __forceinline__ float get(const V &x, int e) { return __uint_as_float((e & 1) ? (x[e >> 1] & 0xffff0000u) : (x[e >> 1] << 16)); }
};

// (value, id) a beats b: a candidate (id >= 0) with the larger value, the smaller id on a tie.  Commutative and associative: any reduction tree gives one result.
__device__ __forceinline__ bool pv_better(double av, int32_t ai, double bv, int32_t bi) { return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi)); }

// acc[e] = fma(R[a, i0 + e], INIT ? the same : q[a], acc[e]) for a = 0 .. kq-1 in ascending order.  VECLOAD: one aligned 16-byte load per row;
// otherwise (unaligned rows, the ragged end of R) one load per element, those at or beyond nvalid not read.
template <typename T, bool INIT, bool VECLOAD>
__device__ __forceinline__ void pv_walk(const T *__restrict__ col, int64_t ldr, int kq, int nvalid, const double *q, double (&acc)[PvVec<T>::N]) {
	constexpr int N = PvVec<T>::N;
	typedef typename PvVec<T>::V V;
	int a = 0;
	for (; a + PV_ROWS <= kq; a += PV_ROWS) {
		float x[PV_ROWS][N];
		if constexpr (VECLOAD) {
			V raw[PV_ROWS];
#pragma unroll
			for (int u = 0; u < PV_ROWS; ++u) raw[u] = *reinterpret_cast<const V *>(col + (int64_t)(a + u) * ldr);
#pragma unroll
			for (int u = 0; u < PV_ROWS; ++u)
#pragma unroll
				for (int e = 0; e < N; ++e) x[u][e] = PvVec<T>::get(raw[u], e);
		} else {
#pragma unroll
			for (int u = 0; u < PV_ROWS; ++u)
#pragma unroll
				for (int e = 0; e < N; ++e) x[u][e] = e < nvalid ? load_as_f32<T>(col + (int64_t)(a + u) * ldr + e) : 0.f;
		}
#pragma unroll
		for (int u = 0; u < PV_ROWS; ++u) {
			const double qa = INIT ? 0.0 : q[a + u];
#pragma unroll
			for (int e = 0; e < N; ++e) {
				const double r = (double)x[u][e];
				acc[e] = __builtin_fma(r, INIT ? r : qa, acc[e]);
			}
		}
	}
	for (; a < kq; ++a) {
		float x[N];
		if constexpr (VECLOAD) {
			const V raw = *reinterpret_cast<const V *>(col + (int64_t)a * ldr);
#pragma unroll
			for (int e = 0; e < N; ++e) x[e] = PvVec<T>::get(raw, e);
		} else {
#pragma unroll
			for (int e = 0; e < N; ++e) x[e] = e < nvalid ? load_as_f32<T>(col + (int64_t)a * ldr + e) : 0.f;
		}
		const double qa = INIT ? 0.0 : q[a];
#pragma unroll
		for (int e = 0; e < N; ++e) {
			const double r = (double)x[e];
			acc[e] = __builtin_fma(r, INIT ? r : qa, acc[e]);
		}
	}
}

// ALIGNED: R and its row pitch are multiples of 16 bytes, so every slice's vectors are (a slice starts at a multiple of 16 bytes of items).
template <typename T, bool INIT, bool ALIGNED>
__global__ __launch_bounds__(PV_THREADS) void pivot_step_kernel(const T *__restrict__ R, int64_t ldr, int kq, int64_t m, int64_t nslices,
																 const double *__restrict__ qrow, const PvHeader *__restrict__ hdr, double *__restrict__ d,
																 PvMax *__restrict__ parts) {
	extern __shared__ __attribute__((aligned(16))) double q[];
	constexpr int N = PvVec<T>::N;
	constexpr int64_t SLICE = (int64_t)PV_THREADS * N;
	const int tid = threadIdx.x;
	if (!INIT) {
		if (hdr->stopped != 0) return;   // (the same word in every thread: a uniform exit)
		for (int a = tid; a < kq; a += PV_THREADS) q[a] = qrow[a];
		__syncthreads();
	}
	double best = 0.0;
	int32_t bid = -1;
	for (int64_t s = blockIdx.x; s < nslices; s += gridDim.x) {
		const int64_t i0 = s * SLICE + (int64_t)tid * N;
		const int64_t left = m - i0;
		const int nvalid = left >= N ? N : (left > 0 ? (int)left : 0);
		if (nvalid == 0) continue;
		double acc[N];
#pragma unroll
		for (int e = 0; e < N; ++e) acc[e] = 0.0;
		if (ALIGNED && nvalid == N) pv_walk<T, INIT, true>(R + i0, ldr, kq, nvalid, q, acc);
		else pv_walk<T, INIT, false>(R + i0, ldr, kq, nvalid, q, acc);
#pragma unroll
		for (int e = 0; e < N; ++e)
			if (e < nvalid) {
				const double dn = INIT ? acc[e] : __builtin_fma(-acc[e], acc[e], d[i0 + e]);
				d[i0 + e] = dn;
				if (fabs(dn) < INFINITY && (bid < 0 || dn > best)) {   // (NaN and +-inf fail the first test: never candidates)
					best = dn;
					bid = (int32_t)(i0 + e);
				}
			}
	}
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) {
		const double ov = __shfl_xor(best, s);
		const int32_t oi = __shfl_xor(bid, s);
		if (pv_better(ov, oi, best, bid)) {
			best = ov;
			bid = oi;
		}
	}
	if (tid == 0) {
		PvMax out;
		out.v = best;
		out.id = bid;
		out.pad = 0;
		parts[blockIdx.x] = out;
	}
}

// sum of scr[0 .. PK_THREADS) in the fixed order of the halving tree -> every thread
__device__ __forceinline__ double pk_tree_sum(double *scr, int tid) {
	__syncthreads();
	for (int s = PK_THREADS / 2; s > 0; s >>= 1) {
		if (tid < s) scr[tid] += scr[tid + s];
		__syncthreads();
	}
	const double r = scr[0];
	__syncthreads();
	return r;
}

template <typename T>
__global__ __launch_bounds__(PK_THREADS) void pivot_pick_kernel(const T *__restrict__ R, int64_t ldr, int kq, int t, int nparts, const PvMax *__restrict__ parts,
																 PvHeader *hdr, double *d, double *basis, int32_t *__restrict__ out_ids,
																 double *__restrict__ out_gain, int32_t *__restrict__ n_sel) {
	extern __shared__ __attribute__((aligned(16))) double sm[];
	double *v = sm;                          // [kq]: column p, then its component outside the span
	double *coef = v + kq;                   // [t]: the coefficients of one Gram-Schmidt pass
	double *scr = coef + t;                  // [PK_THREADS]
	int32_t *redi = (int32_t *)(scr + PK_THREADS);   // [PK_THREADS]
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	constexpr int NW = PK_THREADS / 64;
	if (t > 0 && hdr->stopped != 0) {   // (uniform)
		if (tid == 0) {
			out_ids[t] = -1;
			out_gain[t] = 0.0;
		}
		return;
	}
	double best = 0.0;
	int32_t bid = -1;
	for (int i = tid; i < nparts; i += PK_THREADS) {
		const PvMax c = parts[i];
		if (pv_better(c.v, c.id, best, bid)) {
			best = c.v;
			bid = c.id;
		}
	}
	scr[tid] = best;
	redi[tid] = bid;
	__syncthreads();
	for (int s = PK_THREADS / 2; s > 0; s >>= 1) {
		if (tid < s && pv_better(scr[tid + s], redi[tid + s], scr[tid], redi[tid])) {
			scr[tid] = scr[tid + s];
			redi[tid] = redi[tid + s];
		}
		__syncthreads();
	}
	const double dp = scr[0];
	const int32_t p = redi[0];
	const double dfirst = t > 0 ? hdr->d_first : dp;
	__syncthreads();
	bool stop = p < 0 || !(dp > 0.0) || (t > 0 && dp <= 0x1p-40 * dfirst);   // (the same values in every thread)
	if (!stop) {
		for (int a = tid; a < kq; a += PK_THREADS) v[a] = (double)load_as_f32<T>(R + (int64_t)a * ldr + p);
		__syncthreads();
		const int kqp = (kq + 63) & ~63;
		const int G = 2 * kqp <= PK_THREADS ? PK_THREADS / kqp : 1;   // groups of threads that share the basis rows of one update
		for (int pass = 0; pass < 2 && t > 0; ++pass) {
			// coef[j] = <q_j, v>: a wave per j, lane l sums a = l, l + 64, .. in ascending order, then the butterfly over the lanes
			for (int j = wave; j < t; j += NW) {
				const double *qj = basis + (int64_t)j * kq;
				double s = 0.0;
				for (int a = lane; a < kq; a += 64) s = __builtin_fma(qj[a], v[a], s);
#pragma unroll
				for (int x = 32; x > 0; x >>= 1) s += __shfl_xor(s, x);
				if (lane == 0) coef[j] = s;
			}
			__syncthreads();
			// v[a] -= sum_j coef[j] q_j[a], j ascending; with G > 1 group g sums its contiguous share of the j and the shares are added in group order
			if (G > 1) {
				const int g = tid / kqp, a = tid - g * kqp, share = (t + G - 1) / G;
				double s = 0.0;
				if (g < G && a < kq) {
					const int j1 = (g + 1) * share < t ? (g + 1) * share : t;
					for (int j = g * share; j < j1; ++j) s = __builtin_fma(coef[j], basis[(int64_t)j * kq + a], s);
				}
				scr[tid] = s;
				__syncthreads();
				if (tid < kq) {
					double tot = scr[tid];
					for (int gg = 1; gg < G; ++gg) tot += scr[gg * kqp + tid];
					v[tid] -= tot;
				}
			} else {
				for (int a = tid; a < kq; a += PK_THREADS) {
					double s = 0.0;
					for (int j = 0; j < t; ++j) s = __builtin_fma(coef[j], basis[(int64_t)j * kq + a], s);
					v[a] -= s;
				}
			}
			__syncthreads();
		}
		double s = 0.0;
		for (int a = tid; a < kq; a += PK_THREADS) s = __builtin_fma(v[a], v[a], s);
		scr[tid] = s;
		const double nrm2 = pk_tree_sum(scr, tid);
		stop = !(nrm2 > 0.0 && nrm2 < INFINITY);   // (cannot happen while d tracks the residual to 2^-44: a guard against writing a non-finite q_t)
		if (!stop) {
			const double nrm = sqrt(nrm2);
			for (int a = tid; a < kq; a += PK_THREADS) basis[(int64_t)t * kq + a] = v[a] / nrm;
		}
	}
	if (tid != 0) return;
	if (stop) {
		hdr->stopped = 1;
		if (t == 0) hdr->d_first = 0.0;
		*n_sel = t;
		out_ids[t] = -1;
		out_gain[t] = 0.0;
	} else {
		if (t == 0) {
			hdr->stopped = 0;
			hdr->d_first = dp;
		}
		*n_sel = t + 1;
		out_ids[t] = p;
		out_gain[t] = dp;
		d[p] = __longlong_as_double(0x7ff8000000000000ll);   // taken
	}
}

bool pivot_shape_ok(int64_t m, int64_t kq, int64_t k) {
	return kq >= 1 && kq <= ANNCUR_LSTSQ_MAX_KQ && m >= 1 && m < (int64_t)0x80000000ll && k >= 1 && k <= kq && k <= m && k <= ANNCUR_MAX_TOPK;
}
int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }
int64_t pivot_slices(int64_t m, int dtype) { return ceil_div64(m, (int64_t)PV_THREADS * (dtype == ANNCUR_F32 ? PvVec<float>::N : PvVec<uint16_t>::N)); }
int64_t pivot_parts(int64_t m) { const int64_t ns = pivot_slices(m, ANNCUR_F32); return ns < PV_MAX_WG ? ns : PV_MAX_WG; }   // (the larger of the two dtypes' counts)

template <typename T>
int pivot_launch(const T *R, int64_t ldr, int kq, int64_t m, int k, int32_t *out_ids, double *out_gain, int32_t *n_sel, unsigned char *ws, hipStream_t st) {
	PvHeader *hdr = (PvHeader *)ws;
	double *d = (double *)(ws + PV_HDR_BYTES);
	double *basis = (double *)(ws + PV_HDR_BYTES + up256(m * 8));
	PvMax *parts = (PvMax *)(ws + PV_HDR_BYTES + up256(m * 8) + up256((int64_t)k * kq * 8));
	const int64_t nslices = ceil_div64(m, (int64_t)PV_THREADS * PvVec<T>::N);
	const unsigned grid = (unsigned)(nslices < PV_MAX_WG ? nslices : PV_MAX_WG);
	const bool aligned = ((uintptr_t)R & 15) == 0 && ((ldr * (int64_t)sizeof(T)) & 15) == 0;
	const size_t q_lds = (size_t)kq * sizeof(double);
	if (aligned) hipLaunchKernelGGL((pivot_step_kernel<T, true, true>), dim3(grid), dim3(PV_THREADS), 0, st, R, ldr, kq, m, nslices, (const double *)nullptr, (const PvHeader *)hdr, d, parts);
	else hipLaunchKernelGGL((pivot_step_kernel<T, true, false>), dim3(grid), dim3(PV_THREADS), 0, st, R, ldr, kq, m, nslices, (const double *)nullptr, (const PvHeader *)hdr, d, parts);
	for (int t = 0; t < k; ++t) {
		const size_t lds = (size_t)(kq + t + PK_THREADS) * sizeof(double) + (size_t)PK_THREADS * sizeof(int32_t);
		hipLaunchKernelGGL((pivot_pick_kernel<T>), dim3(1), dim3(PK_THREADS), lds, st, R, ldr, kq, t, (int)grid, (const PvMax *)parts, hdr, d, basis, out_ids, out_gain, n_sel);
		if (t + 1 == k) break;
		const double *qrow = basis + (int64_t)t * kq;
		if (aligned) hipLaunchKernelGGL((pivot_step_kernel<T, false, true>), dim3(grid), dim3(PV_THREADS), q_lds, st, R, ldr, kq, m, nslices, qrow, (const PvHeader *)hdr, d, parts);
		else hipLaunchKernelGGL((pivot_step_kernel<T, false, false>), dim3(grid), dim3(PV_THREADS), q_lds, st, R, ldr, kq, m, nslices, qrow, (const PvHeader *)hdr, d, parts);
	}
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

}  // namespace

extern "C" int32_t anncur_select_pivoted_slice_items(int dtype) {
	if (!dtype_ok(dtype)) return 0;
	return PV_THREADS * (dtype == ANNCUR_F32 ? PvVec<float>::N : PvVec<uint16_t>::N);
}

extern "C" size_t anncur_select_pivoted_workspace_bytes(int64_t m, int32_t kq, int32_t k) {
	if (!pivot_shape_ok(m, kq, k)) return 0;
	return (size_t)(PV_HDR_BYTES + up256(m * 8) + up256((int64_t)k * kq * 8) + up256(pivot_parts(m) * (int64_t)sizeof(PvMax)));
}

extern "C" int anncur_select_pivoted(const void *R, int dtype, int64_t ldr, int32_t kq, int64_t m, int32_t k, int32_t *out_ids, double *out_gain, int32_t *n_sel,
									 void *workspace, size_t workspace_bytes, void *stream) {
	ANNCUR_REQUIRE(pivot_shape_ok(m, kq, k), ANNCUR_E_INVALID,
				   "select_pivoted: need 1 <= k <= min(kq, m, ANNCUR_MAX_TOPK) = min(%d, %lld, %d), 1 <= kq <= %d and m < 2^31 (got k = %d, kq = %d, m = %lld)", (int)kq,
				   (long long)m, ANNCUR_MAX_TOPK, ANNCUR_LSTSQ_MAX_KQ, (int)k, (int)kq, (long long)m);
	ANNCUR_REQUIRE(dtype_ok(dtype), ANNCUR_E_INVALID, "select_pivoted: dtype must be ANNCUR_F32 or ANNCUR_BF16 (got %d)", dtype);
	ANNCUR_REQUIRE(ldr >= m, ANNCUR_E_INVALID, "select_pivoted: the row pitch ldr = %lld is shorter than the row of m = %lld", (long long)ldr, (long long)m);
	ANNCUR_REQUIRE(R && out_ids && out_gain && n_sel, ANNCUR_E_INVALID, "select_pivoted: null pointer");
	const size_t need = anncur_select_pivoted_workspace_bytes(m, kq, k);
	ANNCUR_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 255) == 0, ANNCUR_E_WORKSPACE,
				   "select_pivoted: workspace missing, misaligned (256 bytes) or too small (%zu < %zu bytes)", workspace_bytes, need);
	hipStream_t st = (hipStream_t)stream;
	if (dtype == ANNCUR_F32) return pivot_launch<float>((const float *)R, ldr, kq, m, k, out_ids, out_gain, n_sel, (unsigned char *)workspace, st);
	return pivot_launch<uint16_t>((const uint16_t *)R, ldr, kq, m, k, out_ids, out_gain, n_sel, (unsigned char *)workspace, st);
}
