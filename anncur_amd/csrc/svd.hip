// One-sided (Hestenes) Jacobi SVD of ONE matrix in fp64 and the column scaling of the truncated pseudo-inverse built on it.
// include/anncur_hip.h has the contract (the schedule, the rotation, the tolerance, the order of every sum).  The working set lives in the
// caller's workspace, all fp64:
//   H   [g x Lp]   row i = short-side vector i of W (a column of W if rows >= cols, else a row), widened exactly, contiguous
//   Vt  [g x gp]   starts as the identity; row i receives every rotation H's row i receives, so H_final = Vt . H_0
// g = min(rows, cols), L = max(rows, cols), both pitches rounded up to 32 doubles; the pad is never written and never read.
// A sweep is gE - 1 launches (gE = g rounded up to even) of svd_pair_kernel, one workgroup per pair of the round-robin tournament.  The pairs
// of one step own disjoint rows and the kernel boundary orders the steps: no workgroup waits for another, nothing is launched cooperatively,
// every loop is bounded by L or g.
// A pair's three sums (|h_i|^2, |h_j|^2, h_i.h_j) have ONE order, fixed by L alone: thread t takes the elements t, t + 256, ... by fma in
// ascending order, the 64 lanes of a wave are combined by the xor butterfly 32, 16, .., 1 (every lane ends with the same bits), the four
// waves' values are added in wave order from LDS.  No floating-point atomics; the one atomic is the integer rotation count.
#include "common.hpp"

namespace {

constexpr int SV_THREADS = 256;
constexpr int SV_WAVES = SV_THREADS / WAVE;
constexpr int SV_EPT = 8;                           // elements of each row a thread keeps in registers between the dot pass and the update
constexpr int SV_REG_L = SV_THREADS * SV_EPT;       // ... which covers L <= 2048: 2 x 8 doubles = 32 VGPRs; longer rows are read a second time
constexpr int SV_PITCH = 32;                        // doubles: every row of H and Vt starts on a 256-byte boundary

struct SvGeom {
	int g, L, gE;
	bool tall;          // rows >= cols: the vectors are W's columns
	int64_t Lp, gp;
	size_t vt_off, bytes;
};

bool svd_shape_ok(int64_t rows, int64_t cols) {
	const int64_t g = rows < cols ? rows : cols, L = rows < cols ? cols : rows;
	return g >= 1 && g <= ANNCUR_SVD_MAX_G && L <= ANNCUR_SVD_MAX_L;
}

SvGeom svd_geom(int64_t rows, int64_t cols) {
	SvGeom q;
	q.tall = rows >= cols;
	q.g = (int)(q.tall ? cols : rows);
	q.L = (int)(q.tall ? rows : cols);
	q.gE = (q.g + 1) & ~1;
	q.Lp = ((int64_t)q.L + SV_PITCH - 1) / SV_PITCH * SV_PITCH;
	q.gp = ((int64_t)q.g + SV_PITCH - 1) / SV_PITCH * SV_PITCH;
	q.vt_off = (size_t)q.g * (size_t)q.Lp * sizeof(double);
	q.bytes = q.vt_off + (size_t)q.g * (size_t)q.gp * sizeof(double);
	return q;
}

// (a, b, c) summed over the workgroup in the fixed order described at the top -> the same bits in every thread.  scr: [3 x SV_WAVES] doubles of LDS.
__device__ __forceinline__ void sv_block_sum3(double &a, double &b, double &c, double *scr) {
#pragma unroll
	for (int x = 32; x > 0; x >>= 1) {
		a += __shfl_xor(a, x);
		b += __shfl_xor(b, x);
		c += __shfl_xor(c, x);
	}
	const int wave = threadIdx.x >> 6;
	__syncthreads();   // (the previous use of scr is over)
	if (lane_id() == 0) {
		scr[wave] = a;
		scr[SV_WAVES + wave] = b;
		scr[2 * SV_WAVES + wave] = c;
	}
	__syncthreads();
	a = scr[0];
	b = scr[SV_WAVES];
	c = scr[2 * SV_WAVES];
#pragma unroll
	for (int w = 1; w < SV_WAVES; ++w) {
		a += scr[w];
		b += scr[SV_WAVES + w];
		c += scr[2 * SV_WAVES + w];
	}
}

// H[i, l] = the element of W that belongs to vector i, position l.  TALL: W[l, i] (a 32 x 32 tile turned through LDS so that both the read and
// the write run along contiguous memory); otherwise W[i, l].  Grid: (ceil(L / 32), ceil(g / 32)), 32 x 8 threads.
template <typename T, bool TALL>
__global__ __launch_bounds__(SV_THREADS) void svd_widen_kernel(const T *__restrict__ W, int64_t ldw, int g, int L, double *__restrict__ H, int64_t Lp) {
	__shared__ double tile[32][33];
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	const int l0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
	if (TALL) {
		for (int r = ty; r < 32; r += 8) {
			const int l = l0 + r, i = i0 + tx;
			tile[r][tx] = (l < L && i < g) ? (double)load_as_f32<T>(W + (int64_t)l * ldw + i) : 0.0;
		}
		__syncthreads();
		for (int r = ty; r < 32; r += 8) {
			const int i = i0 + r, l = l0 + tx;
			if (i < g && l < L) H[(int64_t)i * Lp + l] = tile[tx][r];
		}
	} else {
		for (int r = ty; r < 32; r += 8) {
			const int i = i0 + r, l = l0 + tx;
			if (i < g && l < L) H[(int64_t)i * Lp + l] = (double)load_as_f32<T>(W + (int64_t)i * ldw + l);
		}
	}
}

// Vt = I on its [g x g] part.  Grid: (ceil(g / 256), g).
__global__ __launch_bounds__(SV_THREADS) void svd_identity_kernel(double *__restrict__ Vt, int64_t gp, int g) {
	const int i = blockIdx.y, k = blockIdx.x * SV_THREADS + threadIdx.x;
	if (k < g) Vt[(int64_t)i * gp + k] = k == i ? 1.0 : 0.0;
}

// One step of a sweep: workgroup p orthogonalises its pair.  REG: L <= SV_REG_L, the elements stay in registers between the two passes.
template <bool REG>
__global__ __launch_bounds__(SV_THREADS) void svd_pair_kernel(double *__restrict__ H, int64_t Lp, int L, double *__restrict__ Vt, int64_t gp, int g, int gE, int step,
															   double tol, int32_t *__restrict__ rotations) {
	__shared__ double scr[3 * SV_WAVES];
	const int tid = threadIdx.x, p = blockIdx.x, n1 = gE - 1;
	const int a = p == 0 ? gE - 1 : (step + p) % n1;
	const int b = p == 0 ? step : (step - p + n1) % n1;
	const int i = a < b ? a : b, j = a < b ? b : a;
	if (j >= g) return;   // (the dummy index of an odd g; the same in every thread)
	double *hi = H + (int64_t)i * Lp, *hj = H + (int64_t)j * Lp;
	double xi[REG ? SV_EPT : 1], xj[REG ? SV_EPT : 1];
	double alpha = 0.0, beta = 0.0, gamma = 0.0;
	if (REG) {
#pragma unroll
		for (int e = 0; e < SV_EPT; ++e) {
			const int l = tid + e * SV_THREADS;
			xi[e] = l < L ? hi[l] : 0.0;
			xj[e] = l < L ? hj[l] : 0.0;
		}
#pragma unroll
		for (int e = 0; e < SV_EPT; ++e) {   // (a zero beyond L adds nothing: the sums are those of the elements below L, in ascending order)
			alpha = __builtin_fma(xi[e], xi[e], alpha);
			beta = __builtin_fma(xj[e], xj[e], beta);
			gamma = __builtin_fma(xi[e], xj[e], gamma);
		}
	} else {
		for (int l = tid; l < L; l += SV_THREADS) {
			const double u = hi[l], v = hj[l];
			alpha = __builtin_fma(u, u, alpha);
			beta = __builtin_fma(v, v, beta);
			gamma = __builtin_fma(u, v, gamma);
		}
	}
	sv_block_sum3(alpha, beta, gamma, scr);
	// dgesvj's tolerance; sqrt(alpha) sqrt(beta) instead of sqrt(alpha beta): the product of two squared norms can leave the fp64 range
	if (!(alpha > 0.0 && beta > 0.0 && fabs(gamma) > tol * (sqrt(alpha) * sqrt(beta)))) return;   // (uniform: every thread holds the same sums)
	const double zeta = (beta - alpha) / (2.0 * gamma);
	const double az = fabs(zeta);
	double t;
	if (az == 0.0) t = 1.0;
	else if (az > 0x1p500) t = 0.5 / zeta;   // (1 + zeta^2 would round to zeta^2 long before it overflows: the same value, without the overflow)
	else t = (zeta < 0.0 ? -1.0 : 1.0) / (az + sqrt(1.0 + zeta * zeta));
	const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
	if (REG) {
#pragma unroll
		for (int e = 0; e < SV_EPT; ++e) {
			const int l = tid + e * SV_THREADS;
			if (l < L) {
				hi[l] = c * xi[e] - s * xj[e];
				hj[l] = s * xi[e] + c * xj[e];
			}
		}
	} else {
		for (int l = tid; l < L; l += SV_THREADS) {
			const double u = hi[l], v = hj[l];
			hi[l] = c * u - s * v;
			hj[l] = s * u + c * v;
		}
	}
	double *vi = Vt + (int64_t)i * gp, *vj = Vt + (int64_t)j * gp;
	for (int k = tid; k < g; k += SV_THREADS) {
		const double u = vi[k], v = vj[k];
		vi[k] = c * u - s * v;
		vj[k] = s * u + c * v;
	}
	if (tid == 0) atomicAdd(rotations, 1);
}

// Workgroup i: sigma_i = |h_i| (the sum in the pair kernel's order), h_i / sigma_i (zeros where sigma_i = 0) and row i of Vt, each written as
// column i of its output: `long_out` [L x g] takes the normalised vector, `short_out` [g x g] the row of Vt.
__global__ __launch_bounds__(SV_THREADS) void svd_finish_kernel(const double *__restrict__ H, int64_t Lp, int L, const double *__restrict__ Vt, int64_t gp, int g,
																 double *__restrict__ sigma, double *__restrict__ long_out, int64_t ld_long, double *__restrict__ short_out,
																 int64_t ld_short, int32_t *__restrict__ flag) {
	__shared__ double scr[3 * SV_WAVES];
	const int tid = threadIdx.x, i = blockIdx.x;
	const double *h = H + (int64_t)i * Lp, *v = Vt + (int64_t)i * gp;
	double n2 = 0.0, z0 = 0.0, z1 = 0.0;
	for (int l = tid; l < L; l += SV_THREADS) n2 = __builtin_fma(h[l], h[l], n2);
	sv_block_sum3(n2, z0, z1, scr);
	const double sg = sqrt(n2);
	if (tid == 0) {
		sigma[i] = sg;
		if (!(fabs(sg) < INFINITY)) *flag = 1;   // (NaN or inf; every workgroup that finds one writes the same 1)
	}
	for (int l = tid; l < L; l += SV_THREADS) long_out[(int64_t)l * ld_long + i] = sg == 0.0 ? 0.0 : h[l] / sg;
	for (int k = tid; k < g; k += SV_THREADS) short_out[(int64_t)k * ld_short + i] = v[k];
}

// out[r, i] = V[r, i] / sigma[i] where sigma[i] > rcond max(sigma), else 0 (numpy.linalg.pinv's rule; a NaN sigma fails the test).  Workgroup r
// takes row r; every workgroup finds the maximum itself (g <= 2048 values; a maximum has no order to fix), workgroup 0 also counts the rank.
__global__ __launch_bounds__(SV_THREADS) void svd_scale_cols_kernel(const double *__restrict__ V, int64_t ldv, int g, const double *__restrict__ sigma, double rcond,
																	 double *__restrict__ out, int64_t ldo, int32_t *__restrict__ rank) {
	__shared__ double smax[SV_WAVES];
	__shared__ int32_t cnt[SV_WAVES];
	const int tid = threadIdx.x, wave = tid >> 6;
	double m = 0.0;
	for (int i = tid; i < g; i += SV_THREADS) {
		const double s = sigma[i];
		if (s > m) m = s;
	}
#pragma unroll
	for (int x = 32; x > 0; x >>= 1) {
		const double o = __shfl_xor(m, x);
		if (o > m) m = o;
	}
	if (lane_id() == 0) smax[wave] = m;
	__syncthreads();
	m = smax[0];
#pragma unroll
	for (int w = 1; w < SV_WAVES; ++w)
		if (smax[w] > m) m = smax[w];
	const double cutoff = rcond * m;
	const int64_t r = blockIdx.x;
	int32_t kept = 0;
	for (int i = tid; i < g; i += SV_THREADS) {
		const double s = sigma[i];
		const bool large = s > cutoff;
		kept += large ? 1 : 0;
		out[r * ldo + i] = large ? V[r * ldv + i] / s : 0.0;
	}
	if (r != 0) return;
#pragma unroll
	for (int x = 32; x > 0; x >>= 1) kept += __shfl_xor(kept, x);
	if (lane_id() == 0) cnt[wave] = kept;
	__syncthreads();
	if (tid == 0) {
		int32_t tot = 0;
		for (int w = 0; w < SV_WAVES; ++w) tot += cnt[w];
		*rank = tot;
	}
}

int svd_args_ok(const char *what, int64_t rows, int64_t cols, const void *ws, size_t ws_bytes, SvGeom *q) {
	ANNCUR_REQUIRE(svd_shape_ok(rows, cols), ANNCUR_E_INVALID, "%s: need 1 <= min(rows, cols) <= ANNCUR_SVD_MAX_G = %d and max(rows, cols) <= ANNCUR_SVD_MAX_L = %d (got %lld x %lld)",
				   what, ANNCUR_SVD_MAX_G, ANNCUR_SVD_MAX_L, (long long)rows, (long long)cols);
	*q = svd_geom(rows, cols);
	ANNCUR_REQUIRE(ws && ws_bytes >= q->bytes && ((uintptr_t)ws & 255) == 0, ANNCUR_E_WORKSPACE, "%s: workspace missing, misaligned (256 bytes) or too small (%zu < %zu bytes)", what,
				   ws_bytes, q->bytes);
	return ANNCUR_OK;
}

template <typename T>
void svd_widen_launch(const T *W, int64_t ldw, const SvGeom &q, double *H, hipStream_t st) {
	const dim3 grid((unsigned)((q.L + 31) / 32), (unsigned)((q.g + 31) / 32));
	if (q.tall) hipLaunchKernelGGL((svd_widen_kernel<T, true>), grid, dim3(SV_THREADS), 0, st, W, ldw, q.g, q.L, H, q.Lp);
	else hipLaunchKernelGGL((svd_widen_kernel<T, false>), grid, dim3(SV_THREADS), 0, st, W, ldw, q.g, q.L, H, q.Lp);
}

}  // namespace

extern "C" size_t anncur_svd_workspace_bytes(int64_t rows, int64_t cols) {
	if (!svd_shape_ok(rows, cols)) return 0;
	return svd_geom(rows, cols).bytes;
}

extern "C" int anncur_svd_init(const void *W, int dtype, int64_t ldw, int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, void *stream) {
	SvGeom q;
	const int rc = svd_args_ok("svd_init", rows, cols, workspace, workspace_bytes, &q);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_REQUIRE(dtype_ok(dtype), ANNCUR_E_INVALID, "svd_init: dtype must be ANNCUR_F32 or ANNCUR_BF16 (got %d)", dtype);
	ANNCUR_REQUIRE(W && ldw >= cols, ANNCUR_E_INVALID, "svd_init: null W or a row pitch ldw = %lld shorter than the row of %lld", (long long)ldw, (long long)cols);
	hipStream_t st = (hipStream_t)stream;
	double *H = (double *)workspace, *Vt = (double *)((unsigned char *)workspace + q.vt_off);
	if (dtype == ANNCUR_F32) svd_widen_launch<float>((const float *)W, ldw, q, H, st);
	else svd_widen_launch<uint16_t>((const uint16_t *)W, ldw, q, H, st);
	hipLaunchKernelGGL(svd_identity_kernel, dim3((unsigned)((q.g + SV_THREADS - 1) / SV_THREADS), (unsigned)q.g), dim3(SV_THREADS), 0, st, Vt, q.gp, q.g);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_svd_sweep(int64_t rows, int64_t cols, void *workspace, size_t workspace_bytes, int32_t *rotations, void *stream) {
	SvGeom q;
	const int rc = svd_args_ok("svd_sweep", rows, cols, workspace, workspace_bytes, &q);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_REQUIRE(rotations, ANNCUR_E_INVALID, "svd_sweep: null rotations");
	hipStream_t st = (hipStream_t)stream;
	double *H = (double *)workspace, *Vt = (double *)((unsigned char *)workspace + q.vt_off);
	const double tol = sqrt((double)q.L) * 0x1p-53;
	ANNCUR_TRY(anncur_fill_words_async(rotations, 0u, 1, st));
	for (int step = 0; step < q.gE - 1; ++step) {
		if (q.L <= SV_REG_L) hipLaunchKernelGGL((svd_pair_kernel<true>), dim3((unsigned)(q.gE / 2)), dim3(SV_THREADS), 0, st, H, q.Lp, q.L, Vt, q.gp, q.g, q.gE, step, tol, rotations);
		else hipLaunchKernelGGL((svd_pair_kernel<false>), dim3((unsigned)(q.gE / 2)), dim3(SV_THREADS), 0, st, H, q.Lp, q.L, Vt, q.gp, q.g, q.gE, step, tol, rotations);
	}
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_svd_finish(int64_t rows, int64_t cols, const void *workspace, size_t workspace_bytes, double *sigma, double *U, int64_t ldu, double *V, int64_t ldv,
								 int32_t *flag, void *stream) {
	SvGeom q;
	const int rc = svd_args_ok("svd_finish", rows, cols, workspace, workspace_bytes, &q);
	if (rc != ANNCUR_OK) return rc;
	ANNCUR_REQUIRE(sigma && U && V && flag, ANNCUR_E_INVALID, "svd_finish: null pointer");
	ANNCUR_REQUIRE(ldu >= q.g && ldv >= q.g, ANNCUR_E_INVALID, "svd_finish: ldu = %lld or ldv = %lld is shorter than a row of g = %d", (long long)ldu, (long long)ldv, q.g);
	hipStream_t st = (hipStream_t)stream;
	const double *H = (const double *)workspace, *Vt = (const double *)((const unsigned char *)workspace + q.vt_off);
	ANNCUR_TRY(anncur_fill_words_async(flag, 0u, 1, st));
	// rows >= cols: U [rows x g] = the normalised vectors, V [cols x g] = Vt^T; otherwise the roles swap
	double *long_out = q.tall ? U : V, *short_out = q.tall ? V : U;
	const int64_t ld_long = q.tall ? ldu : ldv, ld_short = q.tall ? ldv : ldu;
	hipLaunchKernelGGL(svd_finish_kernel, dim3((unsigned)q.g), dim3(SV_THREADS), 0, st, H, q.Lp, q.L, Vt, q.gp, q.g, sigma, long_out, ld_long, short_out, ld_short, flag);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_svd_scale_cols(const double *V, int64_t ldv, int64_t n, int32_t g, const double *sigma, double rcond, double *out, int64_t ldo, int32_t *rank, void *stream) {
	ANNCUR_REQUIRE(g >= 1 && g <= ANNCUR_SVD_MAX_G && n >= 1 && n <= ANNCUR_SVD_MAX_L, ANNCUR_E_INVALID,
				   "svd_scale_cols: need 1 <= g <= ANNCUR_SVD_MAX_G = %d and 1 <= n <= ANNCUR_SVD_MAX_L = %d (got g = %d, n = %lld)", ANNCUR_SVD_MAX_G, ANNCUR_SVD_MAX_L, (int)g, (long long)n);
	ANNCUR_REQUIRE(rcond >= 0.0 && rcond < 1.0, ANNCUR_E_INVALID, "svd_scale_cols: rcond = %g outside [0, 1)", rcond);
	ANNCUR_REQUIRE(V && sigma && out && rank && ldv >= g && ldo >= g, ANNCUR_E_INVALID, "svd_scale_cols: null pointer or a row pitch shorter than g = %d", (int)g);
	hipLaunchKernelGGL(svd_scale_cols_kernel, dim3((unsigned)n), dim3(SV_THREADS), 0, (hipStream_t)stream, V, ldv, (int)g, sigma, rcond, out, ldo, rank);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
