// Sparse inner-product search: S = Xq . Xi^T for CSR queries against a term-major (inverted) item index, then the exact scan.
//   tfidf evaluation method                   eval/run_retrieval_eval_wrt_exact_crossenc_w_fixed_train_test_splits.py:360-385
//   TF-IDF hard-negative mining                utils/data_process.py:373-397 ; utils/compute_tfidf_hard_negs.py
//
// sparse_score_kernel.  The score of (q, i) is ONE fp32 chain over the terms the two share, in ascending term order, from +0.0f, product and
// sum rounded separately (sp_step below, compiled with contraction off).  No floating-point atomics: every (query, item) pair has one owner.
//  * A workgroup of four waves serves one query; its (term, weight) list is staged once in LDS (at most ANNCUR_SPARSE_MAX_QNNZ terms).
//  * A wave owns a span of consecutive windows of ANNCUR_SPARSE_WINDOW = 2048 items and keeps private fp32 accumulators for the current
//    window in LDS, plus two words per query term: `cur`, the position inside the term's posting list of its first posting at or past the
//    window, and `nxt`, the item of that posting (0xffffffff when the list is exhausted).
//  * Span start: lane j finds cur / nxt of term j by a lower bound on post_item, 64 terms per pass.  These are the only dependent-load chains.
//  * Per window, 64 terms per pass: nxt < window end is a ballot, and its set bits are taken in ascending order.  For such a term the lanes
//    read the next 64 postings at the cursor; those inside the window do acc[item - base] += w . v.  The items of one term are distinct, so
//    no two lanes touch one address; the LDS operations of one wave execute in order, so the next term sees the sums.  The cursor advances
//    by the count, which also finds the next window's start: there is no second search.
//  * Window end: 2048 scores as 16-byte stores, 32 group maxima (64 items each, fmaxf from NaN as few_score_kernel's GM), accumulators
//    back to +0.0f.
// After the query stage there is no workgroup barrier.  Safety: a term id outside [0, V) is never looked up, a list length is clamped to
// [0, I], a posting contributes only with (uint32)(item - base) < window length, a query's length is clamped to the stage.
//
// LDS: 8 KB of staged query + 4 x (8 KB accumulators + 4 KB cur + 4 KB nxt) = 72 KB per workgroup: two workgroups, eight waves per CU.
//
// Selection is anncur_rowwise_topk on the score rows (no selector of its own): see include/anncur_hip.h.
#include "common.hpp"

// The contract is a product and a sum with a rounding each.  __fmul_rn / __fadd_rn do not keep hipcc from fusing the pair: they are inline
// functions of a header compiled with contraction allowed, and after inlining the update became one v_fmac_f32 -- one rounding instead of
// two, a third of the scores off by an ulp.  So contraction is switched off for this file and the step is written with plain operators,
// which carry this file's setting (the build's disassembly shows v_mul_f32 + v_add_f32).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float sp_step(float acc, float w, float v) {
	const float prod = w * v;   // rounded
	return acc + prod;          // rounded again
}

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int SP_WINDOW = ANNCUR_SPARSE_WINDOW;        // items per window of accumulators
constexpr int SP_WAVES = 4;                            // waves per workgroup (all of one query)
constexpr int SP_MAX_WAVES = 2048;                     // waves of a launch: eight per CU on 256 CUs (a host constant: the plan needs no device)
constexpr int SP_QNNZ = ANNCUR_SPARSE_MAX_QNNZ;        // staged query terms
constexpr int SP_GROUP = 64;                           // items per group maximum
constexpr uint32_t SP_NONE = 0xffffffffu;              // nxt of an exhausted (or unusable) posting list
constexpr int SP_LDS_BYTES = SP_QNNZ * 8 + SP_WAVES * (SP_WINDOW * 4 + SP_QNNZ * 8);
static_assert(SP_WINDOW == 2048 && SP_WINDOW % (4 * WAVE) == 0 && SP_QNNZ % WAVE == 0, "the epilogue reads 256 items per pass");
static_assert(SP_LDS_BYTES == 73728, "include/anncur_hip.h states the LDS account");

struct SparsePlan {
	bool ok;
	int64_t windows, wpw, spans, wg_per_query, workgroups, groups, pitch;
};

// shape -> launch geometry (host only)
SparsePlan sparse_plan_of(int64_t Q, int64_t I) {
	SparsePlan P{};
	if (Q < 1 || I < 1 || I >= (int64_t)0x7fffffff) return P;
	P.windows = ceil_div64(I, SP_WINDOW);
	P.groups = ceil_div64(I, SP_GROUP);
	P.pitch = ceil_div64(I, 32) * 32;
	// windows per wave: about SP_MAX_WAVES waves in all, never less than one window
	const int64_t units_hi = P.windows > ((int64_t)1 << 40) / Q ? (int64_t)1 << 40 : Q * P.windows;
	P.wpw = ceil_div64(units_hi, SP_MAX_WAVES);
	if (P.wpw > P.windows) P.wpw = P.windows;
	P.spans = ceil_div64(P.windows, P.wpw);
	P.wg_per_query = ceil_div64(P.spans, SP_WAVES);
	if (P.wg_per_query > (int64_t)0x7fffffff / Q) return P;
	P.workgroups = Q * P.wg_per_query;
	P.ok = true;
	return P;
}

struct SparseArgs {
	const int64_t *q_ptr;
	const int32_t *q_term;
	const float *q_val;
	const int64_t *term_ptr;
	const int32_t *post_item;
	const float *post_val;
	uint32_t V, I, wpw, wg_per_query;
	float *S;
	int64_t lds;
	float *GM;
	int64_t ldg;
	int vec_ok;   // S + q lds is 16-byte aligned for every q
};

// the posting list of term t: its start in post_item / post_val and its length, clamped to [0, I] (a canonical list holds each item once)
__device__ __forceinline__ uint32_t sp_list(const SparseArgs &p, uint32_t t, int64_t &start) {
	start = p.term_ptr[t];
	int64_t len = p.term_ptr[t + 1] - start;
	len = len < 0 ? 0 : (len > (int64_t)p.I ? (int64_t)p.I : len);
	return start < 0 ? 0u : (uint32_t)len;
}

__global__ __launch_bounds__(SP_WAVES * 64) void sparse_score_kernel(const SparseArgs p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	int32_t *const qterm = reinterpret_cast<int32_t *>(smem);
	float *const qval = reinterpret_cast<float *>(smem + SP_QNNZ * 4);
	unsigned char *const mine = smem + SP_QNNZ * 8 + wave * (SP_WINDOW * 4 + SP_QNNZ * 8);
	float *const acc = reinterpret_cast<float *>(mine);
	uint32_t *const cur = reinterpret_cast<uint32_t *>(mine + SP_WINDOW * 4);
	uint32_t *const nxt = cur + SP_QNNZ;

	const int64_t q = blockIdx.x / p.wg_per_query;
	const uint32_t wg = blockIdx.x % p.wg_per_query;

	// ---- the query, once per workgroup
	const int64_t qs = p.q_ptr[q];
	int64_t nq64 = p.q_ptr[q + 1] - qs;
	nq64 = nq64 < 0 ? 0 : (nq64 > SP_QNNZ ? SP_QNNZ : nq64);
	const uint32_t nq = (uint32_t)nq64;
	for (uint32_t i = tid; i < nq; i += SP_WAVES * 64) {
		qterm[i] = p.q_term[qs + i];
		qval[i] = p.q_val[qs + i];
	}
	for (uint32_t i = lane; i < SP_WINDOW; i += 64) acc[i] = 0.f;
	__syncthreads();

	// ---- this wave's span of windows
	const int64_t span = (int64_t)wg * SP_WAVES + wave;
	const int64_t lo64 = span * p.wpw * SP_WINDOW;
	if (lo64 >= (int64_t)p.I) return;
	const uint32_t span_lo = (uint32_t)lo64;
	const uint32_t span_hi = lo64 + (int64_t)p.wpw * SP_WINDOW < (int64_t)p.I ? (uint32_t)(lo64 + (int64_t)p.wpw * SP_WINDOW) : p.I;

	// ---- cursors: lane j searches term j's list for the first posting at or past span_lo
	for (uint32_t t0 = 0; t0 < nq; t0 += 64) {
		const uint32_t j = t0 + lane;
		if (j < nq) {
			const uint32_t t = (uint32_t)qterm[j];
			uint32_t c = 0, first = SP_NONE;
			if (t < p.V) {
				int64_t start;
				const uint32_t len = sp_list(p, t, start);
				uint32_t hi = span_lo == 0u ? 0u : len;
				while (c < hi) {
					const uint32_t mid = c + ((hi - c) >> 1);
					if ((uint32_t)p.post_item[start + mid] < span_lo) c = mid + 1u;
					else hi = mid;
				}
				if (c < len) first = (uint32_t)p.post_item[start + c];
			}
			cur[j] = c;
			nxt[j] = first;
		}
	}

	float *const Srow = p.S + q * p.lds;
	for (uint32_t base = span_lo; base < span_hi; base += SP_WINDOW) {
		const uint32_t wlen = span_hi - base < (uint32_t)SP_WINDOW ? span_hi - base : (uint32_t)SP_WINDOW;
		const uint32_t wend = base + wlen;

		// ---- the terms with a posting in the window, ascending
		for (uint32_t t0 = 0; t0 < nq; t0 += 64) {
			const uint32_t j = t0 + lane;
			unsigned long long todo = __ballot(j < nq && nxt[j] < wend);
			while (todo != 0ull) {   // (uniform)
				const uint32_t jt = t0 + (uint32_t)(__ffsll((long long)todo) - 1);
				todo &= todo - 1ull;
				const uint32_t t = (uint32_t)qterm[jt];
				const float w = qval[jt];
				int64_t start;
				const uint32_t len = sp_list(p, t, start);
				uint32_t c = cur[jt];
				for (;;) {
					const uint32_t pos = c + lane;
					const bool in = pos < len;
					const uint32_t item = in ? (uint32_t)p.post_item[start + pos] : SP_NONE;
					const float v = in ? p.post_val[start + pos] : 0.f;
					const bool hit = in && item - base < wlen;
					if (hit) acc[item - base] = sp_step(acc[item - base], w, v);
					const uint32_t cnt = (uint32_t)__popcll(__ballot(hit));
					c += cnt;
					if (cnt < 64u) {
						if (lane == cnt) nxt[jt] = item;   // the first posting past the window (SP_NONE at the end of the list)
						break;
					}
				}
				if (lane == 0u) cur[jt] = c;
				__builtin_amdgcn_wave_barrier();
			}
		}

		// ---- the window's scores and group maxima; the accumulators start the next window from zero
		for (uint32_t r0 = 0; r0 < wlen; r0 += 4 * 64) {
			const uint32_t off = r0 + 4u * lane;
			const f32x4 v = *reinterpret_cast<const f32x4 *>(acc + off);
			*reinterpret_cast<f32x4 *>(acc + off) = (f32x4){0.f, 0.f, 0.f, 0.f};
			const uint32_t item0 = base + off;
			float m = __uint_as_float(0x7fc00000u);
			if (item0 + 3u < wend) {
				if (p.vec_ok) *reinterpret_cast<f32x4 *>(Srow + item0) = v;
				else {
#pragma unroll
					for (int r = 0; r < 4; ++r) Srow[item0 + (uint32_t)r] = v[r];
				}
				m = fmaxf(fmaxf(fmaxf(fmaxf(m, v[0]), v[1]), v[2]), v[3]);
			} else {
#pragma unroll
				for (int r = 0; r < 4; ++r)
					if (item0 + (uint32_t)r < wend) {
						Srow[item0 + (uint32_t)r] = v[r];
						m = fmaxf(m, v[r]);
					}
			}
			if (p.GM) {   // (uniform) sixteen lanes hold one group of 64 items
				m = fmaxf(m, __shfl_xor(m, 1));
				m = fmaxf(m, __shfl_xor(m, 2));
				m = fmaxf(m, __shfl_xor(m, 4));
				m = fmaxf(m, __shfl_xor(m, 8));
				if ((lane & 15u) == 0u && item0 < wend) p.GM[q * p.ldg + (item0 >> 6)] = m;
			}
		}
	}
}

int launch_sparse_score(const SparsePlan &P, const int64_t *q_ptr, const int32_t *q_term, const float *q_val, const int64_t *term_ptr, const int32_t *post_item,
						const float *post_val, int64_t V, int64_t I, float *S, int64_t lds, float *GM, int64_t ldg, hipStream_t st) {
	SparseArgs a;
	a.q_ptr = q_ptr; a.q_term = q_term; a.q_val = q_val; a.term_ptr = term_ptr; a.post_item = post_item; a.post_val = post_val;
	a.V = (uint32_t)V; a.I = (uint32_t)I; a.wpw = (uint32_t)P.wpw; a.wg_per_query = (uint32_t)P.wg_per_query;
	a.S = S; a.lds = lds; a.GM = GM; a.ldg = ldg;
	a.vec_ok = ((uintptr_t)S % 16) == 0 && (lds % 4) == 0;
	const int rc = anncur_ensure_dyn_lds((const void *)sparse_score_kernel, SP_LDS_BYTES);
	if (rc != ANNCUR_OK) return rc;
	hipLaunchKernelGGL(sparse_score_kernel, dim3((unsigned)P.workgroups), dim3(SP_WAVES * 64), SP_LDS_BYTES, st, a);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

int sparse_check(const char *what, const SparsePlan &P, const void *q_ptr, const void *term_ptr, int64_t Q, int64_t V, int64_t I) {
	ANNCUR_REQUIRE(I >= 1 && I < (int64_t)0x7fffffff, ANNCUR_E_INVALID, "%s: I = %lld items is outside 1..2^31 - 2", what, (long long)I);
	ANNCUR_REQUIRE(V >= 0 && V < ((int64_t)1 << 31), ANNCUR_E_INVALID, "%s: V = %lld terms is outside 0..2^31 - 1", what, (long long)V);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_UNSUPPORTED, "%s: Q = %lld queries on I = %lld items need more than 2^31 - 1 workgroups: search in chunks", what, (long long)Q,
				   (long long)I);
	ANNCUR_REQUIRE(q_ptr && term_ptr, ANNCUR_E_INVALID, "%s: null q_ptr or term_ptr", what);
	return ANNCUR_OK;
}

}  // namespace

extern "C" int anncur_sparse_plan(int64_t Q, int64_t I, int32_t *out, int32_t n_out) {
	ANNCUR_REQUIRE(out && n_out >= 1, ANNCUR_E_INVALID, "sparse_plan: need an output array");
	const SparsePlan P = sparse_plan_of(Q, I);
	ANNCUR_REQUIRE(P.ok, ANNCUR_E_INVALID, "sparse_plan: (Q=%lld, I=%lld) is outside Q >= 1, 1 <= I < 2^31 - 1, Q x workgroups per query < 2^31", (long long)Q,
				   (long long)I);
	const int32_t w[ANNCUR_SPARSE_PLAN_WORDS] = {(int32_t)P.windows, (int32_t)P.wpw, (int32_t)P.spans, (int32_t)P.wg_per_query, (int32_t)P.workgroups, SP_WAVES,
												 SP_LDS_BYTES, (int32_t)(P.pitch / 32), (int32_t)P.groups, SP_QNNZ};
	for (int i = 0; i < n_out && i < ANNCUR_SPARSE_PLAN_WORDS; ++i) out[i] = w[i];
	return ANNCUR_OK;
}

extern "C" int anncur_sparse_score_rows(const int64_t *q_ptr, const int32_t *q_term, const float *q_val, int64_t Q, const int64_t *term_ptr, const int32_t *post_item,
										 const float *post_val, int64_t V, int64_t I, float *S, int64_t lds, float *GM, int64_t ldg, void *stream) {
	ANNCUR_REQUIRE(Q >= 0, ANNCUR_E_INVALID, "sparse_score_rows: Q = %lld", (long long)Q);
	if (Q == 0) return ANNCUR_OK;
	const SparsePlan P = sparse_plan_of(Q, I);
	if (const int rc = sparse_check("sparse_score_rows", P, q_ptr, term_ptr, Q, V, I)) return rc;
	ANNCUR_REQUIRE(S && lds >= I, ANNCUR_E_INVALID, "sparse_score_rows: S must be non-null with lds >= I (got %lld)", (long long)lds);
	ANNCUR_REQUIRE(!GM || ldg >= P.groups, ANNCUR_E_INVALID, "sparse_score_rows: ldg = %lld is shorter than the %lld groups of 64 items", (long long)ldg,
				   (long long)P.groups);
	return launch_sparse_score(P, q_ptr, q_term, q_val, term_ptr, post_item, post_val, V, I, S, lds, GM, ldg, (hipStream_t)stream);
}

extern "C" size_t anncur_sparse_score_topk_workspace_bytes(int64_t Q, int64_t I, int32_t k) {
	const SparsePlan P = sparse_plan_of(Q, I);
	if (!P.ok || k < 1 || k > ANNCUR_MAX_TOPK || (int64_t)k > I) return 0;
	return (size_t)Q * (size_t)P.pitch * 4;
}

extern "C" int anncur_sparse_score_topk(const int64_t *q_ptr, const int32_t *q_term, const float *q_val, int64_t Q, const int64_t *term_ptr, const int32_t *post_item,
										 const float *post_val, int64_t V, int64_t I, int32_t k, float *out_val, int32_t *out_idx, void *workspace, size_t workspace_bytes,
										 void *stream) {
	ANNCUR_REQUIRE(Q >= 0, ANNCUR_E_INVALID, "sparse_score_topk: Q = %lld", (long long)Q);
	ANNCUR_REQUIRE(I >= 1 && k >= 1 && k <= ANNCUR_MAX_TOPK && (int64_t)k <= I, ANNCUR_E_INVALID, "sparse_score_topk: k = %d is outside 1..min(I = %lld, %d)", k,
				   (long long)I, ANNCUR_MAX_TOPK);
	if (Q == 0) return ANNCUR_OK;
	const SparsePlan P = sparse_plan_of(Q, I);
	if (const int rc = sparse_check("sparse_score_topk", P, q_ptr, term_ptr, Q, V, I)) return rc;
	ANNCUR_REQUIRE(out_val && out_idx, ANNCUR_E_INVALID, "sparse_score_topk: null output pointer");
	const size_t need = (size_t)Q * (size_t)P.pitch * 4;
	ANNCUR_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace % 256) == 0, ANNCUR_E_WORKSPACE,
				   "sparse_score_topk: workspace of %zu bytes (256-byte aligned) required, got %zu", need, workspace_bytes);
	float *S = reinterpret_cast<float *>(workspace);
	const int rc = launch_sparse_score(P, q_ptr, q_term, q_val, term_ptr, post_item, post_val, V, I, S, P.pitch, nullptr, 0, (hipStream_t)stream);
	if (rc != ANNCUR_OK) return rc;
	return anncur_rowwise_topk(S, ANNCUR_F32, Q, I, P.pitch, k, out_val, out_idx, stream);
}
