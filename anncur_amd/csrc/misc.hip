// Error reporting and device introspection for libanncur_hip.
#include <string.h>
#include <mutex>
#include <vector>
#include "common.hpp"

namespace {
thread_local char g_err[512] = "";
}

void anncur_set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

// hipFuncSetAttribute and the CU count belong to a DEVICE: both are remembered per (function, device) / per device, so a process
// that drives several GPUs (CURApprox(device=...), --device cuda:N) sets the > 64 KiB dynamic-LDS attribute on each of them.
namespace {
struct AttrEntry { const void *fn; int dev; int bytes; };
std::mutex g_attr_mu;
std::vector<AttrEntry> g_attr;
int g_cu[64] = {0};
}

int anncur_ensure_dyn_lds(const void *fn, int bytes) {
	int dev = 0;
	ANNCUR_HIP_OK(hipGetDevice(&dev));
	std::lock_guard<std::mutex> lock(g_attr_mu);
	for (auto &e : g_attr)
		if (e.fn == fn && e.dev == dev) {
			if (e.bytes >= bytes) return ANNCUR_OK;
			ANNCUR_HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
			e.bytes = bytes;
			return ANNCUR_OK;
		}
	ANNCUR_HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
	g_attr.push_back({fn, dev, bytes});
	return ANNCUR_OK;
}

int anncur_num_cu() {
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
	std::lock_guard<std::mutex> lock(g_attr_mu);
	if (g_cu[dev] == 0) {
		hipDeviceProp_t prop;
		g_cu[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;  // 256 = MI355X
	}
	return g_cu[dev];
}

// A small pool of timing-less events per (host thread, device) for the fork / join edges of anncur_eval_topk: created once, reused
// by every call of the thread (a recorded event may be re-recorded as soon as the wait that reads it has been enqueued).
namespace {
constexpr int EVENT_POOL = 16;
thread_local hipEvent_t tl_events[64][EVENT_POOL];
thread_local bool tl_events_ready[64] = {false};
}
int anncur_event_pool(hipEvent_t **out, int n) {
	int dev = 0;
	ANNCUR_HIP_OK(hipGetDevice(&dev));
	ANNCUR_REQUIRE(dev >= 0 && dev < 64 && n <= EVENT_POOL, ANNCUR_E_INVALID, "event_pool: bad device / count");
	if (!tl_events_ready[dev]) {
		for (int i = 0; i < EVENT_POOL; ++i) ANNCUR_HIP_OK(hipEventCreateWithFlags(&tl_events[dev][i], hipEventDisableTiming));
		tl_events_ready[dev] = true;
	}
	*out = tl_events[dev];
	return ANNCUR_OK;
}

// The library's memset (common.hpp says why it is a kernel): grid-strided, one word per lane and step.
namespace {
__global__ __launch_bounds__(256) void fill_words_kernel(uint32_t *__restrict__ dst, uint32_t word, size_t n_words) {
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (size_t)gridDim.x * 256) dst[i] = word;
}
}
int anncur_fill_words_async(void *dst, uint32_t word, size_t n_words, hipStream_t st) {
	if (n_words == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(dst && ((uintptr_t)dst % 4) == 0, ANNCUR_E_INVALID, "fill_words: null or misaligned pointer");
	const size_t blocks = (n_words + 255) / 256;
	hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, st, (uint32_t *)dst, word, n_words);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}

extern "C" int anncur_version(void) { return 1000 * 0 + 4; }

extern "C" const char *anncur_last_error(void) { return g_err; }

extern "C" int anncur_device_info(int *n_cu, int *wave_size, char *arch_name, int arch_name_len) {
	int dev = 0;
	ANNCUR_HIP_OK(hipGetDevice(&dev));
	hipDeviceProp_t prop;
	ANNCUR_HIP_OK(hipGetDeviceProperties(&prop, dev));
	if (n_cu) *n_cu = prop.multiProcessorCount;
	if (wave_size) *wave_size = prop.warpSize;
	if (arch_name && arch_name_len > 0) {
		strncpy(arch_name, prop.gcnArchName, (size_t)arch_name_len - 1);
		arch_name[arch_name_len - 1] = 0;
	}
	return ANNCUR_OK;
}

// ---- anncur_sort_id_rows: the scored set S_q of the adaptive search, kept sorted on the device ---------------------------
// One workgroup per row: a bitonic sort in LDS of 64-bit keys (id key, position in the row) -- distinct, so the order is total and equal
// ids (a contract violation, and the holes) keep their order.  An id < 0 sorts behind every id, the padding up to the power of two behind
// those.  The scores are staged in LDS as well, so the call may sort a row in place.
namespace {
__global__ __launch_bounds__(256) void sort_id_rows_kernel(const int32_t *in_ids, const float *in_val, int64_t ld_in, int w, int P, int32_t *out_ids, float *out_val,
															int64_t ld_out, int32_t *__restrict__ counts) {   // (out may alias in: no __restrict__ on the rows)
	extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];
	uint64_t *key = (uint64_t *)sort_smem;                 // [P]
	int32_t *ids = (int32_t *)(key + P);                   // [w]
	float *val = (float *)(ids + w);                       // [w]
	__shared__ int n_valid;
	const int tid = threadIdx.x;
	const int64_t q = blockIdx.x;
	if (tid == 0) n_valid = 0;
	__syncthreads();
	int mine = 0;
	for (int j = tid; j < P; j += 256) {
		uint64_t k = ~0ull;
		if (j < w) {
			const int32_t id = in_ids[q * ld_in + j];
			ids[j] = id;
			val[j] = in_val[q * ld_in + j];
			k = ((uint64_t)(id < 0 ? 0xffffffffu : (uint32_t)id) << 32) | (uint32_t)j;
			mine += id >= 0;
		}
		key[j] = k;
	}
	if (mine) atomicAdd(&n_valid, mine);
	__syncthreads();
	for (int len = 2; len <= P; len <<= 1)
		for (int s = len >> 1; s > 0; s >>= 1) {
			for (int t = tid; t < P / 2; t += 256) {
				const int lo = ((t & ~(s - 1)) << 1) | (t & (s - 1)), hi = lo + s;
				const bool up = (lo & len) == 0;
				const uint64_t a = key[lo], b = key[hi];
				if ((a > b) == up) { key[lo] = b; key[hi] = a; }
			}
			__syncthreads();
		}
	for (int j = tid; j < w; j += 256) {
		const int src = (int)(uint32_t)key[j];
		out_ids[q * ld_out + j] = ids[src];
		out_val[q * ld_out + j] = val[src];
	}
	if (tid == 0) counts[q] = n_valid;
}
}  // namespace

extern "C" int anncur_sort_id_rows(const int32_t *in_ids, const float *in_val, int64_t ld_in, int64_t Q, int32_t w, int32_t *out_ids, float *out_val,
								   int64_t ld_out, int32_t *counts, void *stream) {
	ANNCUR_REQUIRE(Q >= 0 && Q < (int64_t)0x7fffffff && w >= 1 && w <= ANNCUR_MAX_TOPK && ld_in >= w && ld_out >= w, ANNCUR_E_INVALID,
				   "sort_id_rows: need 0 <= Q < 2^31, 1 <= w <= %d and row pitches >= w (got Q = %lld, w = %d)", ANNCUR_MAX_TOPK, (long long)Q, (int)w);
	if (Q == 0) return ANNCUR_OK;
	ANNCUR_REQUIRE(in_ids && in_val && out_ids && out_val && counts, ANNCUR_E_INVALID, "sort_id_rows: null pointer");
	int P = 2;
	while (P < w) P <<= 1;
	const size_t lds = (size_t)P * 8 + (size_t)w * 8;   // at most 32 KiB
	hipLaunchKernelGGL(sort_id_rows_kernel, dim3((unsigned)Q), dim3(256), lds, (hipStream_t)stream, in_ids, in_val, ld_in, (int)w, P, out_ids, out_val, ld_out,
					   counts);
	ANNCUR_LAUNCH_OK();
	return ANNCUR_OK;
}
