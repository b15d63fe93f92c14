// The Gumbel noise of the SoftMax item sampling (the contract is written out in include/anncur_hip.h).
//
// g(q, i) is a pure function of (seed, stream, row key, item id): a counter-based generator -- two splitmix64 finalisers -- with no state,
// so the noise does not depend on launch shape, row chunking or a row's position in the call.  ONE device function, called by the sampler
// (sample_topk_kernel) and by the audit kernel (gumbel_noise_kernel) alike.
#pragma once
#include "common.hpp"

namespace anncur {

__host__ __device__ __forceinline__ uint64_t gumbel_mix64(uint64_t z) {
	z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
	z ^= z >> 27; z *= 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// the call's part of the counter (host code: the launchers pass it to the kernels)
__host__ __device__ __forceinline__ uint64_t gumbel_base(uint64_t seed, uint32_t stream_id) {
	return gumbel_mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)stream_id + 1ull));
}

// the row's part: base ^ (row_key << 32 | item) = (base ^ row_key << 32) ^ item
__device__ __forceinline__ uint64_t gumbel_row(uint64_t base, uint32_t row_key) { return base ^ ((uint64_t)row_key << 32); }

constexpr float GUMBEL_MAX = 16.64f;   // g <= -log(-log(1 - 2^-24)) = 16.6355...: an upper bound the sampler's prefilter adds to a scaled score

// u = (23 bits + 0.5) 2^-23: exact in fp32 (24 significant bits), strictly inside (0, 1), so both logarithms are finite;
// logf is the accurate one (this library is built without fast-math)
__device__ __forceinline__ float gumbel_noise(uint64_t row, uint32_t item) {
	const uint64_t z = gumbel_mix64(row ^ (uint64_t)item);
	// the 23 bits n as the fraction of a float in [1, 2), less 1 - 2^-24: (1 + n 2^-23) - (1 - 2^-24) = (n + 0.5) 2^-23, an exact difference
	// (an integer-to-float conversion of z >> 41 costs hipcc six instructions more)
	const float u = __fsub_rn(__uint_as_float(0x3f800000u | (uint32_t)(z >> 41)), 0.99999994f);
	return -logf(-logf(u));
}

// the perturbed key: two separately rounded fp32 operations (hipcc would contract a * b + c into an fma)
__device__ __forceinline__ float gumbel_key(float s, float inv_T, float g) { return __fadd_rn(__fmul_rn(s, inv_T), g); }

}  // namespace anncur
