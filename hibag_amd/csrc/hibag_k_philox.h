// hibag_k_philox.h -- the counter-based generator of the draw finish (hibag_k_draw.h) and of the association tests'
// permutations (hibag_k_assoc.h): Philox4x32-10 (Salmon et al., SC'11), 32 x 32 -> 64 multiplies and xors on the vector ALU.
#ifndef HIBAG_K_PHILOX_H_
#define HIBAG_K_PHILOX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// all four output words of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
	uint32_t &w0, uint32_t &w1, uint32_t &w2, uint32_t &w3)
{
#pragma unroll
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	w0 = c0; w1 = c1; w2 = c2; w3 = c3;
}

// the first two output words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
	uint32_t &w0, uint32_t &w1)
{
	uint32_t w2, w3;
	philox4x32_10(c0, c1, c2, c3, k0, k1, w0, w1, w2, w3);
}

#endif
