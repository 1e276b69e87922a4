// hibag_k_cohort.h -- part of hibag_kernels.hip (included there): k_cohort_pack / k_cohort_counts, the kernels of the resident
// cohort (hibag_cohort.hip, include/hibag_hip.h "resident cohort").
//
// The resident form is PLINK's own: 2 bits per genotype, SNP-major, four samples per byte with the lowest bits first, the
// codes 00 = 2, 01 = missing, 10 = 1, 11 = 0 (the inverse of bed_code in hibag_k_pack.h), rows `stride` bytes apart with
// `stride` a multiple of 16.  k_bed_codes (mode != 0) reads such rows as they stand; the samples behind the cohort's last
// one read as missing (the rows are preset to 0x55 bytes, and the kernels here write 01 into the slots they do not fill).
#ifndef HIBAG_K_COHORT_H_
#define HIBAG_K_COHORT_H_

// genotype -> PLINK code; anything outside 0..2 (NA_integer_ included) is missing, the rule of k_codes
__device__ __forceinline__ uint32_t cohort_code(int g)
{
	return (unsigned)g <= 2u ? (0x023u >> (4 * g)) & 3u : 1u;
}

#define COHORT_TILE_SAMP 256       // samples x SNPs of a workgroup's tile of a sample-major slab
#define COHORT_TILE_SNP  64

// k_cohort_pack: one slab of the host's int32 matrix -> its part of the resident rows.  `out` points at the resident row of
// the slab's first SNP, `byte0` is the byte of the slab's first sample inside a row (the slabs of a cohort start at
// multiples of 256 samples, so bytes and dwords never straddle two slabs).
//   SNP_MAJOR: slab [n_snp][ld], one row of n_samp genotypes per SNP, ld a multiple of 4 and the slab 16-byte aligned: no
//     transpose -- block = 256 bytes of one row, lane = one byte: one 16-byte load of four genotypes, one byte stored,
//     both contiguous along the samples across the wavefront.
//   otherwise: slab [n_samp][ld] with the SNP fastest (the memory of R's SNP x sample matrix): a tile of 256 samples x 64
//     SNPs goes through LDS as codes, like k_codes -- the int32 reads are coalesced along SNPs; then a lane forms one dword
//     (16 samples) of one SNP row, and sixteen neighbouring lanes store 64 contiguous bytes of it.
// Nothing crosses lanes outside the LDS tile; every store is an ordinary vector store.
template <bool SNP_MAJOR>
__global__ __launch_bounds__(256) void k_cohort_pack(const int32_t *__restrict__ slab, size_t ld, int n_snp, int n_samp,
	uint8_t *__restrict__ out, size_t stride, size_t byte0)
{
	if (SNP_MAJOR) {
		const int b = blockIdx.x * 256 + threadIdx.x;
		const int k = blockIdx.y;
		if (k >= n_snp || 4 * (long long)b >= n_samp) return;
		const int4 g = *(const int4 *)(slab + (size_t)k * ld + 4 * (size_t)b);
		const int left = n_samp - 4 * b;             // genotypes of this byte that exist (the others: missing)
		const uint32_t v = cohort_code(g.x) | (left > 1 ? cohort_code(g.y) : 1u) << 2 |
			(left > 2 ? cohort_code(g.z) : 1u) << 4 | (left > 3 ? cohort_code(g.w) : 1u) << 6;
		out[(size_t)k * stride + byte0 + (size_t)b] = (uint8_t)v;
	} else {
		__shared__ uint8_t tile[COHORT_TILE_SAMP][COHORT_TILE_SNP + 1];
		const int s0 = blockIdx.x * COHORT_TILE_SAMP, k0 = blockIdx.y * COHORT_TILE_SNP;
		const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
		for (int r = ty; r < COHORT_TILE_SAMP; r += 4) {
			const int s = s0 + r, k = k0 + tx;
			int g = -1;
			if (s < n_samp && k < n_snp) g = slab[(size_t)s * ld + k];
			tile[r][tx] = (uint8_t)cohort_code(g);
		}
		__syncthreads();
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int at = q * 256 + threadIdx.x;
			const int kk = at >> 4, d = at & 15;       // dword d of the tile's SNP kk: samples s0 + 16 d ...
			if (k0 + kk >= n_snp || s0 + 16 * d >= n_samp) continue;
			uint32_t w = 0;
#pragma unroll
			for (int i = 0; i < 16; i++) w |= (uint32_t)tile[16 * d + i][kk] << (2 * i);
			*(uint32_t *)(out + (size_t)(k0 + kk) * stride + byte0 + (size_t)(s0 / 4 + 4 * d)) = w;
		}
	}
}

// k_cohort_counts: per resident row the number of called genotypes and their sum, by popcounts on the 2-bit codes: exact
// integers, so the order of the additions does not matter.  Wavefront = SNP row, four rows per workgroup; a lane walks the
// row in 16-byte steps (64 lanes: 1 KB contiguous per step) and the 64 partial sums meet in LDS.  The row is read to its
// full stride: the slots behind the last sample hold the missing code and count as such.
__global__ __launch_bounds__(256) void k_cohort_counts(const uint8_t *__restrict__ rows, size_t stride, int n_snp,
	int32_t *__restrict__ n_valid, int64_t *__restrict__ sum)
{
	__shared__ uint32_t red[4][2][64];
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int k = blockIdx.x * 4 + w;
	const size_t nq = stride / 16;
	uint32_t miss = 0, tot = 0;
	if (k < n_snp) {
		const uint4 *row = (const uint4 *)(rows + (size_t)k * stride);
		for (size_t q = lane; q < nq; q += 64) {
			const uint4 v = row[q];
			const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int i = 0; i < 4; i++) {
				const uint32_t lo = x[i] & 0x55555555u, hi = (x[i] >> 1) & 0x55555555u;
				miss += __popc(lo & ~hi);                                            // 01
				tot += 2u * __popc(~(lo | hi) & 0x55555555u) + __popc(hi & ~lo);    // 00 = 2, 10 = 1
			}
		}
	}
	red[w][0][lane] = miss;
	red[w][1][lane] = tot;
	__syncthreads();
	for (int off = 32; off > 0; off >>= 1) {
		if (lane < off) {
			red[w][0][lane] += red[w][0][lane + off];
			red[w][1][lane] += red[w][1][lane + off];
		}
		__syncthreads();
	}
	if (lane == 0 && k < n_snp) {
		n_valid[k] = (int32_t)((uint32_t)(stride * 4) - red[w][0][0]);
		sum[k] = (int64_t)red[w][1][0];
	}
}

#endif
