// hibag_k_ld.h -- kernels of hlaGenoLD and hlaLDMatrix (R/HIBAG.R:1399-1446, :1453-1541): r^2 between SNP genotypes and
// HLA allele dosages, and between SNPs, as int8 Gram matrices over samples on the matrix cores.  Host side: hibag_ld.hip.
//
// Every sum behind r^2 is a dot product of small integers over samples (genotypes and dosages are 0/1/2), so the products
// run on v_mfma_i32_32x32x32_i8 with int32 accumulators and are exact; the epilogue turns the sums into r^2 with the
// formula of DESIGN.md "LD", in int64 and then double, with one rounding per operation (-ffp-contract=off).
//
// Operand layout: int8 [rows][kp], a row per SNP (or per allele), samples contiguous along K, kp a multiple of
// HIBAG_LD_KPAD (four MFMA K blocks of 32).  Padding columns hold zeros in every operand, so they add nothing to a sum.
#ifndef HIBAG_K_LD_H_
#define HIBAG_K_LD_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HIBAG_LD_KPAD 128           // K step of k_ld_gram: the operands' row length is a multiple of it
#define HIBAG_LD_MISSING 3          // code of a missing genotype in the resident matrix (values outside {0,1,2})
#define HIBAG_LD_TILE 64            // k_ld_gram: a workgroup computes a 64 x 64 tile of the Gram, four waves of 32 x 32
#define HIBAG_LD_LDS_ROW (HIBAG_LD_KPAD + 16)   // bytes per LDS row: the pad keeps the ds_read_b128 rows off one bank set

typedef int ld_v4i __attribute__((ext_vector_type(4)));
typedef int ld_v16i __attribute__((ext_vector_type(16)));

// r^2 from the integer sums over n samples.  NaN (the quiet NaN numpy writes) where either variance is zero.
__device__ __forceinline__ double ld_r2(long long n, long long sxy, long long sx, long long sy, long long sxx, long long syy)
{
	const long long num = n * sxy - sx * sy;
	const long long dx = n * sxx - sx * sx;
	const long long dy = n * syy - sy * sy;
	if (dx == 0 || dy == 0) return __builtin_nan("");
	const double a = (double)num;
	return (a * a) / ((double)dx * (double)dy);
}

// k_ld_pack: the caller's int32 genotypes -> codes int8 [n_snp][kp] (0/1/2, HIBAG_LD_MISSING for anything else and for
// the padding columns), plus per SNP the number of called genotypes and their sum (both zeroed by the caller).
// One workgroup per tile of 64 SNPs x 64 samples, transposed through LDS when the input is sample-major, so that the
// reads are coalesced in either order.  Grid: (kp / 64, ceil(n_snp / 64)), 256 threads.
__global__ void __launch_bounds__(256) k_ld_pack(const int32_t *__restrict__ geno, int n_snp, int n_samp, int snp_major,
	int kp, int8_t *__restrict__ codes, int32_t *__restrict__ n_valid, int32_t *__restrict__ sum)
{
	__shared__ int8_t tile[64][64 + 4];
	const int s0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
	const int t = threadIdx.x;
	for (int e = t; e < 64 * 64; e += 256) {
		// the fast index of the read follows the input's contiguous axis
		const int fast = e & 63, slow = e >> 6;
		const int j = snp_major ? slow : fast, s = snp_major ? fast : slow;
		const int gj = j0 + j, gs = s0 + s;
		int v = HIBAG_LD_MISSING;
		if (gj < n_snp && gs < n_samp) {
			const int g = snp_major ? geno[(size_t)gj * n_samp + gs] : geno[(size_t)gs * n_snp + gj];
			if (g >= 0 && g <= 2) v = g;
		}
		tile[j][s] = (int8_t)v;
	}
	__syncthreads();
	// 4 threads per SNP row, 16 samples (4 dwords) each
	const int j = t >> 2, q = t & 3, gj = j0 + j;
	if (gj >= n_snp) return;
	int nv = 0, sm = 0;
	uint32_t w[4];
#pragma unroll
	for (int d = 0; d < 4; d++) {
		uint32_t x = 0;
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int c = tile[j][q * 16 + d * 4 + b];
			if (c != HIBAG_LD_MISSING) { nv++; sm += c; }
			x |= (uint32_t)c << (8 * b);
		}
		w[d] = x;
	}
	*(uint4 *)(codes + (size_t)gj * kp + s0 + q * 16) = make_uint4(w[0], w[1], w[2], w[3]);
	nv += __shfl_xor(nv, 1); sm += __shfl_xor(sm, 1);
	nv += __shfl_xor(nv, 2); sm += __shfl_xor(sm, 2);
	if (q == 0 && nv) { atomicAdd(n_valid + gj, nv); atomicAdd(sum + gj, sm); }
}

// k_ld_complete: flag[s] = 1 if sample s has a called genotype at every SNP of idx (casewise deletion, R's
// use = "na.or.complete").  One thread per sample; a wave reads 64 consecutive bytes of one SNP row per step.
__global__ void __launch_bounds__(256) k_ld_complete(const int8_t *__restrict__ codes, int kp, int n_samp,
	const int32_t *__restrict__ idx, int n_idx, uint8_t *__restrict__ flag)
{
	const int s = blockIdx.x * 256 + threadIdx.x;
	if (s >= n_samp) return;
	int ok = 1;
	for (int i = 0; i < n_idx && ok; i++) ok = codes[(size_t)idx[i] * kp + s] != HIBAG_LD_MISSING;
	flag[s] = (uint8_t)ok;
}

// k_ld_compact: xc[i][t] = genotype of SNP idx[i] at complete sample samp[t] (t < n_c; zero up to kc), and the SNP's
// Sx, Sxx over the complete samples.  One workgroup per SNP.
__global__ void __launch_bounds__(256) k_ld_compact(const int8_t *__restrict__ codes, int kp, const int32_t *__restrict__ idx,
	const int32_t *__restrict__ samp, int n_c, int kc, int8_t *__restrict__ xc, int32_t *__restrict__ sx, int32_t *__restrict__ sxx)
{
	__shared__ int red[2][4];
	const int i = blockIdx.x;
	const int8_t *src = codes + (size_t)idx[i] * kp;
	int8_t *dst = xc + (size_t)i * kc;
	int a = 0, b = 0;
	for (int t = threadIdx.x; t < kc; t += 256) {
		const int v = t < n_c ? src[samp[t]] : 0;       // a complete sample's code is 0, 1 or 2
		dst[t] = (int8_t)v;
		a += v;
		b += v * v;
	}
	for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
	const int wv = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { red[0][wv] = a; red[1][wv] = b; }
	__syncthreads();
	if (threadIdx.x == 0) {
		sx[i] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
		sxx[i] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
	}
}

// k_ld_hla_snp_operand: the SNP side of hlaGenoLD's Gram, three row blocks of n_snp rows: X (genotype, 0 where missing),
// X^2, M (1 where called).  Byte-parallel on the codes, one dword (4 samples) per thread.
__global__ void __launch_bounds__(256) k_ld_hla_snp_operand(const int8_t *__restrict__ codes, int n_snp, int kp,
	int8_t *__restrict__ a)
{
	const size_t per = (size_t)kp / 4;
	const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= (size_t)n_snp * per) return;
	const uint32_t w = ((const uint32_t *)codes)[e];
	const uint32_t m3 = w & (w >> 1) & 0x01010101u;       // 1 in every byte that holds the missing code 3
	const uint32_t x = w & ~(m3 * 3u);                    // missing -> 0 (bytes are 0/1, so m3 * 3 has no carry)
	const uint32_t x2 = x + (x & 0x02020202u);            // 0/1/2 -> 0/1/4
	const uint32_t m = 0x01010101u ^ m3;
	uint32_t *o = (uint32_t *)a;
	const size_t blk = (size_t)n_snp * per;
	o[e] = x;
	o[blk + e] = x2;
	o[2 * blk + e] = m;
}

// k_ld_hla_allele_operand: the allele side, 2 n_allele + 1 rows: Y_a (dosage of allele a, 0 for unusable samples),
// Y_a^2, then V (1 where both alleles are known).  a1 / a2 are 0-based allele indices or NA (anything negative).
__global__ void __launch_bounds__(256) k_ld_hla_allele_operand(const int32_t *__restrict__ a1, const int32_t *__restrict__ a2,
	int n_samp, int n_allele, int kp, int8_t *__restrict__ b)
{
	const int s = blockIdx.x * 256 + threadIdx.x;
	const int row = blockIdx.y;
	if (s >= kp) return;
	int v = 0;
	if (s < n_samp) {
		const int x1 = a1[s], x2 = a2[s];
		if (x1 >= 0 && x2 >= 0) {
			if (row == 2 * n_allele) v = 1;
			else {
				const int a = row < n_allele ? row : row - n_allele;
				const int y = (x1 == a) + (x2 == a);
				v = row < n_allele ? y : y * y;
			}
		}
	}
	b[(size_t)row * kp + s] = (int8_t)v;
}

// Epilogue of k_ld_gram
struct LdGramOut {
	// raw sums: out32[i][j], i < ma, j < mb, row stride ld
	int32_t *out32 = nullptr;
	// r^2 (hlaLDMatrix): out64[i][j] of the panel whose first SNP is row0; n the number of complete samples,
	// sx / sxx per SNP (global index)
	double *out64 = nullptr;
	int row0 = 0;
	long long n = 0;
	const int32_t *sx = nullptr, *sxx = nullptr;
	size_t ld = 0;
};

// 16 operand bytes of a staged row; the address is always inside the operand (an invalid row reads row 0), the value of
// an invalid row is zero (a select of values: a select of addresses would put the zeros in scratch memory)
__device__ __forceinline__ uint4 ld_stage(const int8_t *p, bool valid)
{
	const uint4 v = *(const uint4 *)p;
	return valid ? v : make_uint4(0, 0, 0, 0);
}

// k_ld_gram: C[i][j] = sum_k A[i][k] B[j][k] over kp int8 columns (A [ma][kp], B [mb][kp]), 64 x 64 tiles, one tile per
// 256-thread workgroup.  Each K step stages 64 rows x 128 bytes of both operands in LDS (the next step's are loaded into
// registers meanwhile); each wave issues four v_mfma_i32_32x32x32_i8 into its 32 x 32 accumulator.  Rows past ma / mb
// are staged as zeros and never stored.  RAW = 1: store the int32 sums; 0: store r^2 (hlaLDMatrix, A and B the same
// compacted matrix, A offset by the panel's first row).  Grid: (ceil(mb / 64), ceil(ma / 64)).
template <int RAW>
__global__ void __launch_bounds__(256) k_ld_gram(const int8_t *__restrict__ A, int ma, const int8_t *__restrict__ B, int mb,
	int kp, LdGramOut O)
{
	__shared__ __attribute__((aligned(16))) int8_t sa[HIBAG_LD_TILE * HIBAG_LD_LDS_ROW];
	__shared__ __attribute__((aligned(16))) int8_t sb[HIBAG_LD_TILE * HIBAG_LD_LDS_ROW];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int wr = wave >> 1, wc = wave & 1;                  // the wave's 32 x 32 quadrant
	const int i0 = blockIdx.y * HIBAG_LD_TILE, j0 = blockIdx.x * HIBAG_LD_TILE;

	// staging: 64 rows x 8 chunks of 16 bytes per operand, two chunks per thread (rows t / 8 and t / 8 + 32).  A row past
	// ma / mb reads row 0 instead and stages zeros.
	const int srow = t >> 3, soff = (t & 7) * 16;
	const bool va0 = i0 + srow < ma, va1 = i0 + srow + 32 < ma, vb0 = j0 + srow < mb, vb1 = j0 + srow + 32 < mb;
	const int8_t *pa0 = A + (va0 ? (size_t)(i0 + srow) * kp : 0) + soff, *pa1 = A + (va1 ? (size_t)(i0 + srow + 32) * kp : 0) + soff;
	const int8_t *pb0 = B + (vb0 ? (size_t)(j0 + srow) * kp : 0) + soff, *pb1 = B + (vb1 ? (size_t)(j0 + srow + 32) * kp : 0) + soff;
	uint4 ra0 = ld_stage(pa0, va0), ra1 = ld_stage(pa1, va1), rb0 = ld_stage(pb0, vb0), rb1 = ld_stage(pb1, vb1);
	int8_t *const wa = sa + srow * HIBAG_LD_LDS_ROW + soff, *const wb = sb + srow * HIBAG_LD_LDS_ROW + soff;

	ld_v16i acc;
#pragma unroll
	for (int r = 0; r < 16; r++) acc[r] = 0;
	const int r32 = lane & 31, h = lane >> 5;
	const int8_t *la = sa + (wr * 32 + r32) * HIBAG_LD_LDS_ROW + 16 * h;
	const int8_t *lb = sb + (wc * 32 + r32) * HIBAG_LD_LDS_ROW + 16 * h;

	for (int k0 = 0; k0 < kp; k0 += HIBAG_LD_KPAD) {
		__syncthreads();                                  // the previous step's reads are done
		*(uint4 *)wa = ra0;
		*(uint4 *)(wa + 32 * HIBAG_LD_LDS_ROW) = ra1;
		*(uint4 *)wb = rb0;
		*(uint4 *)(wb + 32 * HIBAG_LD_LDS_ROW) = rb1;
		__syncthreads();
		const int kn = k0 + HIBAG_LD_KPAD;
		if (kn < kp) {
			ra0 = ld_stage(pa0 + kn, va0);
			ra1 = ld_stage(pa1 + kn, va1);
			rb0 = ld_stage(pb0 + kn, vb0);
			rb1 = ld_stage(pb1 + kn, vb1);
		}
		// lane l holds row l % 32 and the 16 K positions 16 (l / 32) .. +15 of each 32-wide K block, for A and B alike
#pragma unroll
		for (int kk = 0; kk < HIBAG_LD_KPAD / 32; kk++) {
			const ld_v4i a = *(const ld_v4i *)(la + kk * 32);
			const ld_v4i b = *(const ld_v4i *)(lb + kk * 32);
			acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
		}
	}

	// accumulator register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of the wave's quadrant
	const int j = j0 + wc * 32 + r32;
	if (j >= mb) return;
	long long sxj = 0, sxxj = 0;
	if (!RAW) { sxj = O.sx[j]; sxxj = O.sxx[j]; }
#pragma unroll
	for (int r = 0; r < 16; r++) {
		const int i = i0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
		if (i >= ma) continue;
		if (RAW) {
			O.out32[(size_t)i * O.ld + j] = acc[r];
		} else {
			const int gi = O.row0 + i;
			double v;
			if (gi == j) v = O.n >= 2 ? 1.0 : __builtin_nan("");
			else v = ld_r2(O.n, acc[r], O.sx[gi], sxj, O.sxx[gi], sxxj);
			O.out64[(size_t)i * O.ld + j] = v;
		}
	}
}

// k_ld_hla_finish: per SNP j the r^2 with every allele from the sums of the raw Gram C [3 n_snp][2 n_allele + 1]
// (rows X, X^2, M; columns Y, Y^2, V), and ld[j] = the mean of the non-NaN ones, summed in allele order (NaN if none).
__global__ void __launch_bounds__(256) k_ld_hla_finish(const int32_t *__restrict__ C, int n_snp, int n_allele,
	double *__restrict__ ld, double *__restrict__ r2)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n_snp) return;
	const size_t mb = 2 * (size_t)n_allele + 1;
	const int32_t *cx = C + (size_t)j * mb, *cx2 = C + ((size_t)n_snp + j) * mb, *cm = C + (2 * (size_t)n_snp + j) * mb;
	const long long n = cm[2 * n_allele], sx = cx[2 * n_allele], sxx = cx2[2 * n_allele];
	double s = 0.0;
	int cnt = 0;
	for (int a = 0; a < n_allele; a++) {
		const double v = ld_r2(n, cx[a], sx, cm[a], sxx, cm[n_allele + a]);
		if (r2) r2[(size_t)j * n_allele + a] = v;
		if (!__builtin_isnan(v)) { s += v; cnt++; }
	}
	ld[j] = cnt ? s / (double)cnt : __builtin_nan("");
}

#endif
