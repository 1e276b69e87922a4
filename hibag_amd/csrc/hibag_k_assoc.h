// hibag_k_assoc.h -- kernels of hlaAssocTest (R/Association.R): chi-square tests of every allele (and every level of every
// allele partition) against a case / control label, under the observed labelling and under permutations of it.  Host side:
// hibag_assoc.hip; the definitions: DESIGN.md section 20.
//
// Every statistic is a function of the margins and of ONE integer per test and labelling: the number of case carriers, a
// dot product over samples of a 0/1/2 feature row with a 0/1 label row.  All tests under all permutations of a panel are
// therefore one int8 Gram matrix, features x labels, made by k_ld_gram<1> (hibag_k_ld.h) with exact int32 sums; the
// kernels here build its two operands and turn its cells into statistics, per-permutation maxima and counts.
//
// Operand layout (that of hibag_k_ld.h): int8 [rows][kp], samples contiguous along K, kp a multiple of HIBAG_LD_KPAD,
// padding columns zero.
#ifndef HIBAG_K_ASSOC_H_
#define HIBAG_K_ASSOC_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// hibag_k_ld.h defines its kernels with external linkage for hibag_ld.hip; this translation unit takes the header as it
// is, inside a namespace of its own, so that the library links with both (k_ld_gram<1> is the only kernel launched from here)
namespace hibag_assoc_ld {
#include "hibag_k_ld.h"
}
using hibag_assoc_ld::k_ld_gram;
using hibag_assoc_ld::LdGramOut;

#include "hibag_k_philox.h"

#define ASSOC_DOMINANT 0
#define ASSOC_ADDITIVE 1
#define ASSOC_RECESSIVE 2
#define ASSOC_GENOTYPE 3

// What every launch of a handle shares.  A unit is a sample, for the additive model a chromosome.
struct AssocDims {
	int model = 0;
	int n = 0;                  // kept samples
	int n_test = 0;             // tests; the feature matrix has n_test rows, 2 n_test (het, hom per test) for `genotype`
	long long N = 0, c1 = 0;    // units and case units: n and n_case, twice that for `additive`
};

// k_assoc_features: the feature rows of all tests.  Test t asks for level lev[t] of partition part[t] of the alleles
// (group_of [n_part][n_allele], the identity partition first); with d = (group of a1 == level) + (group of a2 == level)
// the row holds d >= 1 (dominant), d (additive), d == 2 (recessive); `genotype` has the rows 2t: d == 1 and 2t + 1: d == 2.
// One thread per four samples of one row (a dword store); the row sums (zeroed by the caller) are reduced per wavefront
// and added with one integer atomic.  Grid: (ceil(kp / 1024), rows), 256 threads.
__global__ void __launch_bounds__(256) k_assoc_features(const int32_t *__restrict__ a1, const int32_t *__restrict__ a2,
	AssocDims D, const int32_t *__restrict__ group_of, int n_allele, const int32_t *__restrict__ part,
	const int32_t *__restrict__ lev, int kp, int8_t *__restrict__ feat, int32_t *__restrict__ row_sum)
{
	const int row = blockIdx.y;
	const int t = D.model == ASSOC_GENOTYPE ? row >> 1 : row;
	const int32_t *g = group_of + (size_t)part[t] * n_allele;
	const int level = lev[t];
	const int s0 = (blockIdx.x * 256 + threadIdx.x) * 4;
	uint32_t w = 0;
	int sum = 0;
	if (s0 < kp) {
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int s = s0 + b;
			int v = 0;
			if (s < D.n) {
				const int d = (g[a1[s]] == level) + (g[a2[s]] == level);
				if (D.model == ASSOC_DOMINANT) v = d >= 1;
				else if (D.model == ASSOC_ADDITIVE) v = d;
				else if (D.model == ASSOC_RECESSIVE) v = d == 2;
				else v = (row & 1) ? d == 2 : d == 1;
			}
			w |= (uint32_t)v << (8 * b);
			sum += v;
		}
		*(uint32_t *)(feat + (size_t)row * kp + s0) = w;
	}
	for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
	if ((threadIdx.x & 63) == 0 && sum) atomicAdd(row_sum + row, sum);
}

// k_assoc_permute: the label rows of permutations perm0 .. perm0 + n_perm - 1 (perm0 >= 1), int8 0/1 [n_perm][kp].
// Selection sampling over the n samples in order: need = n_case; sample i, with rem = n - i and u = word i & 3 of
// Philox4x32-10(counter (i >> 2, 0, p lo, p hi), key (seed lo, seed hi)), is a case iff u * rem < need << 32 (uint64), and
// then need -= 1.  need == rem forces a case and need == 0 forbids one, so every row has exactly n_case ones.
//
// One lane per permutation: `need` is a serial chain along the samples, so a row cannot be split over lanes.  A lane
// collects 16 labels in registers and stores them with one 16-byte store into its own row.  The alternative, a transpose
// through LDS so that a wavefront writes whole lines of one row, would add a barrier pair per 64 samples to a kernel that
// is bound by the latency of that chain (one Philox block and four dependent compares per four samples) and not by its
// stores: a lane's eight successive stores fill one 128-byte line of its row, which the L2 merges before it writes back,
// and the label bytes are a small fraction of what the Gram reads.  Grid: ceil(n_perm / 64), 64 threads.
__global__ void __launch_bounds__(64) k_assoc_permute(int n, int n_case, int kp, uint64_t seed, uint64_t perm0, int n_perm,
	int8_t *__restrict__ labels)
{
	const int j = blockIdx.x * 64 + threadIdx.x;
	if (j >= n_perm) return;
	const uint64_t p = perm0 + (uint64_t)j;
	const uint32_t plo = (uint32_t)p, phi = (uint32_t)(p >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
	uint4 *row = (uint4 *)(labels + (size_t)j * kp);
	uint32_t need = (uint32_t)n_case;
	for (int i0 = 0; i0 < kp; i0 += 16) {
		uint32_t out[4] = {0, 0, 0, 0};
		if (i0 < n) {
#pragma unroll
			for (int q = 0; q < 4; q++) {
				uint32_t u[4];
				philox4x32_10((uint32_t)((i0 >> 2) + q), 0u, plo, phi, k0, k1, u[0], u[1], u[2], u[3]);
#pragma unroll
				for (int b = 0; b < 4; b++) {
					const int i = i0 + 4 * q + b;
					const bool is_case = i < n && (uint64_t)u[b] * (uint64_t)(n - i) < ((uint64_t)need << 32);
					need -= is_case ? 1u : 0u;
					out[q] |= (is_case ? 1u : 0u) << (8 * b);
				}
			}
		}
		row[i0 >> 4] = make_uint4(out[0], out[1], out[2], out[3]);
	}
}

// The Yates-corrected 2 x 2 chi-square of R's chisq.test from a = case carriers, r1 = carriers, c1 = cases, N = units:
// NaN with an empty margin, 0.0 where the correction takes the whole deviation, else D^2 N / (4 r1 r2 c1 c2) with
// D = 2 |N a - r1 c1| - N; the integers in int64, then one rounding per operation (the file is built with -ffp-contract=off).
__device__ __forceinline__ double assoc_chisq_2x2(long long N, long long a, long long r1, long long c1)
{
	const long long r2 = N - r1, c2 = N - c1;
	if (r1 == 0 || r2 == 0 || c1 == 0 || c2 == 0) return __builtin_nan("");
	const long long det = N * a - r1 * c1;
	const long long D = 2 * (det < 0 ? -det : det) - N;
	if (D <= 0) return 0.0;
	const double d = (double)D;
	return ((d * d) * (double)N) / ((4.0 * (double)(r1 * r2)) * (double)(c1 * c2));
}

__device__ __forceinline__ double assoc_term(long long N, long long x, long long r, long long c)
{
	const double num = (double)(N * x - r * c);
	return (num * num) / ((double)N * (double)(r * c));
}

// The uncorrected 3 x 2 chi-square: rows none / het / hom (r_het, r_hom carriers, x_het, x_hom of them cases), columns
// control / case; the six terms added in that order.  NaN with an empty margin.
__device__ __forceinline__ double assoc_chisq_3x2(long long N, long long c1, long long r_het, long long r_hom, long long x_het,
	long long x_hom)
{
	const long long r_non = N - r_het - r_hom, c0 = N - c1;
	if (r_non == 0 || r_het == 0 || r_hom == 0 || c0 == 0 || c1 == 0) return __builtin_nan("");
	const long long x_non = c1 - x_het - x_hom;
	double s = assoc_term(N, r_non - x_non, r_non, c0);
	s += assoc_term(N, x_non, r_non, c1);
	s += assoc_term(N, r_het - x_het, r_het, c0);
	s += assoc_term(N, x_het, r_het, c1);
	s += assoc_term(N, r_hom - x_hom, r_hom, c0);
	s += assoc_term(N, x_hom, r_hom, c1);
	return s;
}

// k_assoc_stat: the statistics of a panel of labellings from the Gram C [rows][ld] (row = feature row, column = labelling).
// Lane = labelling, the tests walked in order: a wavefront reads 64 consecutive int32 of one Gram row per step, and the
// maximum over the tests is a running value of the lane, without a cross-lane step.
//   stat_out   [n_test] or NULL: the statistic of labelling 0 (the observed one, a panel of its own)
//   max_out    [n_lab] or NULL:  the largest non-NaN statistic of each labelling, NaN if there is none
//   stat_obs / count  [n_test] or NULL: count[t] += the labellings with stat >= stat_obs[t] (false where either is NaN);
//                     per wavefront a population count of the ballot and one integer atomic -- integer sums have no order
// Grid: ceil(n_lab / 64), 64 threads.
__global__ void __launch_bounds__(64) k_assoc_stat(const int32_t *__restrict__ C, size_t ld, int n_lab, AssocDims D,
	const int32_t *__restrict__ row_sum, double *__restrict__ stat_out, double *__restrict__ max_out,
	const double *__restrict__ stat_obs, unsigned long long *__restrict__ count)
{
	const int j = blockIdx.x * 64 + threadIdx.x;
	const bool live = j < n_lab;
	const size_t col = live ? (size_t)j : 0;              // (a dead lane reads column 0 and takes no part in any output)
	double best = -1.0;                                   // (every statistic is >= 0)
	for (int t = 0; t < D.n_test; t++) {
		double st;
		if (D.model == ASSOC_GENOTYPE) {
			const long long x_het = C[(size_t)(2 * t) * ld + col], x_hom = C[(size_t)(2 * t + 1) * ld + col];
			st = assoc_chisq_3x2(D.N, D.c1, row_sum[2 * t], row_sum[2 * t + 1], x_het, x_hom);
		} else {
			st = assoc_chisq_2x2(D.N, C[(size_t)t * ld + col], row_sum[t], D.c1);
		}
		best = st > best ? st : best;                     // (false for NaN)
		if (stat_out && j == 0) stat_out[t] = st;
		if (count) {
			const unsigned long long hits = __ballot(live && st >= stat_obs[t]);
			if (threadIdx.x == 0 && hits) atomicAdd(count + t, (unsigned long long)__popcll(hits));
		}
	}
	if (live && max_out) max_out[j] = best < 0 ? __builtin_nan("") : best;
}

#endif
