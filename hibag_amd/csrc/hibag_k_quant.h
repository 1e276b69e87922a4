// hibag_k_quant.h -- kernels of hlaAssocQuant (R/Association.R:262-313, 368-376): every test of an association handle
// against a quantitative trait, y ~ h + covariates by least squares, under the observed trait and under Freedman-Lane
// permutations of its residuals.  Host side: hibag_assoc.hip.
//
// With the basis q_0 .. q_q (the constant and the covariates, orthonormalised on the host) a permuted statistic is a function
// of g[row] = sum_i F[row][i] r[i], r the permuted residual trait projected off the basis, and of rr = sum r^2.  All tests
// under all permutations of a panel are one real-valued Gram matrix, int8 feature rows x FP64 residual rows, made by
// k_quant_gram on v_mfma_f64_16x16x4_f64; the kernels here build the residual panel and turn the Gram into statistics,
// per-permutation maxima and counts.
//
// Residual panel (written by k_quant_project, read by k_quant_gram): float64 [tiles][kp / 4][4][16] -- per tile of 16
// permutations and per step of four samples the 64 values in the B operand's lane order (lane = 16 (sample & 3) + permutation
// & 15), so a wavefront's operand load is 512 contiguous bytes.  Padding samples (i >= n) and the permutations past the
// panel's last one hold 0.
//
// Order of every sum: a thread adds its own terms in index order, the threads' parts are added in a fixed tree or in thread
// order, a wave walks its steps in order and the waves' tiles are added in wave order.  So every number depends on n, on its
// own row and permutation and on the constants below alone -- not on the panel size, the other tests or the other
// permutations.  No floating-point atomics.
#ifndef HIBAG_K_QUANT_H_
#define HIBAG_K_QUANT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hibag_k_philox.h"

#define QUANT_TILE 16               // permutations of a tile, feature rows of a tile: the MFMA's M and N
#define QUANT_MAX_BASIS 13          // the constant and at most HIBAG_HIP_GLM_MAX_COVAR columns
#define QUANT_GRAM_WAVES 4          // waves of k_quant_gram's workgroup, which split K
#define QUANT_FLAG_RANK 2           // the test is not fitted: the values are NaN (GLM_FLAG_RANK's bit)

typedef double quant_d4 __attribute__((ext_vector_type(4)));

// What the statistic of a test needs beside g and rr.  row_a < 0: not fitted (NaN).  row_b < 0: one column, a11 = sxx.
// Else the two dummies of `genotype` with a11, a22, a12 and det.
struct QuantTest {
	int row_a, row_b;
	double df, a11, a22, a12, det;
};

// The sum of v over the 256 threads of a workgroup in a fixed tree (thread t adds thread t + o for o = 128, 64, ... 1);
// every thread gets it.  s: 256 doubles of LDS.
__device__ __forceinline__ double quant_block_sum(double v, double *s)
{
	const int tid = threadIdx.x;
	__syncthreads();
	s[tid] = v;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if (tid < o) s[tid] += s[tid + o];
		__syncthreads();
	}
	return s[0];
}

// k_quant_classes: per test and class d in {0, 1, 2} of its samples (the row value; het -> 1, hom -> 2 for `genotype`) the
// count, S1 = sum y_c and S2 = sum y_c^2.  One workgroup per test, thread t takes the samples t, t + 256, ...
// Outputs [n_test][3].  Grid: n_test, 256 threads.
__global__ void __launch_bounds__(256) k_quant_classes(const int8_t *__restrict__ feat, int kp, int n, int genotype,
	const double *__restrict__ yc, long long *__restrict__ cnt, double *__restrict__ S1, double *__restrict__ S2)
{
	__shared__ double s[256];
	__shared__ int s_cnt[3];
	const int t = blockIdx.x, tid = threadIdx.x;
	const int8_t *fa = feat + (size_t)(genotype ? 2 * t : t) * kp;
	const int8_t *fb = genotype ? fa + kp : nullptr;
	int c[3] = {0, 0, 0};
	double a1[3] = {0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0};
	if (tid < 3) s_cnt[tid] = 0;
	for (int i = tid; i < n; i += 256) {
		const int d = genotype ? fa[i] + 2 * fb[i] : fa[i];
		const double v = yc[i];
#pragma unroll
		for (int k = 0; k < 3; k++)
			if (d == k) { c[k]++; a1[k] += v; a2[k] += v * v; }
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 3; k++) {
		if (c[k]) atomicAdd(&s_cnt[k], c[k]);            // (integer sums have no order)
		const double x1 = quant_block_sum(a1[k], s);
		const double x2 = quant_block_sum(a2[k], s);
		if (tid == 0) { S1[(size_t)t * 3 + k] = x1; S2[(size_t)t * 3 + k] = x2; }
	}
	__syncthreads();
	if (tid < 3) cnt[(size_t)t * 3 + tid] = s_cnt[tid];
}

// k_quant_proj: proj[row][k] = sum_i F[row][i] q_k[i] for the nb basis rows Q [nb][kp].  One workgroup per feature row.
// Grid: rows, 256 threads.
__global__ void __launch_bounds__(256) k_quant_proj(const int8_t *__restrict__ feat, int kp, int n, const double *__restrict__ Q,
	int nb, double *__restrict__ proj)
{
	__shared__ double s[256];
	const int row = blockIdx.x, tid = threadIdx.x;
	const int8_t *f = feat + (size_t)row * kp;
	for (int k = 0; k < nb; k++) {
		const double *q = Q + (size_t)k * kp;
		double a = 0.0;
		for (int i = tid; i < n; i += 256) a += (double)f[i] * q[i];
		a = quant_block_sum(a, s);
		if (tid == 0) proj[(size_t)row * nb + k] = a;
	}
}

// k_quant_perm: the rows of permutations perm0 .. perm0 + n_perm - 1, int32 [n_perm][ld], by the inside-out Fisher-Yates
// shuffle: for i = 0 .. n - 1, j = (u (i + 1)) >> 32 with u = word i & 3 of Philox4x32-10(counter (i >> 2, 1, p lo, p hi),
// key (seed lo, seed hi)); row[i] = row[j]; row[j] = i.  Permutation 0 is the identity (the observed run).
//
// One lane per permutation over its row in global memory.  The words u do not depend on the row, but row[j] does, on every
// earlier store: the chain is serial along i, and a row cannot be split over lanes.  The alternative, a workgroup per
// permutation with the row in LDS, shortens the step's latency (an LDS access instead of a cache access) but keeps one lane of
// 64 busy and holds n <= 16 K; it needs this kernel behind it for larger n anyway.  DESIGN.md section 25 has the measured
// time of the permutation call, which bounds what that variant could save.  Grid: ceil(n_perm / 64), 64 threads.
__global__ void __launch_bounds__(64) k_quant_perm(int n, int ld, uint64_t seed, uint64_t perm0, int n_perm, int32_t *rows)
{
	const int lane_p = blockIdx.x * 64 + threadIdx.x;
	if (lane_p >= n_perm) return;
	const uint64_t p = perm0 + (uint64_t)lane_p;
	const uint32_t plo = (uint32_t)p, phi = (uint32_t)(p >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
	int32_t *row = rows + (size_t)lane_p * ld;
	if (p == 0) {
		for (int i = 0; i < n; i++) row[i] = i;
		return;
	}
	for (int i0 = 0; i0 < n; i0 += 4) {
		uint32_t u[4];
		philox4x32_10((uint32_t)(i0 >> 2), 1u, plo, phi, k0, k1, u[0], u[1], u[2], u[3]);
#pragma unroll
		for (int b = 0; b < 4; b++) {
			const int i = i0 + b;
			if (i < n) {
				const int j = (int)(((uint64_t)u[b] * (uint64_t)(i + 1)) >> 32);       // 0 <= j <= i
				if (j != i) row[i] = row[j];
				row[j] = i;
			}
		}
	}
}

// k_quant_project: the residual panel and rr of the permutations of a panel:
// v[i] = yt[perm[i]], c_k = q_k . v for all k from v, r = v - sum_k c_k q_k with k in order, rr = sum r^2.
//
// One workgroup per tile of 16 permutations: thread = (permutation col = tid & 15, part o = tid >> 4 of the samples); part o
// takes the steps o >> 2, (o >> 2) + 4, ... and of each step sample 4 step + (o & 3) -- so a wave stores the 64 values of a
// step in the operand's order, 512 contiguous bytes.  A thread adds its terms in step order; the 16 parts of a permutation are
// added in part order by one thread.  The walk is done twice (the projections need all of v first); v is gathered again
// rather than kept.  The columns of the last tile past permutation n_lab - 1 hold zeros, and rr is not written for them.
// Grid: ceil(n_lab / 16), 256 threads.
__global__ void __launch_bounds__(256) k_quant_project(const int32_t *__restrict__ perm, int ld, int n_lab, int n, int kp,
	const double *__restrict__ yt, const double *__restrict__ Q, int nb, double *__restrict__ R, double *__restrict__ rr)
{
	__shared__ double s_part[16][QUANT_MAX_BASIS][16];   // [part][k][col]
	__shared__ double s_c[QUANT_MAX_BASIS][16];
	const int tile = blockIdx.x, tid = threadIdx.x, col = tid & 15, o = tid >> 4, k4 = o & 3;
	const int j = tile * QUANT_TILE + col;
	const bool live = j < n_lab;
	const int32_t *row = perm + (size_t)(live ? j : 0) * ld;
	const int n_steps = kp >> 2;
	double c[QUANT_MAX_BASIS];
#pragma unroll
	for (int k = 0; k < QUANT_MAX_BASIS; k++) c[k] = 0.0;
	for (int step = o >> 2; step < n_steps; step += 4) {
		const int i = 4 * step + k4;
		if (live && i < n) {
			const double v = yt[row[i]];
#pragma unroll
			for (int k = 0; k < QUANT_MAX_BASIS; k++)
				if (k < nb) c[k] += Q[(size_t)k * kp + i] * v;
		}
	}
#pragma unroll
	for (int k = 0; k < QUANT_MAX_BASIS; k++) s_part[o][k][col] = c[k];
	__syncthreads();
	if (tid < 16 * QUANT_MAX_BASIS) {
		const int k = tid >> 4, cc = tid & 15;
		double a = s_part[0][k][cc];
		for (int w = 1; w < 16; w++) a += s_part[w][k][cc];
		s_c[k][cc] = a;
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < QUANT_MAX_BASIS; k++) c[k] = s_c[k][col];
	double ss = 0.0;
	double *out = R + (size_t)tile * n_steps * 64 + (tid & 63);
	for (int step = o >> 2; step < n_steps; step += 4) {
		const int i = 4 * step + k4;
		double r = 0.0;
		if (live && i < n) {
			r = yt[row[i]];
#pragma unroll
			for (int k = 0; k < QUANT_MAX_BASIS; k++)
				if (k < nb) r -= c[k] * Q[(size_t)k * kp + i];
			ss += r * r;
		}
		out[(size_t)step * 64] = r;
	}
	__syncthreads();
	s_part[o][0][col] = ss;
	__syncthreads();
	if (tid < 16 && live) {
		double a = s_part[0][0][tid];
		for (int w = 1; w < 16; w++) a += s_part[w][0][tid];
		rr[j] = a;
	}
}

// k_quant_gram: C[row][perm] = sum_i (double)F[row][i] R[perm][i] for a tile of 16 feature rows x 16 permutations, on
// v_mfma_f64_16x16x4_f64 (the lane map of hibag_k_glm.h): per step of four samples lane l gives a = F[row0 + (l & 15)][4 step +
// (l >> 4)], converted from int8 in registers, and b = the panel's value l of the step; the result has column (permutation) l &
// 15 and row (l >> 4) + 4 reg.  A lane loads 16 bytes of its feature row per four steps.  Wave w takes the groups of four steps
// w, w + 4, ... in order; the waves' tiles are added in wave order.  Feature rows past the last one read as 0 and are not
// stored.  C: float64 [rows][ldc], ldc a multiple of 16.  Grid: (tiles of permutations, ceil(rows / 16)), 256 threads.
__global__ void __launch_bounds__(QUANT_GRAM_WAVES * 64) k_quant_gram(const int8_t *__restrict__ feat, int rows, int kp,
	const double *__restrict__ R, double *__restrict__ C, size_t ldc)
{
	__shared__ double s_tile[QUANT_GRAM_WAVES][256];
	const int tile = blockIdx.x, row0 = blockIdx.y * QUANT_TILE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = lane & 15, k = lane >> 4;
	const int n_steps = kp >> 2, n_groups = kp >> 4;
	const bool has_row = row0 + i < rows;
	const int8_t *f = feat + (size_t)(has_row ? row0 + i : 0) * kp;
	const double *b = R + (size_t)tile * n_steps * 64 + lane;
	quant_d4 acc = {0.0, 0.0, 0.0, 0.0};
	for (int g = wave; g < n_groups; g += QUANT_GRAM_WAVES) {
		uint4 w = *(const uint4 *)(f + (size_t)g * 16);
		if (!has_row) w = make_uint4(0u, 0u, 0u, 0u);
		const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
		for (int s = 0; s < 4; s++) {
			const double a = (double)(int8_t)(word[s] >> (8 * k));
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[(size_t)(4 * g + s) * 64], acc, 0, 0, 0);
		}
	}
#pragma unroll
	for (int r = 0; r < 4; r++) s_tile[wave][(k + 4 * r) * 16 + i] = acc[r];
	__syncthreads();
	if (tid < 256) {
		double a = s_tile[0][tid];
		for (int w = 1; w < QUANT_GRAM_WAVES; w++) a += s_tile[w][tid];
		const int row = row0 + (tid >> 4);
		if (row < rows) C[(size_t)row * ldc + (size_t)tile * QUANT_TILE + (tid & 15)] = a;
	}
}

// The statistic of one test from its Gram cells and rr, one rounding per operation.
__device__ __forceinline__ double quant_stat(const QuantTest &t, double g1, double g2, double rr)
{
	double m, d;
	if (t.row_b < 0) {
		m = (g1 * g1) / t.a11;
		d = 1.0;
	} else {
		const double t1 = t.a22 * (g1 * g1), t2 = ((2.0 * t.a12) * g1) * g2, t3 = t.a11 * (g2 * g2);
		m = ((t1 - t2) + t3) / t.det;
		d = 2.0;
	}
	const double den = rr - m;
	if (!(den > 0.0)) return __builtin_nan("");
	return (m / d) / (den / t.df);
}

// k_quant_stat: the statistics of a panel of permutations from the Gram C [rows][ldc] and rr [n_lab].  Lane = permutation,
// the tests walked in order, the maximum a running value of the lane; outputs as k_assoc_stat's:
//   stat_out   [n_test] or NULL: the statistic of permutation 0 of the panel (the observed run, a panel of its own)
//   max_out    [n_lab] or NULL:  the largest non-NaN statistic of each permutation, NaN if there is none
//   stat_obs / count  [n_test] or NULL: count[t] += the permutations with stat >= stat_obs[t] (false where either is NaN)
// Grid: ceil(n_lab / 64), 64 threads.
__global__ void __launch_bounds__(64) k_quant_stat(const double *__restrict__ C, size_t ldc, const double *__restrict__ rr, int n_lab,
	const QuantTest *__restrict__ tests, int n_test, double *__restrict__ stat_out, double *__restrict__ max_out,
	const double *__restrict__ stat_obs, unsigned long long *__restrict__ count)
{
	const int j = blockIdx.x * 64 + threadIdx.x;
	const bool live = j < n_lab;
	const size_t col = live ? (size_t)j : 0;
	const double r2 = rr[col];
	double best = -1.0;                                   // (every statistic is >= 0)
	for (int t = 0; t < n_test; t++) {
		const QuantTest qt = tests[t];
		double st = __builtin_nan("");
		if (qt.row_a >= 0) {
			const double g1 = C[(size_t)qt.row_a * ldc + col];
			const double g2 = qt.row_b >= 0 ? C[(size_t)qt.row_b * ldc + col] : 0.0;
			st = quant_stat(qt, g1, g2, r2);
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
