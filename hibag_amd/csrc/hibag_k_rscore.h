// hibag_k_rscore.h -- the score tests of hibag_k_score.h on REAL-VALUED feature rows (hlaAssocHaplo: a haplotype's expected
// dosage per sample).  Host side: hibag_assoc.hip (hibag_hip_assoc_rscore_sets).
//
// X is float64 [m][kp], zero on the padding samples.  Everything that does not read the features -- the base fit, the weighted
// basis, the sign stream, the residual panels (k_score_coef, k_score_project) and k_score_stat -- is hibag_k_score.h's, unchanged;
// the three kernels here take the place of k_score_proj, k_score_setgram and k_quant_gram and keep their reduction trees: a
// thread adds its own terms in index order, parts are added in quant_block_sum's tree, a wave walks its groups of four steps
// in order and the waves' tiles are added in wave order.  So every number depends on n, on its own row and replicate and on
// compile-time constants alone, as section 28 item 10 asks.  No floating-point atomics.
#ifndef HIBAG_K_RSCORE_H_
#define HIBAG_K_RSCORE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hibag_k_quant.h"
#include "hibag_k_score.h"

// k_rscore_proj: proj[row][k] = sum_i X[row][i] (w_i q_k[i]) for the nb basis rows Q [nb][kp]: k_score_proj with float64 rows.
// Grid: rows, 256 threads.
__global__ void __launch_bounds__(256) k_rscore_proj(const double *__restrict__ X, int kp, int n, const double *__restrict__ w,
	const double *__restrict__ Q, int nb, double *__restrict__ proj)
{
	__shared__ double s[256];
	const int row = blockIdx.x, tid = threadIdx.x;
	const double *f = X + (size_t)row * kp;
	for (int k = 0; k < nb; k++) {
		const double *q = Q + (size_t)k * kp;
		double a = 0.0;
		for (int i = tid; i < n; i += 256) a += f[i] * (w[i] * q[i]);
		a = quant_block_sum(a, s);
		if (tid == 0) proj[(size_t)row * nb + k] = a;
	}
}

// k_rscore_setgram: the weighted Gram of a set of m <= 30 rows of X, S[a][b] = sum_i (w_i X[a][i]) X[b][i]: k_score_setgram
// with float64 rows -- the same blocks, lane map, wave split and output (S float64 [n_sets][32][32], the three lower 16 x 16
// blocks written).  Lane l gives row (l & 15) of a block at sample 4 step + (l >> 4); rows past m read as 0.
// Grid: n_sets, 256 threads.
__global__ void __launch_bounds__(SCORE_GRAM_WAVES * 64) k_rscore_setgram(const double *__restrict__ X, int kp,
	const double *__restrict__ w, const int32_t *__restrict__ set_start, const int32_t *__restrict__ set_rows, double *__restrict__ S)
{
	__shared__ double s_tile[SCORE_GRAM_WAVES][3][256];
	const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = lane & 15, k = lane >> 4;
	const int m = set_start[t + 1] - set_start[t];
	const int32_t *rows = set_rows + set_start[t];
	const bool has0 = i < m, has1 = 16 + i < m, wide = m > 16;
	const double *f0 = X + (size_t)(has0 ? rows[i] : 0) * kp;
	const double *f1 = X + (size_t)(has1 ? rows[16 + i] : 0) * kp;
	const int n_groups = kp >> 4;
	quant_d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc10 = acc00, acc11 = acc00;
	for (int g = wave; g < n_groups; g += SCORE_GRAM_WAVES) {
#pragma unroll
		for (int s = 0; s < 4; s++) {
			const int at = 16 * g + 4 * s + k;
			const double wt = w[at];
			const double x0 = has0 ? f0[at] : 0.0, x1 = has1 ? f1[at] : 0.0;
			acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(wt * x0, x0, acc00, 0, 0, 0);
			if (wide) {
				const double a1 = wt * x1;
				acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x0, acc10, 0, 0, 0);
				acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x1, acc11, 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int r = 0; r < 4; r++) {
		s_tile[wave][0][(k + 4 * r) * 16 + i] = acc00[r];
		s_tile[wave][1][(k + 4 * r) * 16 + i] = acc10[r];
		s_tile[wave][2][(k + 4 * r) * 16 + i] = acc11[r];
	}
	__syncthreads();
	double *out = S + (size_t)t * SCORE_SET_LD * SCORE_SET_LD;
#pragma unroll
	for (int b = 0; b < 3; b++) {
		double a = s_tile[0][b][tid];
		for (int v = 1; v < SCORE_GRAM_WAVES; v++) a += s_tile[v][b][tid];
		const int row = (b > 0 ? 16 : 0) + (tid >> 4), col = (b > 1 ? 16 : 0) + (tid & 15);
		out[row * SCORE_SET_LD + col] = a;
	}
}

// k_rscore_gram: C[row][rep] = sum_i X[row][i] R[rep][i] for a tile of 16 rows x 16 replicates on v_mfma_f64_16x16x4_f64:
// k_quant_gram with the a operand loaded as float64 -- per step of four samples lane l gives a = X[row0 + (l & 15)][4 step +
// (l >> 4)] and b = the panel's value l of the step (the layout k_score_project writes); the result has column (replicate)
// l & 15 and row (l >> 4) + 4 reg.  Wave w takes the groups of four steps w, w + 4, ... in order; the waves' tiles are added in
// wave order.  Rows past the last one read as 0 and are not stored.  The four lanes of a row read 32 contiguous bytes per
// step; a row's 128 bytes of a group come in over its four steps.  C: float64 [rows][ldc], ldc a multiple of 16.
// Grid: (tiles of replicates, ceil(rows / 16)), 256 threads.
__global__ void __launch_bounds__(QUANT_GRAM_WAVES * 64) k_rscore_gram(const double *__restrict__ X, int rows, int kp,
	const double *__restrict__ R, double *__restrict__ C, size_t ldc)
{
	__shared__ double s_tile[QUANT_GRAM_WAVES][256];
	const int tile = blockIdx.x, row0 = blockIdx.y * QUANT_TILE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = lane & 15, k = lane >> 4;
	const int n_steps = kp >> 2, n_groups = kp >> 4;
	const bool has_row = row0 + i < rows;
	const double *f = X + (size_t)(has_row ? row0 + i : 0) * kp + k;
	const double *b = R + (size_t)tile * n_steps * 64 + lane;
	quant_d4 acc = {0.0, 0.0, 0.0, 0.0};
	for (int g = wave; g < n_groups; g += QUANT_GRAM_WAVES) {
		double a[4];
#pragma unroll
		for (int s = 0; s < 4; s++) a[s] = has_row ? f[16 * g + 4 * s] : 0.0;
#pragma unroll
		for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[(size_t)(4 * g + s) * 64], acc, 0, 0, 0);
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

#endif
