// hibag_k_score.h -- kernels of hlaAssocScore: covariate-adjusted score tests of a case / control trait on the tests (or sets
// of feature rows) of an association handle, under the observed residuals and under Lin's multiplier resampling of them
// (DESIGN.md section 28).  Host side: hibag_assoc.hip.
//
// Under the base model y ~ covariates, with the basis q_0 .. q_q orthonormal under the weights w (Q'WQ = I), the score of a
// feature row under replicate p is g[row][p] = sum_i F[row][i] r_i, r the sign-flipped residual e o s_p projected off the
// basis; a set's statistic is |L^-1 g_set|^2 with L the Cholesky factor of the set's projected information.  All rows under
// all replicates of a panel are one real-valued Gram matrix, int8 feature rows x FP64 residual rows: k_quant_gram of
// hibag_k_quant.h, unchanged, on the panel layout described there.  The kernels here make what is computed once per handle
// (k_score_proj, k_score_setgram), build the residual panel from the signs (k_score_coef, k_score_project) and turn the Gram into
// statistics, per-replicate maxima per degree of freedom, and counts (k_score_stat).
//
// Order of every sum: as hibag_k_quant.h -- a thread adds its own terms in index order, parts are added in part order, a
// wave walks its steps in order and the waves' tiles are added in wave order.  No floating-point atomics.
#ifndef HIBAG_K_SCORE_H_
#define HIBAG_K_SCORE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hibag_k_philox.h"
#include "hibag_k_quant.h"

#define SCORE_MAX_ROWS 30           // feature rows of a set (two 16-row blocks of the set Gram, as the 32-slot design of hibag_k_glmw.h)
#define SCORE_SET_LD 32             // row stride of a set's Gram in k_score_setgram's output
#define SCORE_BLOCK 128             // replicates whose signs one Philox call holds for a sample
#define SCORE_PARTS 4               // parts of the samples in k_score_project: part o takes the samples 4 step + o
#define SCORE_THREADS (SCORE_BLOCK * SCORE_PARTS)  // k_score_project's workgroup
#define SCORE_CHUNK 256             // samples whose sign words, basis rows, e and w a workgroup of k_score_project holds at a time
#define SCORE_SEG 1024              // samples of a segment: a workgroup of k_score_coef / k_score_project walks one
#define SCORE_STREAM 2u             // counter word 1 of the sign stream (0: hibag_k_assoc.h, 1: k_quant_perm)
#define SCORE_GRAM_WAVES 4          // waves of k_score_setgram's workgroup, which split the samples

// What k_score_stat needs of a set: its kept rows rows[row0 .. row0 + d) in column order, the packed lower-triangular factor
// L at l_off (row a at a (a + 1) / 2), and the slot of its degrees of freedom among the distinct ones.  d = 0: NaN.
struct ScoreSet {
	int row0, d, slot, l_off;
};

// The 128 sign bits of sample i for the replicates of block blk (= p >> 7): DESIGN.md section 28 item 5.
__device__ __forceinline__ uint4 score_sign_words(uint32_t i, uint64_t blk, uint64_t seed)
{
	uint4 w;
	philox4x32_10(i, SCORE_STREAM, (uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w.x, w.y, w.z, w.w);
	return w;
}

// replicate p's sign from its block's words: true = -1.  Replicate 0 is all +1.
__device__ __forceinline__ bool score_negative(const uint32_t *words, uint64_t p)
{
	const uint32_t at = (uint32_t)p & (SCORE_BLOCK - 1);
	return p != 0 && ((words[at >> 5] >> (at & 31)) & 1u);
}

// k_score_proj: proj[row][k] = sum_i F[row][i] (w_i q_k[i]) for the nb basis rows Q [nb][kp].  One workgroup per feature row,
// thread t takes the samples t, t + 256, ...; the parts are added in quant_block_sum's tree.  Grid: rows, 256 threads.
__global__ void __launch_bounds__(256) k_score_proj(const int8_t *__restrict__ feat, int kp, int n, const double *__restrict__ w,
	const double *__restrict__ Q, int nb, double *__restrict__ proj)
{
	__shared__ double s[256];
	const int row = blockIdx.x, tid = threadIdx.x;
	const int8_t *f = feat + (size_t)row * kp;
	for (int k = 0; k < nb; k++) {
		const double *q = Q + (size_t)k * kp;
		double a = 0.0;
		for (int i = tid; i < n; i += 256) a += (double)f[i] * (w[i] * q[i]);
		a = quant_block_sum(a, s);
		if (tid == 0) proj[(size_t)row * nb + k] = a;
	}
}

// k_score_setgram: the weighted Gram of a set of m <= 30 feature rows, S[a][b] = sum_i (w_i F[a][i]) F[b][i], on
// v_mfma_f64_16x16x4_f64 (the lane map of hibag_k_glm.h): the set's rows in two blocks of 16, the lower blocks (0, 0), (1, 0)
// and (1, 1) per step of four samples, the last two only where m > 16.  Lane l gives row (l & 15) of a block at sample
// 4 step + (l >> 4), converted from int8 in registers, 16 bytes of each of its two rows per four steps; rows past m read as 0.
// Wave v takes the groups of four steps v, v + 4, ...; the waves' tiles are added in wave order through LDS.  One workgroup per
// set.  S: float64 [n_sets][32][32], the cells (a, b) of the three lower blocks written (the host reads a >= b), w zero on the
// padding samples.  Grid: n_sets, 256 threads.
__global__ void __launch_bounds__(SCORE_GRAM_WAVES * 64) k_score_setgram(const int8_t *__restrict__ feat, int kp,
	const double *__restrict__ w, const int32_t *__restrict__ set_start, const int32_t *__restrict__ set_rows, double *__restrict__ S)
{
	__shared__ double s_tile[SCORE_GRAM_WAVES][3][256];
	const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = lane & 15, k = lane >> 4;
	const int m = set_start[t + 1] - set_start[t];
	const int32_t *rows = set_rows + set_start[t];
	const bool has0 = i < m, has1 = 16 + i < m, wide = m > 16;
	const int8_t *f0 = feat + (size_t)(has0 ? rows[i] : 0) * kp;
	const int8_t *f1 = feat + (size_t)(has1 ? rows[16 + i] : 0) * kp;
	const int n_groups = kp >> 4;
	quant_d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc10 = acc00, acc11 = acc00;
	for (int g = wave; g < n_groups; g += SCORE_GRAM_WAVES) {
		uint4 u0 = *(const uint4 *)(f0 + (size_t)g * 16), u1 = make_uint4(0u, 0u, 0u, 0u);
		if (!has0) u0 = make_uint4(0u, 0u, 0u, 0u);
		if (has1) u1 = *(const uint4 *)(f1 + (size_t)g * 16);
		const uint32_t word0[4] = {u0.x, u0.y, u0.z, u0.w}, word1[4] = {u1.x, u1.y, u1.z, u1.w};
#pragma unroll
		for (int s = 0; s < 4; s++) {
			const double wt = w[16 * g + 4 * s + k];
			const double x0 = (double)(int8_t)(word0[s] >> (8 * k)), x1 = (double)(int8_t)(word1[s] >> (8 * k));
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

// k_score_signs: the signs themselves, out int8 [n_lab][ld]: row j is replicate p0 + j, +1 or -1 per kept sample (for tests
// of the generator).  Thread = sample, the replicates walked in order, one Philox call per block of 128 entered.
// Grid: ceil(n / 256), 256 threads.
__global__ void __launch_bounds__(256) k_score_signs(int n, size_t ld, uint64_t seed, uint64_t p0, int n_lab, int8_t *__restrict__ out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint4 w = make_uint4(0u, 0u, 0u, 0u);
	uint64_t have = ~(uint64_t)0;
	for (int j = 0; j < n_lab; j++) {
		const uint64_t p = p0 + (uint64_t)j;
		if ((p >> 7) != have) { have = p >> 7; w = score_sign_words((uint32_t)i, have, seed); }
		const uint32_t words[4] = {w.x, w.y, w.z, w.w};
		out[(size_t)j * ld + i] = score_negative(words, p) ? -1 : 1;
	}
}

// k_score_coef and k_score_project: the residual panel of the replicates p0 .. p0 + n_lab - 1 (DESIGN.md section 28 items 5
// and 6): v_i = e_i s_ip, c_k = sum_i q_k[i] v_i for all k from v (k_score_coef), r_i = v_i - w_i sum_k c_k q_k[i] with k in
// order (k_score_project), written in k_quant_project's layout for k_quant_gram.  Two walks over the samples, as
// k_quant_project's, because the projections need all of v first.
//
// Each kernel runs over a grid of (128 replicates of the panel, a segment of SCORE_SEG samples): thread = (replicate col =
// tid & 127, part o = tid >> 7), part o takes the samples 4 step + o of its segment in step order; the four parts of a
// replicate are added in part order, then the segments in segment order -- so c depends on n and the constants here alone.
// (The segments are what fills the device: a panel of 3,312 replicates is 26 workgroups a segment.)  A segment's samples go
// by in chunks of 256, and what a chunk needs is shared through LDS (score_stage).  The sign words: thread t makes the Philox
// call of sample chunk + (t & 255) for block t >> 8, the second block only where the workgroup's replicates straddle two
// blocks of 128, which a call starting at replicate 1 always does; so the generator runs once or twice per (sample, 128
// replicates) and walk, not per (sample, tile).  The chunk's basis rows, e and w: loaded once and coalesced; every thread of
// a wave reads the same sample's values, a broadcast from LDS where a load from memory would cost its latency at every
// step.  The second walk stages the chunks again rather than keeping them.  The columns of the last tile past replicate
// n_lab - 1 and the padding samples hold zeros; tiles past the last are not written.
struct ScoreStage {
	uint4 words[2][SCORE_CHUNK];
	double buf[(SCORE_PARTS - 1) * QUANT_MAX_BASIS * SCORE_BLOCK];   // a chunk's q [13][256], e [256], w [256]; between the walks the parts' sums
};
static_assert((QUANT_MAX_BASIS + 2) * SCORE_CHUNK <= (SCORE_PARTS - 1) * QUANT_MAX_BASIS * SCORE_BLOCK, "a chunk fits the parts' room");

__device__ __forceinline__ void score_stage(ScoreStage &S, int i0, int n, int kp, uint64_t seed, uint64_t blk0, bool two,
	const double *__restrict__ e, const double *__restrict__ w, const double *__restrict__ Q, int nb)
{
	const int tid = threadIdx.x, c = tid & (SCORE_CHUNK - 1), b = tid >> 8;
	__syncthreads();                                        // (the chunk before is read)
	if (i0 + c < n && (b == 0 || two)) S.words[b][c] = score_sign_words((uint32_t)(i0 + c), blk0 + (uint64_t)b, seed);
	for (int at = tid; at < (QUANT_MAX_BASIS + 2) * SCORE_CHUNK; at += SCORE_THREADS) {
		const int r = at / SCORE_CHUNK, i = i0 + (at & (SCORE_CHUNK - 1));
		double v = 0.0;
		if (i < kp) {
			if (r < QUANT_MAX_BASIS) { if (r < nb) v = Q[(size_t)r * kp + i]; }
			else v = r == QUANT_MAX_BASIS ? e[i] : w[i];
		}
		S.buf[at] = v;
	}
	__syncthreads();
}

// the fields of a thread of the two kernels below
struct ScoreLane {
	int col, o, j, which;
	bool live, two;
	uint64_t p, blk0;
};

__device__ __forceinline__ ScoreLane score_lane(uint64_t p0, int n_lab)
{
	ScoreLane t;
	t.col = threadIdx.x & (SCORE_BLOCK - 1);
	t.o = threadIdx.x >> 7;
	t.j = blockIdx.x * SCORE_BLOCK + t.col;
	t.live = t.j < n_lab;
	t.p = p0 + (uint64_t)t.j;
	const uint64_t first = p0 + (uint64_t)blockIdx.x * SCORE_BLOCK;
	t.blk0 = first >> 7;
	t.two = (first & (SCORE_BLOCK - 1)) != 0;
	t.which = t.live ? (int)((t.p >> 7) - t.blk0) : 0;
	return t;
}

// k_score_coef: the first walk.  part[seg][k][j] = the sum of q_k[i] v_i over the samples of segment seg for replicate j of
// the panel (0 for the columns past n_lab - 1), row stride ldp.  Grid: (ceil(n_lab / 128), ceil(n / SCORE_SEG)), 512 threads.
__global__ void __launch_bounds__(SCORE_THREADS) k_score_coef(uint64_t seed, uint64_t p0, int n_lab, int n, int kp,
	const double *__restrict__ e, const double *__restrict__ w, const double *__restrict__ Q, int nb, double *__restrict__ part, size_t ldp)
{
	__shared__ ScoreStage S;
	const double *s_q = S.buf, *s_e = S.buf + QUANT_MAX_BASIS * SCORE_CHUNK;
	double (*s_part)[QUANT_MAX_BASIS][SCORE_BLOCK] = (double (*)[QUANT_MAX_BASIS][SCORE_BLOCK])S.buf;
	const ScoreLane t = score_lane(p0, n_lab);
	const int seg = blockIdx.y, i_lo = seg * SCORE_SEG, i_hi = min(n, i_lo + SCORE_SEG);
	double c[QUANT_MAX_BASIS];
#pragma unroll
	for (int k = 0; k < QUANT_MAX_BASIS; k++) c[k] = 0.0;
	for (int i0 = i_lo; i0 < i_hi; i0 += SCORE_CHUNK) {
		score_stage(S, i0, n, kp, seed, t.blk0, t.two, e, w, Q, nb);
		for (int s = 0; s < SCORE_CHUNK / SCORE_PARTS; s++) {
			const int at = SCORE_PARTS * s + t.o;
			if (i0 + at >= i_hi) break;
			if (t.live) {
				const double v = score_negative((const uint32_t *)&S.words[t.which][at], t.p) ? -s_e[at] : s_e[at];
#pragma unroll
				for (int k = 0; k < QUANT_MAX_BASIS; k++)
					if (k < nb) c[k] += s_q[k * SCORE_CHUNK + at] * v;
			}
		}
	}
	__syncthreads();                                        // (the last chunk is read: its room takes the parts' sums)
	if (t.o > 0) {
#pragma unroll
		for (int k = 0; k < QUANT_MAX_BASIS; k++) s_part[t.o - 1][k][t.col] = c[k];
	}
	__syncthreads();
	if (t.o == 0) {
#pragma unroll
		for (int k = 0; k < QUANT_MAX_BASIS; k++) {
			double a = c[k];
			for (int v = 0; v < SCORE_PARTS - 1; v++) a += s_part[v][k][t.col];
			part[((size_t)seg * QUANT_MAX_BASIS + k) * ldp + t.j] = a;
		}
	}
}

// k_score_project: the second walk.  c_k = the segments' parts added in segment order; the workgroup writes the panel of its
// segment of the samples (the padding samples included).  Grid: (ceil(n_lab / 128), ceil(kp / SCORE_SEG)), 512 threads.
__global__ void __launch_bounds__(SCORE_THREADS) k_score_project(uint64_t seed, uint64_t p0, int n_lab, int n, int kp,
	const double *__restrict__ e, const double *__restrict__ w, const double *__restrict__ Q, int nb, const double *__restrict__ part,
	size_t ldp, double *__restrict__ R)
{
	__shared__ ScoreStage S;
	const double *s_q = S.buf, *s_e = S.buf + QUANT_MAX_BASIS * SCORE_CHUNK, *s_w = s_e + SCORE_CHUNK;
	const ScoreLane t = score_lane(p0, n_lab);
	const int n_steps = kp >> 2, tiles = (n_lab + QUANT_TILE - 1) / QUANT_TILE, tile = t.j >> 4;
	const int n_seg = (n + SCORE_SEG - 1) / SCORE_SEG, i_lo = blockIdx.y * SCORE_SEG, i_hi = min(kp, i_lo + SCORE_SEG);
	double c[QUANT_MAX_BASIS];
#pragma unroll
	for (int k = 0; k < QUANT_MAX_BASIS; k++) {
		double a = 0.0;
		if (k < nb) {
			a = part[(size_t)k * ldp + t.j];
			for (int s = 1; s < n_seg; s++) a += part[((size_t)s * QUANT_MAX_BASIS + k) * ldp + t.j];
		}
		c[k] = a;
	}
	double *out = R + (size_t)tile * n_steps * 64 + t.o * 16 + (t.col & 15);
	for (int i0 = i_lo; i0 < i_hi; i0 += SCORE_CHUNK) {
		score_stage(S, i0, n, kp, seed, t.blk0, t.two, e, w, Q, nb);
		for (int s = 0; s < SCORE_CHUNK / SCORE_PARTS; s++) {
			const int at = SCORE_PARTS * s + t.o, i = i0 + at;
			if (i >= i_hi) break;
			double r = 0.0;
			if (t.live && i < n) {
				const double v = score_negative((const uint32_t *)&S.words[t.which][at], t.p) ? -s_e[at] : s_e[at];
				double u = 0.0;
#pragma unroll
				for (int k = 0; k < QUANT_MAX_BASIS; k++)
					if (k < nb) u += c[k] * s_q[k * SCORE_CHUNK + at];
				r = v - s_w[at] * u;
			}
			if (tile < tiles) out[(size_t)(i >> 2) * 64] = r;
		}
	}
}

// k_score_stat: the statistics of a panel of replicates from the Gram C [rows][ldc].  Lane = replicate, the sets walked in
// order: forward substitution L t = g over the set's kept rows in order (t in the lane's column of LDS), T = sum t_a^2 with a
// in order, one rounding per operation; the running maxima, one per distinct number of degrees of freedom, in the lane's
// column of LDS.  Outputs:
//   stat_out   [n_sets] or NULL: the statistic of replicate 0 of the panel (the observed run, a panel of its own)
//   max_out    [n_lab][n_df] or NULL: per replicate and slot the largest non-NaN statistic of the sets of that slot, NaN if none
//   stat_obs / count  [n_sets] or NULL: count[t] += the replicates with T >= stat_obs[t] (false where either is NaN)
// Grid: ceil(n_lab / 64), 64 threads.
__global__ void __launch_bounds__(64) k_score_stat(const double *__restrict__ C, size_t ldc, int n_lab, const ScoreSet *__restrict__ sets,
	int n_sets, const int32_t *__restrict__ rows, const double *__restrict__ Lf, int n_df, double *__restrict__ stat_out,
	double *__restrict__ max_out, const double *__restrict__ stat_obs, unsigned long long *__restrict__ count)
{
	__shared__ double s_t[SCORE_MAX_ROWS][64];
	__shared__ double s_best[SCORE_MAX_ROWS][64];
	const int lane = threadIdx.x, j = blockIdx.x * 64 + lane;
	const bool live = j < n_lab;
	const size_t col = live ? (size_t)j : 0;
	for (int s = 0; s < n_df; s++) s_best[s][lane] = -1.0;     // (every statistic is >= 0)
	for (int t = 0; t < n_sets; t++) {
		const ScoreSet S = sets[t];
		double st = __builtin_nan("");
		if (S.d > 0) {
			const double *L = Lf + S.l_off;
			const int32_t *rw = rows + S.row0;
			double T = 0.0;
			for (int a = 0; a < S.d; a++) {
				const double *La = L + a * (a + 1) / 2;
				double v = C[(size_t)rw[a] * ldc + col];
				for (int b = 0; b < a; b++) v -= La[b] * s_t[b][lane];
				const double ta = v / La[a];
				s_t[a][lane] = ta;
				T += ta * ta;
			}
			st = T;
			const double cur = s_best[S.slot][lane];
			s_best[S.slot][lane] = st > cur ? st : cur;       // (false for NaN)
		}
		if (stat_out && j == 0) stat_out[t] = st;
		if (count) {
			const unsigned long long hits = __ballot(live && st >= stat_obs[t]);
			if (lane == 0 && hits) atomicAdd(count + t, (unsigned long long)__popcll(hits));
		}
	}
	if (live && max_out)
		for (int s = 0; s < n_df; s++) {
			const double b = s_best[s][lane];
			max_out[(size_t)j * n_df + s] = b < 0 ? __builtin_nan("") : b;
		}
}

#endif
