// hibag_k_draw.h -- part of hibag_kernels.hip (included there behind hibag_k_finish.h, whose normalised() it shares):
// k_finish_draw, the finish of the draw entries (hibag_hip_predict_draw*): per sample n_draw allele pairs drawn from the
// NORMALISED ensemble matrix -- the values k_finish_prob would write -- with the drawn pairs' probabilities, in place of the
// call / dosage / posterior-matrix finish.  n_draw * 20 + 8 bytes per sample leave the device instead of 8 * n_cell.
//
// The sampling rule (the contract), p[c] the sample's normalised posterior in cell order:
//   cum[c] = cum[c - 1] + p[c], plain FP64 additions in cell order (no FMA: the translation unit is built with
//   -ffp-contract=off), S = cum[n_cell - 1];
//   draw t of sample i (i in the CALLER's numbering: the launcher is told the index of lane 0) uses
//   u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 with (w0, w1, ., .) = Philox4x32-10(counter (i lo, i hi, t, 0), key (seed lo, seed hi));
//   the drawn cell is the first c in cell order with cum[c] > u * S (one FP64 multiply) -- a cell with p[c] == 0 repeats
//   cum[c - 1] and is never the first; if none qualifies, the last cell with p[c] > 0;
//   S > 0 false: every draw of the sample is NA_INTEGER / NA_INTEGER, prob = NaN if S is NaN (a sample poisoned by an
//   underflow, a batch poisoned by a failed hand-over), 0.0 otherwise.
// A sample's draws depend on (seed, i, t) and its posterior alone: not on batches, slices, routes or n_draw.
//
// Shape: lane = sample, like every finish kernel (`part` is cell-major: a wavefront's loads are coalesced, nothing crosses
// lanes, there is no LDS and no barrier).  The running sum is serial in cell order, so a wavefront walks its 64 samples' cells
// twice, eight rows in flight: once for S, once -- with the same additions, hence the same cum bit for bit -- for the search.
// A wavefront holds DRAW_PER_WAVE draws: their thresholds u * S and their cells live in registers, updated per cell by fully
// unrolled selects, so no index into the lists is ever a run-time value and nothing goes to a private segment.  Further draws
// go to further wavefronts of the workgroup (NW = 1, 2, 4: up to 16, 32, 64 draws; the launcher takes the smallest that holds
// the call's n_draw), each repeating the scan of the same 64 samples out of the same cache lines.
#ifndef HIBAG_K_DRAW_H_
#define HIBAG_K_DRAW_H_

#include "hibag_k_philox.h"         // philox4x32_10, shared with the association tests' permutations

#define DRAW_PER_WAVE 16

// one cell of the search: the running sum, then every draw that has no cell yet and whose threshold the sum has passed
__device__ __forceinline__ void draw_step(double x, int c, double &cum, int &last, const double (&thr)[DRAW_PER_WAVE],
	int (&idx)[DRAW_PER_WAVE])
{
	cum += x;
	last = x > 0 ? c : last;
#pragma unroll
	for (int j = 0; j < DRAW_PER_WAVE; j++) idx[j] = (idx[j] < 0 && cum > thr[j]) ? c : idx[j];
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_finish_draw(HibagModelView M, HibagBatchView B,
	const double *__restrict__ part, int n_draw, uint64_t seed, int64_t sample0, int32_t *__restrict__ H1,
	int32_t *__restrict__ H2, double *__restrict__ prob, double *__restrict__ matching)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int s = blockIdx.x * 64 + lane;
	const int P = M.n_cell;
	const size_t np = (size_t)B.n_pad;
	const int t0 = wave * DRAW_PER_WAVE;
	if (t0 >= n_draw) return;                         // (33 .. 48 draws: the fourth wavefront has none; wave-uniform, no barrier below)
	const double sum_w = part[(size_t)P * np + s];
	const bool scale = sum_w > 0, poisoned = sum_w != sum_w;       // (poisoned batch: every value is NaN, as k_finish_prob writes it)
	const double ff = 1.0 / sum_w;
	// pass 1: S
	double S = 0;
	int p = 0;
	for (; p + 8 <= P; p += 8) {                  // eight rows in flight, added in cell order
		double v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = part[(size_t)(p + j) * np + s];
#pragma unroll
		for (int j = 0; j < 8; j++) S += poisoned ? sum_w : normalised(v[j], scale, ff);
	}
	for (; p < P; p++) S += poisoned ? sum_w : normalised(part[(size_t)p * np + s], scale, ff);
	// the thresholds of this wavefront's draws
	const uint64_t i = (uint64_t)(sample0 + (int64_t)s);
	double thr[DRAW_PER_WAVE];
	int idx[DRAW_PER_WAVE];
#pragma unroll
	for (int j = 0; j < DRAW_PER_WAVE; j++) {
		uint32_t w0, w1;
		philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)(t0 + j), 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w0, w1);
		const double u = (double)(((uint64_t)(w0 >> 5) << 26) + (uint64_t)(w1 >> 6)) * 0x1p-53;       // (exact: 53 bits)
		thr[j] = u * S;
		idx[j] = -1;
	}
	// pass 2: the same sums again, and the search
	double cum = 0;
	int last = -1;
	for (p = 0; p + 8 <= P; p += 8) {
		double v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = part[(size_t)(p + j) * np + s];
#pragma unroll
		for (int j = 0; j < 8; j++) draw_step(poisoned ? sum_w : normalised(v[j], scale, ff), p + j, cum, last, thr, idx);
	}
	for (; p < P; p++) draw_step(poisoned ? sum_w : normalised(part[(size_t)p * np + s], scale, ff), p, cum, last, thr, idx);
	if (s >= B.n_samp) return;
	const bool any = S > 0;                           // (false for NaN)
	const size_t at = (size_t)s * (size_t)n_draw + (size_t)t0;
#pragma unroll
	for (int j = 0; j < DRAW_PER_WAVE; j++) {
		if (t0 + j >= n_draw) continue;
		const int cell = !any ? -1 : idx[j] >= 0 ? idx[j] : last;
		int b1 = NA_INTEGER, b2 = NA_INTEGER;
		double pr = S != S ? S : 0.0;
		if (cell >= 0) {
			cell_pair(cell, M.n_hla, b1, b2);
			pr = normalised(part[(size_t)cell * np + s], scale, ff);      // the drawn pair's posterior: the value pass 2 added
		}
		H1[at + j] = b1; H2[at + j] = b2;
		prob[at + j] = pr;
	}
	if (matching && wave == 0) matching[s] = matching_of(part, P, np, s);
}

#endif
