// hibag_k_groups.h -- part of hibag_kernels.hip (included there behind hibag_k_finish.h, whose normalised() it shares):
// k_finish_groups, the finish of the group entries (hibag_hip_predict_groups*): per sample and per partition of the model's
// alleles into groups, the best PAIR OF GROUPS under the collapsed posterior, its probability and, optionally, the expected
// dosage of every group -- in place of the call / dosage / posterior-matrix finish.  n_part * 16 + 8 bytes per sample leave
// the device (plus 8 per group with the dosages) instead of 8 * n_cell.
//
// The contract, p[c] the sample's normalised posterior in cell order -- the values k_finish_prob
// would write --, m(h) the group of allele h in the partition:
//   bin (a <= b) has index b + a (2G - a - 1) / 2; cell (h1, h2) belongs to bin (min, max) of (m(h1), m(h2));
//   B[bin] = the sum of p[c] over the bin's cells in increasing cell order, plain FP64 additions from +0.0 (no FMA: the
//   translation unit is built with -ffp-contract=off);
//   the call is the first bin in bin order with best < B strictly (best starts at 0: BestGuessEnsemble's rule on bins), NA / NA
//   with probability 0.0 if there is none, NA / NA with probability NaN if the weight sum is NaN (a poisoned batch);
//   D[g] = the sum over the cells with an allele in g, in increasing cell order, of p[c] (one allele in g) or 2 p[c] (both),
//   the weight sum itself where that is NaN (as finish_dosage).
// With m(h) = h this is finish_call and finish_dosage bit for bit.
//
// Shape.  The other finish kernels are lane = sample and read `part` cell-major; once per partition that would read the
// ensemble sums n_part times.  Here a workgroup stages the normalised posterior of `tile` samples in LDS ONCE and its threads
// take the (sample of the tile, partition) pairs, partition fastest.  A pair's thread walks the partition's LIST: the cells
// sorted by (bin, cell), the last cell of every bin marked.  Per entry one LDS read and one addition; at a mark the compare and
// the reset, as selects.  Every thread makes exactly n_cell steps, the lists are partition-minor (a wavefront's loads of step
// i are consecutive words), nothing crosses lanes.  The dosage is a second walk of the same form over a second list: the
// cells sorted by (group, cell) -- a cell with alleles in two groups is listed twice --, marked where the cell counts twice and
// where a group ends, padded to the longest partition of the plan.  A group without alleles has one entry that adds +0.0.
// LDS = false is the same walk reading `part` itself: models whose posterior does not fit (8 * n_cell bytes per sample
// against HIBAG_GROUPS_LDS_DOUBLES), and HIBAG_GROUPS_NO_LDS=1.
#ifndef HIBAG_K_GROUPS_H_
#define HIBAG_K_GROUPS_H_

#define GROUPS_THREADS 256
#define GRP_END 0x80000000u                      // the last entry of a bin (call list) / of a group (dosage list)
#define GRP_TWICE 0x40000000u                    // dosage list: both alleles of the cell are in the group
#define GRP_ZERO 0x20000000u                     // dosage list: the one entry of a group without alleles
#define GRP_CELL 0x1fffffffu

template <bool LDS>
__global__ __launch_bounds__(GROUPS_THREADS) void k_finish_groups(HibagModelView M, HibagBatchView B,
	const double *__restrict__ part, HibagGroupsView V, int tile, int32_t *__restrict__ G1, int32_t *__restrict__ G2,
	double *__restrict__ prob, double *__restrict__ matching, double *__restrict__ dosage)
{
	extern __shared__ double grp_p[];                 // [tile][n_cell]: the tile's normalised posteriors
	__shared__ double grp_w[HIBAG_GROUPS_TILE_MAX], grp_f[HIBAG_GROUPS_TILE_MAX];
	const int P = M.n_cell, Q = V.n_part;
	const size_t np = (size_t)B.n_pad;
	const int s0 = (int)blockIdx.x * tile;
	if (LDS) {
		if ((int)threadIdx.x < tile) {
			const int s = s0 + (int)threadIdx.x;
			const double sum_w = s < B.n_pad ? part[(size_t)P * np + s] : 0.0;
			grp_w[threadIdx.x] = sum_w;
			grp_f[threadIdx.x] = 1.0 / sum_w;
		}
		__syncthreads();
		// sample fastest: the tile's columns of a row of `part` lie side by side
		for (int i = threadIdx.x; i < tile * P; i += GROUPS_THREADS) {
			const int c = i / tile, t = i - c * tile;
			const int s = s0 + t;
			const double sum_w = grp_w[t];
			double v = 0.0;
			if (s < B.n_pad) v = sum_w != sum_w ? sum_w : normalised(part[(size_t)c * np + s], sum_w > 0, grp_f[t]);     // (NaN weight sum: poisoned batch, as k_finish_prob)
			grp_p[(size_t)t * P + c] = v;
		}
		__syncthreads();
	}
	for (int item = threadIdx.x; item < tile * Q; item += GROUPS_THREADS) {
		const int t = item / Q, q = item - t * Q;
		const int s = s0 + t;
		if (s >= B.n_samp) continue;                  // (no barrier below)
		const double sum_w = part[(size_t)P * np + s];
		const bool scale = sum_w > 0, poisoned = sum_w != sum_w;
		const double ff = 1.0 / sum_w;
		const double *__restrict__ pt = grp_p + (size_t)t * P;
		auto value = [&](int c) {
			return LDS ? pt[c] : poisoned ? sum_w : normalised(part[(size_t)c * np + s], scale, ff);
		};
		// the call: bins in bin order, each bin's cells in cell order
		{
			const uint32_t *__restrict__ list = V.call + q;
			double acc = 0.0, best = 0.0;
			int cell = -1;
#pragma unroll 8
			for (int i = 0; i < P; i++) {
				const uint32_t e = list[(size_t)i * Q];
				const int c = (int)(e & GRP_CELL);
				acc += value(c);
				const bool end = (e & GRP_END) != 0;
				const bool win = end && best < acc;
				best = win ? acc : best;
				cell = win ? c : cell;
				acc = end ? 0.0 : acc;
			}
			int a = NA_INTEGER, b = NA_INTEGER;
			double pr = poisoned ? sum_w : 0.0;
			if (cell >= 0 && !poisoned) {
				// invert p = h2 + h1*(2n-h1-1)/2 (src/LibHLA.cpp:1523), as finish_call does: any cell of the bin names its groups
				// (written out, not cell_pair: with the helper this kernel's register count and occupancy change)
				int h1 = 0, row = M.n_hla, rem = cell;
				while (rem >= row) { rem -= row; row--; h1++; }
				const int32_t *__restrict__ of = V.group_of + (size_t)q * M.n_hla;
				const int ga = of[h1], gb = of[h1 + rem];
				a = min(ga, gb); b = max(ga, gb);
				pr = best;
			}
			const size_t at = (size_t)s * Q + q;
			G1[at] = a; G2[at] = b;
			prob[at] = pr;
		}
		if (dosage) {
			const uint32_t *__restrict__ list = V.dose + q;
			double *__restrict__ out = dosage + (size_t)s * V.n_level + V.offset[q];
			const int n_group = V.offset[q + 1] - V.offset[q];
			double acc = 0.0;
			int g = 0;
#pragma unroll 8
			for (int i = 0; i < V.n_dose; i++) {
				const uint32_t e = list[(size_t)i * Q];
				double x = value((int)(e & GRP_CELL));
				x = (e & GRP_ZERO) ? 0.0 : x;
				acc += (e & GRP_TWICE) ? 2 * x : x;
				if (e & GRP_END) {
					if (g < n_group) out[g] = poisoned ? sum_w : acc;     // (the plan marks exactly n_group ends)
					g++;
					acc = 0.0;
				}
			}
		}
		if (matching && q == 0) matching[s] = matching_of(part, P, np, s);
	}
}

#endif
