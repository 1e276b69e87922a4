// hibag_k_topk.h -- part of hibag_kernels.hip (included there behind hibag_k_finish.h, whose normalised() it shares):
// k_finish_topk, the finish of the top-k entries (hibag_hip_predict_topk*): per sample the k largest cells of the
// NORMALISED ensemble matrix -- the values k_finish_prob would write -- as allele pairs with their probabilities, in
// place of the call / dosage / posterior-matrix finish.  k * 20 + 8 bytes per sample leave the device instead of 8 * n_cell.
//
// The ranking rule (the contract):
//   rank 0 is BestGuessEnsemble's cell (src/LibHLA.cpp:1549-1566): the first strict maximum in cell order, only values > 0;
//   rank r is the first strict maximum in cell order among the cells not yet listed, again only values > 0
//   -- i.e. descending value, equal values in ascending cell order; cells that are 0, negative or NaN are never listed
//   (every comparison below is a strict `a < x`, false for NaN, and the list starts as zeros);
//   ranks without a cell: h1 = h2 = NA_INTEGER, prob = 0; a poisoned batch (sum_w NaN, see finish_call): NA and NaN in every rank.
//
// Shape: lane = sample, like every finish kernel (`part` is cell-major: a wavefront's loads are coalesced, nothing crosses
// lanes).  A workgroup is 64 samples x NSEG segments of the cell range; every thread scans its segment in cell order, eight
// rows in flight, and keeps its KMAX best (value, cell) sorted in registers -- the insertion is unrolled over the list with
// selects, so no index into the list is ever a run-time value and the list never leaves the registers (no private segment).
// The segments' lists go through LDS and are merged by segment 0 in segment order, each in rank order, with the same
// strict comparison: an equal value from a later cell lands behind, which reproduces the sequential scan exactly.
// KMAX is the compile-time bound (4, 8, 16; the launcher takes the smallest that holds the call's k), NSEG = 64 / KMAX:
// 16 / 8 / 4 segments, so that the lists in LDS are NSEG * KMAX * 64 * 12 bytes = 48 KB whatever KMAX is (FIN_SEG = 16
// segments of 16 candidates would be 192 KB, over a workgroup's 160).
#ifndef HIBAG_K_TOPK_H_
#define HIBAG_K_TOPK_H_

// (val, idx) sorted by descending value, equal values in the order they came; x joins behind every value >= x
template <int KMAX>
__device__ __forceinline__ void topk_insert(double (&val)[KMAX], int (&idx)[KMAX], double x, int c)
{
#pragma unroll
	for (int j = KMAX - 1; j >= 1; j--) {
		// (val[j - 1] and val[j] are still what they were: the steps before this one wrote val[j + 1 ..] only)
		const bool down = val[j - 1] < x;              // the entry above moves down one place
		const bool here = !down && val[j] < x;         // x's own place: val[j - 1] >= x > val[j]
		val[j] = down ? val[j - 1] : here ? x : val[j];
		idx[j] = down ? idx[j - 1] : here ? c : idx[j];
	}
	const bool top = val[0] < x;
	val[0] = top ? x : val[0];
	idx[0] = top ? c : idx[0];
}

template <int KMAX>
__global__ __launch_bounds__(64 * (64 / KMAX)) void k_finish_topk(HibagModelView M, HibagBatchView B,
	const double *__restrict__ part, int k, int32_t *__restrict__ H1, int32_t *__restrict__ H2,
	double *__restrict__ prob, double *__restrict__ matching)
{
	constexpr int NSEG = 64 / KMAX;
	static_assert(KMAX >= 1 && NSEG >= 1 && NSEG * KMAX == 64, "KMAX must divide 64");
	__shared__ double val_s[NSEG][KMAX][64];
	__shared__ int idx_s[NSEG][KMAX][64];
	const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
	const int s = blockIdx.x * 64 + lane;
	const int P = M.n_cell;
	const size_t np = (size_t)B.n_pad;
	const double sum_w = part[(size_t)P * np + s];
	const bool scale = sum_w > 0;
	const double ff = 1.0 / sum_w;
	const int per = (P + NSEG - 1) / NSEG;
	const int lo = min(P, seg * per), hi = min(P, lo + per);
	double val[KMAX];
	int idx[KMAX];
#pragma unroll
	for (int j = 0; j < KMAX; j++) { val[j] = 0; idx[j] = -1; }
	int p = lo;
	for (; p + 8 <= hi; p += 8) {                 // eight rows in flight, taken in cell order
		double v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = part[(size_t)(p + j) * np + s];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const double x = normalised(v[j], scale, ff);
			if (val[KMAX - 1] < x) topk_insert<KMAX>(val, idx, x, p + j);     // (most cells do not make the list)
		}
	}
	for (; p < hi; p++) {
		const double x = normalised(part[(size_t)p * np + s], scale, ff);
		if (val[KMAX - 1] < x) topk_insert<KMAX>(val, idx, x, p);
	}
	if (seg != 0) {
#pragma unroll
		for (int j = 0; j < KMAX; j++) { val_s[seg][j][lane] = val[j]; idx_s[seg][j][lane] = idx[j]; }
	}
	__syncthreads();
	if (seg != 0 || s >= B.n_samp) return;
	for (int g = 1; g < NSEG; g++)
		for (int r = 0; r < KMAX; r++) {
			const double x = val_s[g][r][lane];
			if (!(val[KMAX - 1] < x)) break;          // (the segment's list is descending: nothing behind this one gets in either)
			topk_insert<KMAX>(val, idx, x, idx_s[g][r][lane]);
		}
	const bool poisoned = sum_w != sum_w;             // (k_scalars: a batch whose hand-overs failed) NA pairs, NaN probabilities
	const size_t at = (size_t)s * (size_t)k;
#pragma unroll
	for (int r = 0; r < KMAX; r++) {
		if (r >= k) break;
		const int cell = poisoned ? -1 : idx[r];
		int b1 = NA_INTEGER, b2 = NA_INTEGER;
		if (cell >= 0) cell_pair(cell, M.n_hla, b1, b2);
		H1[at + r] = b1; H2[at + r] = b2;
		prob[at + r] = poisoned ? sum_w : val[r];     // (a rank without a cell still holds the list's initial 0)
	}
	if (matching) matching[s] = matching_of(part, P, np, s);
}

#endif
