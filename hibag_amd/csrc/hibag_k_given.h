// hibag_k_given.h -- part of hibag_kernels.hip (included there behind hibag_k_finish.h, whose normalised() it shares):
// k_given_masks, k_finish_given and k_given_dosage, the finish of the given entries (hibag_hip_predict_given*): per sample
// the best allele pair among the cells CONSISTENT with what is already known of the sample's typing, that pair's posterior,
// the posterior mass of the consistent cells and, optionally, every allele's dosage restricted to them -- in place of the
// call / dosage / posterior-matrix finish.  24 bytes per sample leave the device (8 n_hla more with the dosages) instead of
// 8 * n_cell.
//
// The contract, p[c] the sample's normalised posterior in cell order -- the values k_finish_prob
// would write --, A and B the sample's two allele sets (bit masks over the model's alleles, bits >= n_hla ignored):
//   cell (h1 <= h2) is consistent iff (h1 in A and h2 in B) or (h1 in B and h2 in A);
//   support = the sum of p[c] over the consistent cells in increasing cell order, plain FP64 additions from +0.0 (no FMA:
//   the translation unit is built with -ffp-contract=off), one serial sum;
//   the call is the first consistent cell in cell order with best < p[c] strictly (best starts at 0: BestGuessEnsemble's rule
//   on the consistent cells), prob = p[that cell] -- the JOINT probability, not divided by support --; NA / NA with prob 0.0 if
//   there is none; a NaN cell never wins and, where consistent, makes support NaN; a NaN weight sum (a poisoned batch) gives
//   NA / NA with prob and support NaN whatever the sets;
//   dosage[h] = the sum over the consistent cells that contain h, in increasing cell order, of p[c] (2 p[c] on the diagonal
//   cell), the weight sum itself where that is NaN (as finish_dosage).
// With A and B both full this is finish_call and finish_dosage bit for bit, and support is k_finish_draw's S.
//
// Shape: lane = sample, like every finish kernel (`part` is cell-major: a wavefront's loads are coalesced, nothing crosses
// lanes, there is no LDS and no barrier).  The sum is serial in cell order, so a wavefront walks its 64 samples' cells once,
// row by row in h1 (wave-uniform), eight rows of `part` in flight.  The masks reach the walk word-major and sample-minor
// ([2 W][n_pad], k_given_masks transposes the caller's sample-major array of the batch): per row the lane loads the one word
// of A and of B that holds h1, per 32 columns the words A_w and B_w, combined into (h1 in A ? B_w : 0) | (h1 in B ? A_w : 0) --
// per cell that leaves a shift by a wave-uniform count, an and, the compare / select and the selected add.  The word index
// is wave-uniform and goes into an address, never into a private array; there is no bound on n_hla.  Slots behind n_samp hold
// empty masks: padded lanes read `part` (padded as well) and select nothing.
#ifndef HIBAG_K_GIVEN_H_
#define HIBAG_K_GIVEN_H_

// the caller's allow [n_samp][2][W] (sample-major) -> masks [2 W][n_pad]: thread = (sample, word)
__global__ __launch_bounds__(256) void k_given_masks(const uint32_t *__restrict__ allow, int n_samp, int n_pad, int W2,
	uint32_t *__restrict__ masks)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)W2 * (size_t)n_pad) return;
	const int j = (int)(i / (size_t)n_pad), s = (int)(i - (size_t)j * (size_t)n_pad);
	masks[i] = s < n_samp ? allow[(size_t)s * W2 + j] : 0u;
}

// one cell of the walk: the selected add, then BestGuessEnsemble's strict comparison on the consistent cells
__device__ __forceinline__ void given_step(double x, bool ok, int c, double &support, double &best, int &cell)
{
	support = ok ? support + x : support;
	const bool win = ok && best < x;
	best = win ? x : best;
	cell = win ? c : cell;
}

__global__ __launch_bounds__(64) void k_finish_given(HibagModelView M, HibagBatchView B, const double *__restrict__ part,
	const uint32_t *__restrict__ masks, int W, int32_t *__restrict__ H1, int32_t *__restrict__ H2, double *__restrict__ prob,
	double *__restrict__ support_out, double *__restrict__ matching)
{
	const int s = blockIdx.x * 64 + threadIdx.x;     // (< n_pad: the grid is n_pad / 64)
	const int n = M.n_hla, P = M.n_cell;
	const size_t np = (size_t)B.n_pad;
	const double sum_w = part[(size_t)P * np + s];
	const bool scale = sum_w > 0, poisoned = sum_w != sum_w;
	const double ff = 1.0 / sum_w;
	const uint32_t *__restrict__ mA = masks + s, *__restrict__ mB = masks + (size_t)W * np + s;
	double support = 0, best = 0;
	int cell = -1;
	int c = 0;                                        // the cell (h1, h1) at the start of a row
	for (int h1 = 0; h1 < n; h1++) {
		const int w1 = h1 >> 5;
		const bool inA = (mA[(size_t)w1 * np] >> (h1 & 31)) & 1u, inB = (mB[(size_t)w1 * np] >> (h1 & 31)) & 1u;
		for (int w = w1; w * 32 < n; w++) {
			const uint32_t both = (inA ? mB[(size_t)w * np] : 0u) | (inB ? mA[(size_t)w * np] : 0u);
			const int lo = max(h1, w * 32), hi = min(n, w * 32 + 32);      // the row's columns in this word
			const int c0 = c + (lo - h1);
			for (int h2 = lo; h2 < hi; h2 += 8) {
				// eight rows in flight, taken in cell order; behind the word's last column the last cell again, not selected
				double v[8];
#pragma unroll
				for (int j = 0; j < 8; j++) v[j] = part[(size_t)(c0 + min(h2 + j, hi - 1) - lo) * np + s];
#pragma unroll
				for (int j = 0; j < 8; j++) {
					const bool ok = h2 + j < hi && ((both >> ((h2 + j) & 31)) & 1u);
					given_step(poisoned ? sum_w : normalised(v[j], scale, ff), ok, c0 + (h2 + j - lo), support, best, cell);
				}
			}
		}
		c += n - h1;
	}
	if (s >= B.n_samp) return;
	if (poisoned) { cell = -1; best = sum_w; support = sum_w; }      // poisoned batch (k_scalars): NA call, NaN everywhere
	int b1 = NA_INTEGER, b2 = NA_INTEGER;
	if (cell >= 0) cell_pair(cell, n, b1, b2);
	H1[s] = b1; H2[s] = b2;
	prob[s] = (cell >= 0 || poisoned) ? best : 0.0;
	support_out[s] = support;
	if (matching) matching[s] = matching_of(part, P, np, s);
}

// The dosage: thread = (sample, allele), finish_dosage's walk -- term g of allele h is the cell (g, h) for g < h, (h, g) for
// g >= h, the diagonal twice -- with the consistency test: per 32 terms one combined word (h in B ? A_w : 0) | (h in A ? B_w : 0).
// Workgroup = 64 samples x FIN_SEG alleles.
__global__ __launch_bounds__(64 * FIN_SEG) void k_given_dosage(HibagModelView M, HibagBatchView B,
	const double *__restrict__ part, const uint32_t *__restrict__ masks, int W, double *__restrict__ dosage)
{
	const int s = blockIdx.x * 64 + (int)(threadIdx.x & 63), h = blockIdx.y * FIN_SEG + (int)(threadIdx.x >> 6);
	const int n = M.n_hla;
	if (s >= B.n_samp || h >= n) return;
	const size_t np = (size_t)B.n_pad;
	const double sum_w = part[(size_t)M.n_cell * np + s];
	const bool scale = sum_w > 0;
	const double ff = 1.0 / sum_w;
	const uint32_t *__restrict__ mA = masks + s, *__restrict__ mB = masks + (size_t)W * np + s;
	const bool inA = (mA[(size_t)(h >> 5) * np] >> (h & 31)) & 1u, inB = (mB[(size_t)(h >> 5) * np] >> (h & 31)) & 1u;
	auto cell_of = [&](int g) {
		const int h1 = g < h ? g : h, h2 = g < h ? h : g;
		return (size_t)h2 + (size_t)h1 * (2 * n - h1 - 1) / 2;
	};
	double d = 0;
	for (int w = 0; w * 32 < n; w++) {
		const uint32_t both = (inB ? mA[(size_t)w * np] : 0u) | (inA ? mB[(size_t)w * np] : 0u);
		const int hi = min(n, w * 32 + 32);
		for (int g = w * 32; g < hi; g += 8) {
			double v[8];
#pragma unroll
			for (int j = 0; j < 8; j++) v[j] = part[cell_of(min(g + j, hi - 1)) * np + s];
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const bool ok = g + j < hi && ((both >> ((g + j) & 31)) & 1u);
				const double x = normalised(v[j], scale, ff);
				d = ok ? d + (g + j == h ? 2 * x : x) : d;
			}
		}
	}
	dosage[(size_t)s * n + h] = sum_w != sum_w ? sum_w : d;      // (NaN weight sum: poisoned batch, see k_scalars)
}

#endif
