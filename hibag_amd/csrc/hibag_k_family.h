// hibag_k_family.h -- part of hibag_kernels.hip (included there behind hibag_k_given.h, whose given_step() and, through
// hibag_k_finish.h, normalised() it shares): k_family_ratios, k_finish_family and k_family_dosage, the finish of the family
// entries (hibag_hip_predict_family*): per sample the best allele pair under the sample's own posterior WEIGHTED with the
// Mendelian transmission probability its parents' results give each pair, that pair's weighted posterior, the weighted mass
// of all pairs and every allele's weighted dosage -- in place of the call / dosage / posterior-matrix finish.  The weight is
// built on the device from other samples' results of the same call: parents are finished before their children.
//
// The contract, p[c] the sample's normalised posterior in cell order -- the values k_finish_prob
// would write --, (father, mother) the sample's row of the call's pedigree (indices into the call, -1 = not in this call):
//   ratio vector of a parent j with joint dosage D_j and support S_j > 0:  r_j[h] = (0.5 * (D_j[h] / S_j)) / prior[h] (the
//   last division skipped without a prior); a parent -1, or one whose S_j is not > 0, is unknown: r == 1.0;
//   weight of cell (h1 <= h2):  a = rf[h1] * rm[h2], b = rf[h2] * rm[h1], w = 0.5 * (a + b), x = p * w -- plain FP64, no FMA
//   (the translation unit is built with -ffp-contract=off); both parents unknown: w == 1.0 and x == p bit for bit;
//   support = the sum of x[c] over all cells in increasing cell order from +0.0, one serial sum;
//   the call is the first cell in cell order with best < x[c] strictly (best starts at 0), prob = x[that cell] -- joint, not
//   divided by support --; NA / NA with prob 0.0 if there is none; a NaN x never wins and makes support NaN; a NaN weight sum
//   (a poisoned batch) gives NA / NA with prob and support NaN;
//   dosage[h] = the sum of x[c] over the cells that contain h in increasing cell order (2 x[c] on the diagonal cell), the
//   weight sum itself where that is NaN.  It is always formed: descendants need it.
// With both parents unknown this is finish_call and finish_dosage bit for bit, and support is k_finish_draw's S.
//
// Rounds: depth(s) = 0 without known parents, else 1 + the larger depth of its parents (the host computes it).  A batch is
// finished in one round per distinct depth in it, ascending: k_family_ratios, k_finish_family, k_family_dosage with that
// depth.  Lanes of another depth neither store nor count; a wavefront without a lane of the round's depth returns at once.
// The call-wide arrays fam_D [n_call][n_hla] and fam_S [n_call] hold every finished sample's (D, S): a parent of an earlier
// round, batch or slice is already there (the kernel stream is in order).
//
// Shape: k_finish_given's -- lane = sample, one wavefront per workgroup, a serial walk row by row in h1, eight loads of
// `part` in flight, nothing crosses lanes, no LDS, no barrier.  The ratios reach the walk allele-major and sample-minor
// ([2 n_hla][n_pad]: rf then rm), so a wavefront's loads of them are coalesced: per row the lane loads rf[h1] and rm[h1], per
// cell rf[h2] and rm[h2].  The allele index is wave-uniform and goes into an address, never into a private array; there is
// no bound on n_hla.  Slots behind n_samp and lanes of another depth hold 1.0.
#ifndef HIBAG_K_FAMILY_H_
#define HIBAG_K_FAMILY_H_

// rule 1 for the batch's samples of depth `round`: thread = (which parent, allele, slot).  ped / depth: the call's, from the
// batch's sample 0 on; fam_D / fam_S: the call's, from the call's sample 0 on (a parent index is the call's numbering).
__global__ __launch_bounds__(256) void k_family_ratios(const double *__restrict__ fam_D, const double *__restrict__ fam_S,
	const int32_t *__restrict__ ped, const int32_t *__restrict__ depth, const double *__restrict__ prior, int n_samp, int n_pad,
	int n_hla, int round, double *__restrict__ ratios)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)2 * (size_t)n_hla * (size_t)n_pad) return;
	const int j = (int)(i / (size_t)n_pad), s = (int)(i - (size_t)j * (size_t)n_pad);
	const int which = j >= n_hla ? 1 : 0, h = j - which * n_hla;
	double r = 1.0;
	if (s < n_samp && depth[s] == round) {
		const int p = ped[(size_t)2 * s + which];
		if (p >= 0) {
			const double S = fam_S[p];
			if (S > 0) {
				r = 0.5 * (fam_D[(size_t)p * n_hla + h] / S);
				if (prior) r = r / prior[h];
			}
		}
	}
	ratios[i] = r;
}

// rule 2: the weight of a cell from the four ratios, and the weighted posterior
__device__ __forceinline__ double family_weighted(double p, double rf1, double rm1, double rf2, double rm2)
{
	const double a = rf1 * rm2, b = rf2 * rm1;
	return p * (0.5 * (a + b));
}

__global__ __launch_bounds__(64) void k_finish_family(HibagModelView M, HibagBatchView B, const double *__restrict__ part,
	const double *__restrict__ ratios, const int32_t *__restrict__ depth, int round, int32_t *__restrict__ H1,
	int32_t *__restrict__ H2, double *__restrict__ prob, double *__restrict__ support_out, double *__restrict__ matching,
	double *__restrict__ fam_S)
{
	const int s = blockIdx.x * 64 + threadIdx.x;     // (< n_pad: the grid is n_pad / 64)
	const bool mine = s < B.n_samp && depth[s] == round;
	if (!__any(mine)) return;                         // (one wavefront per workgroup: wave-uniform)
	const int n = M.n_hla, P = M.n_cell;
	const size_t np = (size_t)B.n_pad;
	const double sum_w = part[(size_t)P * np + s];
	const bool scale = sum_w > 0, poisoned = sum_w != sum_w;
	const double ff = 1.0 / sum_w;
	const double *__restrict__ rf = ratios + s, *__restrict__ rm = ratios + (size_t)n * np + s;
	double support = 0, best = 0;
	int cell = -1;
	int c = 0;                                        // the cell (h1, h1) at the start of a row
	for (int h1 = 0; h1 < n; h1++) {
		const double rf1 = rf[(size_t)h1 * np], rm1 = rm[(size_t)h1 * np];
		for (int h2 = h1; h2 < n; h2 += 8) {
			// eight rows in flight, taken in cell order; behind the row's last column the last cell again, not counted
			double v[8], f[8], g[8];
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const int hh = min(h2 + j, n - 1);
				v[j] = part[(size_t)(c + hh - h1) * np + s];
				f[j] = rf[(size_t)hh * np];
				g[j] = rm[(size_t)hh * np];
			}
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const double x = family_weighted(poisoned ? sum_w : normalised(v[j], scale, ff), rf1, rm1, f[j], g[j]);
				given_step(x, h2 + j < n, c + (h2 + j - h1), support, best, cell);
			}
		}
		c += n - h1;
	}
	if (!mine) return;
	if (poisoned) { cell = -1; best = sum_w; support = sum_w; }      // poisoned batch (k_scalars): NA call, NaN everywhere
	int b1 = NA_INTEGER, b2 = NA_INTEGER;
	if (cell >= 0) cell_pair(cell, n, b1, b2);
	H1[s] = b1; H2[s] = b2;
	prob[s] = (cell >= 0 || poisoned) ? best : 0.0;
	support_out[s] = support;
	fam_S[s] = support;                               // (the batch's part of the call-wide array: what descendants divide by)
	if (matching) matching[s] = matching_of(part, P, np, s);
}

// The dosage: thread = (sample, allele), finish_dosage's walk -- term g of allele h is the cell (g, h) for g < h, (h, g) for
// g >= h, the diagonal twice -- with x[c] in place of p[c].  (a and b of rule 2 swap with the order of g and h; IEEE addition
// and multiplication are commutative, so the weight is the walk's bit for bit.)  Workgroup = 64 samples x FIN_SEG alleles.
// fam_D: the batch's part of the call-wide array; dosage: the caller's, or nullptr.
__global__ __launch_bounds__(64 * FIN_SEG) void k_family_dosage(HibagModelView M, HibagBatchView B,
	const double *__restrict__ part, const double *__restrict__ ratios, const int32_t *__restrict__ depth, int round,
	double *__restrict__ fam_D, double *__restrict__ dosage)
{
	const int s = blockIdx.x * 64 + (int)(threadIdx.x & 63), h = blockIdx.y * FIN_SEG + (int)(threadIdx.x >> 6);
	const int n = M.n_hla;
	if (s >= B.n_samp || h >= n || depth[s] != round) return;
	const size_t np = (size_t)B.n_pad;
	const double sum_w = part[(size_t)M.n_cell * np + s];
	const bool scale = sum_w > 0;
	const double ff = 1.0 / sum_w;
	const double *__restrict__ rf = ratios + s, *__restrict__ rm = ratios + (size_t)n * np + s;
	const double rfh = rf[(size_t)h * np], rmh = rm[(size_t)h * np];
	auto cell_of = [&](int g) {
		const int h1 = g < h ? g : h, h2 = g < h ? h : g;
		return (size_t)h2 + (size_t)h1 * (2 * n - h1 - 1) / 2;
	};
	double d = 0;
	for (int g = 0; g < n; g += 8) {
		double v[8], f[8], q[8];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int gg = min(g + j, n - 1);
			v[j] = part[cell_of(gg) * np + s];
			f[j] = rf[(size_t)gg * np];
			q[j] = rm[(size_t)gg * np];
		}
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const double x = family_weighted(normalised(v[j], scale, ff), rfh, rmh, f[j], q[j]);
			d = g + j < n ? d + (g + j == h ? 2 * x : x) : d;
		}
	}
	d = sum_w != sum_w ? sum_w : d;                   // (NaN weight sum: poisoned batch, see k_scalars)
	fam_D[(size_t)s * n + h] = d;
	if (dosage) dosage[(size_t)s * n + h] = d;
}

#endif
