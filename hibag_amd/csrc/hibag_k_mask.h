// hibag_k_mask.h -- part of hibag_kernels.hip (included there, one translation unit): the per-sample classifier mask of
// hibag_hip_predict_masked: k_mask_counts, k_mask_weight.  Sample s is typed by the sub-model of the classifiers c with
// use[c][s] != 0 (hlaSubModelObj-style: the kept classifiers in model order), so what differs from the model's own step is
// the weights alone -- the cell sums, their in-order total and 1/total depend on the classifier and the sample only
// (DESIGN.md section 12).  The two kernels run between k_pack (which left the full model's weights) and pass 1, and
// overwrite B.cw / B.winv[2 at] the way k_oob_weight does:
//     cnt[snp][s] = the number of classifiers the sample uses that hold the SNP     (_GetSNPWeights of the sub-model,
//                                                                                    src/LibHLA.cpp:2484-2496)
//     cw[c][s]    = (double)num / den, the int sums of cnt over c's typed / all SNPs (src/LibHLA.cpp:2418-2431; k_pack's
//                   own expression), 0 where the sample does not use c, on the padding lanes, or where den == 0.
// A (64-sample group, classifier) pair nobody uses has cw == 0 on all 64 lanes: pass 1 skips it, pass 2 and the vote pass
// over its stale rows, as for a group whose samples miss every SNP of the classifier.  No cross-lane step anywhere.
#ifndef HIBAG_K_MASK_H_
#define HIBAG_K_MASK_H_

// k_mask_counts: grid (n_pad / 64, n_snp), lane = sample, one SNP per blockIdx.y.  The SNP's users -- the inverted index
// SNP -> classifiers in CSR form (HibagMaskView: user_off[n_snp + 1], user_cls[user_off[n_snp]]) -- are walked in model order; each
// step is one coalesced 64-byte read of a mask row.  One int32 store per (SNP, sample): no read-modify-write, nothing to
// zero first (the padding lanes store 0).
__global__ __launch_bounds__(64) void k_mask_counts(HibagModelView M, HibagBatchView B, HibagMaskView K)
{
	const int snp = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	const int u0 = K.user_off[snp], u1 = K.user_off[snp + 1];
	int n = 0;
	if (s < B.n_samp)
		for (int u = u0; u < u1; u++) n += K.use[(size_t)K.user_cls[u] * K.ld + s] != 0;
	K.cnt[(size_t)snp * B.n_pad + s] = n;
}

// k_mask_weight: grid (n_pad / 64, C), thread = sample (the shape of k_oob_weight).  `codes`: the byte codes k_codes left.
__global__ __launch_bounds__(64) void k_mask_weight(HibagModelView M, HibagBatchView B, const uint8_t *__restrict__ codes,
	HibagMaskView K)
{
	const int c = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	const size_t at = (size_t)c * B.n_pad + s;
	double w = 0.0;
	if (s < B.n_samp && K.use[(size_t)c * K.ld + s] != 0) {
		const int k = M.n_snp_c[c];
		const int *__restrict__ idx = M.snp_index + M.snp_off[c];
		int num = 0, den = 0;
		for (int j = 0; j < k; j++) {
			const size_t row = (size_t)idx[j] * B.n_pad + s;
			const int wt = K.cnt[row];
			den += wt;
			if (codes[row] != 3) num += wt;
		}
		w = den > 0 ? ((double)num / den) : 0.0;
	}
	B.cw[at] = w;
	B.winv[2 * at] = w;
}

#endif
