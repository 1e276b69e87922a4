// hibag_k_oob.h -- part of hibag_kernels.hip (included there, one translation unit: the walks are templates that inline into
// their kernels): hlaOutOfBag's per-classifier predictions (R/HIBAG.R:1320-1334): k_oob_weight, k_oob_pick, k_oob_scan,
// k_oob_best_valu.  Classifier c, taken as a one-classifier model of its own, predicts every sample its bootstrap did not
// draw (samp_num[c][s] == 0).
//
// A one-classifier model's SNP weights are all 1 (_GetSNPWeights, src/LibHLA.cpp:2484-2496), so the classifier weight is
// w = (SNPs with a genotype in 0..2) / n_snp_c (src/LibHLA.cpp:2418-2431).  Averaging over one classifier turns the
// normalised posterior p = cell * (1/total) into
//     T(p) = (0 + p * w) * (1 / w)       (AddProbToSum, NormalizeSumPostProb: src/LibHLA.cpp:1497-1518)
// and the call is the first strict maximum of T(p) in pair order, from 0 (:2370 -> :1549-1566); T(p) of the winner is
// the probability returned.  T is monotone but not the identity: cells that p separates by an ulp may tie under T,
// and then the earlier one wins.
#ifndef HIBAG_K_OOB_H_
#define HIBAG_K_OOB_H_

__device__ __forceinline__ double oob_value(double cell, double inv, double w)
{
	return (0.0 + (cell * inv) * w) * (1.0 / w);
}

// One (classifier, sample) result: cell index p (-1 = no call) -> H1, H2 (0-based, NA_integer_) and the probability.
__device__ __forceinline__ void oob_store(const HibagModelView &M, const HibagOobOut &O, int c, int s, int p, double prob)
{
	int h1 = (int)0x80000000, h2 = (int)0x80000000;
	if (p >= 0) {
		h1 = 0;
		int rest = p;
		while (rest >= M.n_hla - h1) { rest -= M.n_hla - h1; h1++; }
		h2 = h1 + rest;
	} else prob = 0.0;
	const size_t at = (size_t)c * O.ld + s;
	O.h1[at] = h1; O.h2[at] = h2; O.prob[at] = prob;
}

// k_oob_weight (after k_pack, which left the full model's weights): the one-classifier weight of every OOB sample, 0 for
// the in-bag ones and for the padding.  grid (n_pad / 64, C), thread = sample.
__global__ __launch_bounds__(64) void k_oob_weight(HibagModelView M, HibagBatchView B, const uint8_t *__restrict__ codes,
	HibagOobOut O)
{
	const int c = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	const size_t at = (size_t)c * B.n_pad + s;
	double w = 0.0;
	if (s < B.n_samp && O.samp_num[(size_t)c * O.ld + s] == 0) {
		const int k = M.n_snp_c[c];
		const int *__restrict__ idx = M.snp_index + M.snp_off[c];
		int num = 0;
		for (int j = 0; j < k; j++) num += codes[(size_t)idx[j] * B.n_pad + s] != 3;
		w = k > 0 ? ((double)num / k) : 0.0;
	}
	B.cw[at] = w;
	B.winv[2 * at] = w;
}

// The reference's own walk over one classifier for one lane (_PostProb2's loop nest, src/LibHLA.cpp:1776-1821): every
// cell summed in order from the plain haplotype table, then the first strict maximum of T.  Only where the record log
// cannot settle the call (k_oob_pick): it costs a full pair walk per lane.
__device__ __noinline__ int oob_rescan(const HibagModelView &M, const HibagOobOut &O, const uint8_t *__restrict__ codes,
	int n_pad, int c, int s, double inv, double w, double *prob)
{
	const int k = M.n_snp_c[c];
	const int *__restrict__ idx = M.snp_index + M.snp_off[c];
	uint64_t s1[2] = {0, 0}, s2[2] = {~0ull, ~0ull};          // TGenotype::IntToSNP, src/LibHLA.cpp:662-706
	for (int j = 0; j < k; j++) {
		const uint32_t g = codes[(size_t)idx[j] * n_pad + s];
		const uint64_t bit = 1ull << (j & 63);
		if (g == 0) s2[j >> 6] &= ~bit;
		else if (g == 1) { s1[j >> 6] |= bit; s2[j >> 6] &= ~bit; }
		else if (g == 2) s1[j >> 6] |= bit;
	}
	const int nw = k <= 64 ? 1 : 2;
	auto hamm = [&](const uint64_t *a, const uint64_t *b) {  // src/LibHLA.cpp:747-819
		int d = 0;
		for (int q = 0; q < nw; q++) {
			const uint64_t miss = s2[q] & ~s1[q];
			const uint64_t mask = ((a[q] ^ s2[q]) | (b[q] ^ s1[q])) & ~miss;
			d += __popcll((a[q] ^ s1[q]) & mask) + __popcll((b[q] ^ s2[q]) & mask);
		}
		return d;
	};
	const int *__restrict__ st = O.hla_start + (size_t)c * (M.n_hla + 1);
	const uint64_t *__restrict__ bits = O.hap_bits + 2 * (size_t)O.hap_off[c];
	const double *__restrict__ freq = O.hap_freq + O.hap_off[c];
	double best = 0;
	int bp = -1, p = 0;
	for (int h1 = 0; h1 < M.n_hla; h1++) {
		const int a0 = st[h1], a1 = st[h1 + 1];
		for (int h2 = h1; h2 < M.n_hla; h2++, p++) {
			double cell = 0;
			if (h1 == h2) {
				for (int a = a0; a < a1; a++) {
					cell += (freq[a] * freq[a]) * M.tab[hamm(bits + 2 * a, bits + 2 * a)];
					const double ff = 2 * freq[a];
					for (int b = a + 1; b < a1; b++) cell += (ff * freq[b]) * M.tab[hamm(bits + 2 * a, bits + 2 * b)];
				}
			} else {
				const int b0 = st[h2], b1 = st[h2 + 1];
				for (int a = a0; a < a1; a++) {
					const double ff = 2 * freq[a];
					for (int b = b0; b < b1; b++) cell += (ff * freq[b]) * M.tab[hamm(bits + 2 * a, bits + 2 * b)];
				}
			}
			const double v = oob_value(cell, inv, w);
			if (best < v) { best = v; bp = p; }
		}
	}
	*prob = best;
	return bp;
}

// k_oob_pick: the matrix-engine classifiers of one K step, from the records pass 1 logged (HibagBatchView::vrec; k_vote_pick).
// T is monotone, so the cells whose T equals the last record's form a suffix of the records, and the earliest of them wins.
// The log holds the first record and the latest six: where all six qualify, the first does not and there were records in
// between, the earliest may be one the log lost -- that lane walks the classifier again (oob_rescan).  `force_rescan`
// (diagnostic): every lane walks.  thread = (sample, classifier).
__global__ __launch_bounds__(64) void k_oob_pick(HibagModelView M, HibagBatchView B, const uint8_t *__restrict__ codes,
	HibagOobOut O, int force_rescan)
{
	const int c = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	if (M.engine[c] == HIBAG_ENGINE_VALU || M.n_step[c] > 1) return;      // k_oob_best_valu / k_oob_scan
	if (s >= B.n_samp) return;
	const size_t at = (size_t)c * B.n_pad + s;
	const double w = B.cw[at];
	int pos = -1, cell = -1;                              // winner: position in the classifier's cell list, or cell index
	double prob = 0;
	if (w > 0) {
		const uint4 *__restrict__ rec = B.vrec + (size_t)c * 8 * B.n_pad + s;
		const uint4 h = rec[0];
		const double vmax = __hiloint2double((int)h.y, (int)h.x), inv = B.inv[at];
		const int n = (int)h.z;
		if (n > 0 && inv == inv) {
			const uint4 f = rec[(size_t)B.n_pad];
			const double fq = oob_value(__hiloint2double((int)f.y, (int)f.x), inv, w);
			if (!(fabs(inv) <= 1.79769313486231570815e+308)) {       // every positive cell is +inf: the first one wins
				pos = (int)f.z;
				prob = fq;
			} else if (force_rescan) {
				cell = oob_rescan(M, O, codes, B.n_pad, c, s, inv, w, &prob);
			} else {
				const double qm = oob_value(vmax, inv, w);
				int best = 0x7FFFFFFF, nq = 0;
				if (fq == qm) best = (int)f.z;
				const int nr = min(n - 1, 6);             // ring entries that belong to this batch: slots 2 .. 1 + nr
				for (int j = 0; j < nr; j++) {
					const uint4 r = rec[(size_t)(2 + j) * B.n_pad];
					if (oob_value(__hiloint2double((int)r.y, (int)r.x), inv, w) == qm) { best = min(best, (int)r.z); nq++; }
				}
				if (fq != qm && n - 1 > 6 && nq == 6) cell = oob_rescan(M, O, codes, B.n_pad, c, s, inv, w, &prob);
				else if (qm > 0) { pos = best; prob = qm; }       // (the last record itself always qualifies)
			}
		}
	}
	if (pos >= 0) cell = (int)M.cls_cell[M.cls_off[c] + pos];
	oob_store(M, O, c, s, cell, prob);
}

// k_oob_scan: the FP4 classifiers of several K steps, whose cell sums pass 1 stores one and all (k_vote_scan): the
// reference's scan over the stored sums, with T.  thread = sample.
__global__ __launch_bounds__(64) void k_oob_scan(HibagModelView M, HibagBatchView B, HibagOobOut O)
{
	const int c = M.wide_cls[blockIdx.y], s = blockIdx.x * 64 + threadIdx.x;
	const size_t at = (size_t)c * B.n_pad + s;
	const double w = B.cw[at];
	const bool active = w > 0;
	if (__ballot(active) == 0) {                                          // (pass 1 skipped the classifier: its rows are stale)
		if (s < B.n_samp) oob_store(M, O, c, s, -1, 0.0);
		return;
	}
	const double *__restrict__ rows = cell_rows(M, B, c, s >> 6) + (s & 63);
	const double inv = B.inv[at];
	const int n = M.cls_n[c];
	double best = 0;
	int bi = -1, i = 0;
	for (; i + 16 <= n; i += 16) {
		double v[16];
#pragma unroll
		for (int j = 0; j < 16; j++) v[j] = rows[(size_t)(i + j) * HIBAG_WAVE];
#pragma unroll
		for (int j = 0; j < 16; j++) { const double q = oob_value(v[j], inv, w); if (best < q) { best = q; bi = i + j; } }
	}
	for (; i < n; i++) { const double q = oob_value(rows[(size_t)i * HIBAG_WAVE], inv, w); if (best < q) { best = q; bi = i; } }
	if (s < B.n_samp) oob_store(M, O, c, s, active && bi >= 0 ? (int)M.cls_cell[M.cls_off[c] + bi] : -1, best);
}

// k_oob_best_valu: the classifiers of the VALU engine (more than 112 SNPs) -- their pairs walked a second time, with 1/total
// in hand (classifier_best, with T).  grid (group quads, classifiers).
template <int NWP>
__device__ __forceinline__ int classifier_best_oob(const HibagModelView &M, const HibagBatchView &B,
	int c, int s, double inv, double w, const double *tab_s, double *prob)
{
	LaneMask<NWP> L;
	load_masks<NWP>(B, M.mask_row[c], s, L);
	const uint32_t *__restrict__ cnt = M.cls_cnt + M.cls_off[c];
	const uint32_t *__restrict__ cell_p = M.cls_cell + M.cls_off[c];
	const uint32_t *__restrict__ cp = M.stream + M.stream_off[c];
	const int ncell = M.cls_n[c];
	double best = 0;
	int best_p = -1;
	for (int i = 0; i < ncell; i++) {
		const double q = oob_value(cell_sum<NWP>(cnt[i], cp, L, tab_s), inv, w);
		if (best < q) { best = q; best_p = (int)cell_p[i]; }
	}
	*prob = best;
	return best_p;
}

__global__ __launch_bounds__(BLOCK_THREADS) void k_oob_best_valu(HibagModelView M, HibagBatchView B, HibagOobOut O)
{
	__shared__ double tab_s[HIBAG_TAB_N];
	const int c = M.c_order[blockIdx.y];
	if (M.engine[c] != HIBAG_ENGINE_VALU) return;
	stage_table(M, tab_s);
	const int group = blockIdx.x * BLOCK_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (group * HIBAG_WAVE >= B.n_pad) return;
	const int s = group * HIBAG_WAVE + (threadIdx.x & 63);
	const size_t at = (size_t)c * B.n_pad + s;
	const double w = B.cw[at];
	const bool active = w > 0;
	if (__ballot(active) == 0) {
		if (s < B.n_samp) oob_store(M, O, c, s, -1, 0.0);
		return;
	}
	const double inv = B.inv[at];
	double prob = 0;
	int bp;
#define CALL(N) bp = classifier_best_oob<N>(M, B, c, s, inv, w, tab_s, &prob)
	HIBAG_DISPATCH_NWP(M.nwp[c], CALL)
#undef CALL
	if (s < B.n_samp) oob_store(M, O, c, s, active ? bp : -1, prob);
}

#endif
