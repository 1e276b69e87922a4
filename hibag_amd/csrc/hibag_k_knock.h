// hibag_k_knock.h -- part of hibag_kernels.hip (included there, one translation unit: pass 1 and the out-of-bag picks run
// unchanged on what these kernels prepare): the out-of-bag SNP knock-out of hibag_hip_oob_knock:
// k_knock_codes, k_knock_weight, k_knock_tally.
//
// A knock-out is a VIRTUAL group of 64 lanes: 64 training samples (block `blk` of the cohort) whose byte codes are the
// cohort's own, except that the row of one SNP is 3 (missing) -- a missing SNP is marginalised exactly, it adds nothing to
// the distance and lowers the classifier weight (src/LibHLA.cpp:747-819, :2418-2431).  Only the classifiers that hold the
// SNP are asked (the others keep 64 zero weights: pass 1 skips them, the picks store NA), and of their lanes only the
// out-of-bag ones.  A group with snp = -1 is a base group: nothing knocked out, every classifier asked -- row c of
// hibag_hip_predict_oob.  The groups of a batch are entries g0 .. g0 + n_pad / 64 of the call's table.
#ifndef HIBAG_K_KNOCK_H_
#define HIBAG_K_KNOCK_H_

// k_knock_codes: the virtual batch's codes [n_snp][n_pad] from the cohort's [n_snp][n_pad0] (k_codes left 3 on the lanes
// beyond the cohort).  grid (groups, n_snp / 4), one wavefront per SNP row, lane = sample: a 64-byte read and a 64-byte
// write per wavefront.
__global__ __launch_bounds__(256) void k_knock_codes(HibagModelView M, HibagBatchView B, HibagKnockView K,
	uint8_t *__restrict__ codes)
{
	const int g = blockIdx.x, row = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (row >= M.n_snp) return;
	const int2 e = K.group[K.g0 + g];
	uint8_t v = K.base[(size_t)row * K.n_pad0 + (size_t)e.y * 64 + lane];
	if (row == e.x) v = 3;
	codes[(size_t)row * B.n_pad + (size_t)g * 64 + lane] = v;
}

// position of classifier c among the users of `snp` (ascending classifiers), -1 = c does not hold it
__device__ __forceinline__ int knock_user(const HibagKnockView &K, int snp, int c)
{
	int lo = K.user_off[snp], hi = K.user_off[snp + 1] - 1;
	while (lo <= hi) {
		const int mid = (lo + hi) >> 1, v = K.user_cls[mid];
		if (v == c) return mid;
		if (v < c) lo = mid + 1; else hi = mid - 1;
	}
	return -1;
}

// k_knock_weight (after k_pack, which left the full model's weights): grid (groups, C), thread = lane, the shape of
// k_oob_weight and its expression -- the one-classifier weight from the VIRTUAL codes, so the knocked-out SNP counts as
// missing; 0 where the sample does not exist, is in the bag of c, or c does not hold the group's SNP.
__global__ __launch_bounds__(64) void k_knock_weight(HibagModelView M, HibagBatchView B, const uint8_t *__restrict__ codes,
	HibagKnockView K)
{
	const int c = blockIdx.y, g = blockIdx.x, s = g * 64 + threadIdx.x;
	const int2 e = K.group[K.g0 + g];
	const int i = e.y * 64 + threadIdx.x;
	const size_t at = (size_t)c * B.n_pad + s;
	const bool holds = e.x < 0 || knock_user(K, e.x, c) >= 0;         // (wave-uniform)
	double w = 0.0;
	if (holds && i < K.n_cohort && K.samp_num[(size_t)c * K.n_cohort + i] == 0) {
		const int k = M.n_snp_c[c];
		const int *__restrict__ idx = M.snp_index + M.snp_off[c];
		int num = 0;
		for (int j = 0; j < k; j++) num += codes[(size_t)idx[j] * B.n_pad + s] != 3;
		w = k > 0 ? ((double)num / k) : 0.0;
	}
	B.cw[at] = w;
	B.winv[2 * at] = w;
}

// k_knock_tally (after the picks): the batch's groups [g_first, g_first + gridDim.x), lane = sample; the users of the
// group's SNP (a base group: every classifier) are walked wave-uniformly, blockIdx.y taking every gridDim.y-th.  Per
// (group, user) the five counters of hlaCompareAllele (R/DataUtilities.R:1376-1420) over the lanes that are out of bag
// for the classifier and whose true pair is known: a __ballot and a population count each, one integer atomic per
// wavefront and counter -- integer sums have no order.  A base group keeps its calls ([C][n_pad0]) for the variants to be
// compared with: base groups come first in the table and are tallied by a launch of their own, ahead of the variants'.
// The raw outputs, where asked for, get the out-of-bag lanes (the driver filled the rest with NA / 0).
__global__ __launch_bounds__(64) void k_knock_tally(HibagModelView M, HibagBatchView B, HibagKnockView K, HibagOobOut O,
	int g_first)
{
	const int NA = (int)0x80000000;
	const int g = g_first + blockIdx.x, lane = threadIdx.x;
	const int2 e = K.group[K.g0 + g];
	const bool base = e.x < 0;
	const int i = e.y * 64 + lane;
	const int u0 = base ? 0 : K.user_off[e.x], u1 = base ? M.n_classifier : K.user_off[e.x + 1];
	const bool exists = i < K.n_cohort;
	int t1 = NA, t2 = NA;
	if (exists) { t1 = K.truth[2 * (size_t)i]; t2 = K.truth[2 * (size_t)i + 1]; }
	const bool known = t1 != NA && t2 != NA;
	for (int u = u0 + (int)blockIdx.y; u < u1; u += (int)gridDim.y) {
		const int c = base ? u : K.user_cls[u];
		const size_t row = base ? (size_t)K.n_variant + c : (size_t)K.user_var[u];
		const size_t at = (size_t)c * O.ld + (size_t)g * 64 + lane;
		const int h1 = O.h1[at], h2 = O.h2[at];
		const double prob = O.prob[at];
		const bool live = exists && K.samp_num[(size_t)c * K.n_cohort + i] == 0;
		if (live && K.H1) {
			const size_t o = row * (size_t)K.n_cohort + i;
			K.H1[o] = h1; K.H2[o] = h2;
		}
		if (live && K.prob) K.prob[row * (size_t)K.n_cohort + i] = prob;
		const size_t bat = (size_t)c * K.n_pad0 + i;
		bool changed = false;
		if (base) { K.base_h1[bat] = h1; K.base_h2[bat] = h2; }
		else changed = h1 != K.base_h1[bat] || h2 != K.base_h2[bat];
		const bool counted = live && known;
		const bool called = counted && h1 != NA && h2 != NA && (!K.use_threshold || prob >= K.threshold);
		// crt.num.haplo: the first true allele takes the predicted one it equals (the first by preference), the second true
		// allele then needs the other one
		const bool a1 = t1 == h1, b1 = !a1 && t1 == h2;
		const bool second = (!a1 && t2 == h1) || (!b1 && t2 == h2);
		const bool both = (t1 == h1 && t2 == h2) || (t2 == h1 && t1 == h2);
		const unsigned long long m_ind = __ballot(counted), m_call = __ballot(called), m_both = __ballot(called && both),
			m_first = __ballot(called && (a1 || b1)), m_second = __ballot(called && second),
			m_changed = __ballot(counted && changed);
		if (lane == 0) {
			unsigned long long *t = (unsigned long long *)K.tally + 5 * row;
			if (m_ind) atomicAdd(t + 0, (unsigned long long)__popcll(m_ind));
			if (m_call) atomicAdd(t + 1, (unsigned long long)__popcll(m_call));
			if (m_both) atomicAdd(t + 2, (unsigned long long)__popcll(m_both));
			if (m_first | m_second) atomicAdd(t + 3, (unsigned long long)(__popcll(m_first) + __popcll(m_second)));
			if (m_changed) atomicAdd(t + 4, (unsigned long long)__popcll(m_changed));
		}
	}
}

#endif
