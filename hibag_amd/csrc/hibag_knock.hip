// hibag_knock.hip -- hibag_hip_oob_knock: the out-of-bag SNP knock-out of a bagged model (hlaSNPImportance, DESIGN.md section
// 21).  Per classifier c and SNP s of c: c, as a one-classifier model of its own, predicts its out-of-bag samples with s set
// to missing, and the calls are counted against the truth the way hlaCompareAllele counts them -- every (c, s) in ONE call
// on the model's workspace, integer tallies coming back in place of calls.
//
// The driver runs on the frame of the whole-call entries (WholeCall, hibag_whole.hip), as the out-of-bag entry does, with
// a different pack: the cohort's byte codes are formed once, and every batch is a run of VIRTUAL 64-lane groups
// (hibag_k_knock.h) of the call's group table -- the base groups first, then per SNP in use, ascending, one group per block
// of 64 samples.  Pass 1 (with its record log) and the three pick kernels are the out-of-bag entry's own, unchanged.

#include "hibag_internal.h"

namespace hibag_detail {

// variants of the model: one per (classifier, position in its SNP list), in the model's own CSR order
static size_t knock_variants(const hibag_hip_model *m)
{
	size_t n = 0;
	for (const HostClassifier &k : m->cls) n += k.snpidx.size();
	return n;
}

// The whole call on the device (WholeCall): genotypes, bootstrap counts, truth and the group table up once, the cohort's
// codes once, batches of at most batch_limit lanes, the tallies [n_variant + C][5] (and the raw outputs asked for,
// [n_variant + C][n_samp] each) down once.
static int oob_knock_locked(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num, const int32_t *truth,
	double call_threshold, int64_t *tally, int32_t *H1, int32_t *H2, double *prob)
{
	if (int rc = oob_hap_table(m)) return rc;
	if (int rc = snp_users_index(m)) return rc;
	const std::vector<int> &user_off = m->snp_users_off;
	const size_t C = (size_t)m->view.n_classifier, n = (size_t)n_samp, S = (size_t)m->n_snp;
	const size_t n_variant = knock_variants(m), rows = n_variant + C;
	const size_t n_blk = (n + 63) / 64, n_pad0 = n_blk * 64;

	// the group table: the base groups, then the groups of every SNP in use
	std::vector<int2> table;
	for (size_t b = 0; b < n_blk; b++) table.push_back(make_int2(-1, (int)b));
	for (size_t s = 0; s < S; s++)
		if (user_off[s + 1] > user_off[s])
			for (size_t b = 0; b < n_blk; b++) table.push_back(make_int2((int)s, (int)b));
	const size_t n_lane = table.size() * 64;

	// a batch is whole groups: the cap counts their lanes
	const size_t lim = (size_t)batch_cap("HIBAG_KNOCK_BATCH", batch_limit(m)), pad_max = std::min(lim, n_lane);
	WholeCall F(m);
	const size_t i_samp = F.in.take(C * n * 4), i_truth = F.in.take(n * 8), i_table = F.in.take(table.size() * sizeof(int2));
	// the cohort's codes [S][n_pad0], a batch's picks [C][pad_max] and the base calls [C][n_pad0]
	const size_t x_base = F.scratch.take(S * n_pad0), x_h1 = F.scratch.take(C * pad_max * 4), x_h2 = F.scratch.take(C * pad_max * 4),
		x_prob = F.scratch.take(C * pad_max * 8), x_b1 = F.scratch.take(C * n_pad0 * 4), x_b2 = F.scratch.take(C * n_pad0 * 4);
	// the tallies, then the raw outputs asked for (both call matrices in one block [2][rows][n]: one fill covers them)
	const size_t o_tally = F.out.take(rows * 5 * 8), o_prob = F.out.take(prob ? rows * n * 8 : 0),
		o_call = F.out.take(H1 ? 2 * rows * n * 4 : 0);
	if (int rc = F.open(n_samp)) return rc;
	const hipStream_t st = F.st;

	HibagKnockView K;
	K.group = F.in.at<int2>(i_table);
	K.n_cohort = n_samp; K.n_pad0 = (int)n_pad0;
	K.base = F.scratch.at<uint8_t>(x_base);
	K.samp_num = F.in.at<int32_t>(i_samp); K.truth = F.in.at<int32_t>(i_truth);
	K.user_off = m->snp_users.as<int>(); K.user_cls = K.user_off + S + 1;
	K.user_var = K.user_cls + std::max<size_t>((size_t)user_off[S], 1);
	K.base_h1 = F.scratch.at<int32_t>(x_b1); K.base_h2 = F.scratch.at<int32_t>(x_b2);
	K.tally = F.out.at<long long>(o_tally);
	K.n_variant = (int)n_variant;
	K.use_threshold = std::isfinite(call_threshold) ? 1 : 0;
	K.threshold = K.use_threshold ? call_threshold : 0.0;
	K.H1 = H1 ? F.out.at<int32_t>(o_call) : nullptr; K.H2 = H1 ? K.H1 + rows * n : nullptr;
	K.prob = prob ? F.out.at<double>(o_prob) : nullptr;

	if (int rc = F.upload_geno(geno)) return rc;
	if (int rc = F.upload(F.in.at<char>(i_samp), samp_num, C * n * 4)) return rc;
	if (int rc = F.upload(F.in.at<char>(i_truth), truth, n * 8)) return rc;
	if (int rc = F.upload(F.in.at<char>(i_table), table.data(), table.size() * sizeof(int2))) return rc;
	HIP_TRY(hipMemsetAsync(K.tally, 0, rows * 5 * 8, st));
	if (K.prob) HIP_TRY(hipMemsetAsync(K.prob, 0, rows * n * 8, st));
	if (K.H1) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)K.H1, (int)0x80000000, 2 * rows * n, st));
	m->timer.begin(HIBAG_HIP_K_PACK, st);
	hibag_launch_knock_base(m->view, F.geno.d_geno, n_samp, F.scratch.at<uint8_t>(x_base), st);
	m->timer.end(st);

	const int force_rescan = oob_force_rescan();
	HibagOobOut O;
	O.samp_num = nullptr;                          // (k_oob_weight's; the picks do not read it)
	O.h1 = F.scratch.at<int32_t>(x_h1); O.h2 = F.scratch.at<int32_t>(x_h2); O.prob = F.scratch.at<double>(x_prob);
	oob_hap_view(m, O);
	if (int rc = F.for_each_batch(n_lane, lim, true, [&](HibagBatchView &B, size_t lane0, int n_lanes) {
		const size_t g0 = lane0 / 64, ng = (size_t)n_lanes / 64;
		O.ld = (size_t)B.n_pad;
		K.g0 = (int)g0;
		const int n_base = g0 < n_blk ? (int)std::min(ng, n_blk - g0) : 0;
		m->timer.begin(HIBAG_HIP_K_TOTAL, st);
		hibag_launch_knock(m->view, B, K, m->ws_codes.as<uint8_t>(), O, n_base, force_rescan, m->side, st);
		m->timer.end(st);
		return 0;
	})) return rc;
	return F.close({{tally, K.tally, rows * 5 * 8}, {prob, K.prob, rows * n * 8}, {H1, K.H1, rows * n * 4}, {H2, K.H2, rows * n * 4}});
}

} // namespace hibag_detail

extern "C" {

static int knock_check_model(const hibag_hip_model *m)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (!m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model not finalized");
	if (!m->have_snpidx)
		return hibag_fail(HIBAG_HIP_ESTATE, "model was built without SNP indices: raw genotypes cannot be packed");
	return 0;
}

int hibag_hip_oob_knock_variants(const hibag_hip_model *m, int *n_variant)
{
	if (int rc = knock_check_model(m)) return rc;
	if (!n_variant) return hibag_fail(HIBAG_HIP_EINVAL, "n_variant is NULL");
	const size_t n = knock_variants(m);
	if (n > 0x7FFFFFFFu) return hibag_fail(HIBAG_HIP_EINVAL, "the model has more than 2^31 - 1 (classifier, SNP) pairs");
	*n_variant = (int)n;
	return 0;
}

int hibag_hip_oob_knock(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num, const int32_t *truth,
	double call_threshold, int64_t *tally, int32_t *H1, int32_t *H2, double *prob)
{
	if (int rc = knock_check_model(m)) return rc;
	if (n_samp < 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_samp < 0");
	if (n_samp > 0 && !geno) return hibag_fail(HIBAG_HIP_EINVAL, "geno is NULL");
	if (n_samp > 0 && !samp_num) return hibag_fail(HIBAG_HIP_EINVAL, "samp_num is NULL");
	if (n_samp > 0 && !truth) return hibag_fail(HIBAG_HIP_EINVAL, "truth is NULL");
	if (!tally) return hibag_fail(HIBAG_HIP_EINVAL, "tally is NULL");
	if ((H1 == nullptr) != (H2 == nullptr)) return hibag_fail(HIBAG_HIP_EINVAL, "H1 and H2 must be given together");
	const size_t rows = knock_variants(m) + m->cls.size();
	if (rows > 0x7FFFFFFFu) return hibag_fail(HIBAG_HIP_EINVAL, "the model has more than 2^31 - 1 (classifier, SNP) pairs");
	if (n_samp == 0 || m->view.n_classifier == 0 || m->n_snp == 0) {
		// nothing is out of bag of nothing: every tally is 0 (and there are no raw rows to fill but the all-NA ones)
		memset(tally, 0, rows * 5 * sizeof(int64_t));
		const size_t cells = rows * (size_t)n_samp;
		for (size_t i = 0; i < cells; i++) { if (H1) { H1[i] = H2[i] = (int32_t)0x80000000; } if (prob) prob[i] = 0.0; }
		return 0;
	}
	std::lock_guard<std::mutex> g(m->lock);
	HIP_TRY(hipSetDevice(m->device));
	return with_handover_repair(&m, 1, [&]() { return oob_knock_locked(m, geno, n_samp, samp_num, truth, call_threshold, tally, H1, H2, prob); });
}

} // extern "C"
