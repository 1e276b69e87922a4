// hibag_knock.hip -- hibag_hip_oob_knock: the out-of-bag SNP knock-out of a bagged model (hlaSNPImportance, DESIGN.md section
// 21).  Per classifier c and SNP s of c: c, as a one-classifier model of its own, predicts its out-of-bag samples with s set
// to missing, and the calls are counted against the truth the way hlaCompareAllele counts them -- every (c, s) in ONE call
// on the model's workspace, integer tallies coming back in place of calls.
//
// The driver is predict_oob_locked's with a different pack: the cohort's byte codes are formed once, and every batch is a
// run of VIRTUAL 64-lane groups (hibag_k_knock.h) of the call's group table -- the base groups first, then per SNP in use,
// ascending, one group per block of 64 samples.  Pass 1 (with its record log) and the three pick kernels are the
// out-of-bag entry's own, unchanged.

#include "hibag_internal.h"

namespace hibag_detail {

// variants of the model: one per (classifier, position in its SNP list), in the model's own CSR order
static size_t knock_variants(const hibag_hip_model *m)
{
	size_t n = 0;
	for (const HostClassifier &k : m->cls) n += k.snpidx.size();
	return n;
}

// The inverted index SNP -> (classifier, variant) of the model on the device (HibagKnockView::user_*), users in model order:
// mask_user_index's, with the variant number of every entry beside its classifier.
static int knock_user_index(hibag_hip_model *m)
{
	if (m->knock_idx_ready) return 0;
	const int S = std::max(m->n_snp, 0);
	std::vector<int> off((size_t)S + 1, 0);
	for (const HostClassifier &k : m->cls) for (int v : k.snpidx) off[(size_t)v + 1]++;
	for (int v = 0; v < S; v++) off[(size_t)v + 1] += off[v];
	const size_t n_user = (size_t)off[S], slots = std::max<size_t>(n_user, 1);
	std::vector<int> at(off.begin(), off.end() - 1), tab((size_t)S + 1 + 2 * slots, 0);
	std::copy(off.begin(), off.end(), tab.begin());
	int var = 0;
	for (size_t c = 0; c < m->cls.size(); c++)
		for (int v : m->cls[c].snpidx) {
			const size_t u = (size_t)at[v]++;
			tab[(size_t)S + 1 + u] = (int)c;
			tab[(size_t)S + 1 + slots + u] = var++;
		}
	if (int rc = m->knock_idx.reserve(tab.size() * sizeof(int))) return rc;
	HIP_TRY(hipMemcpy(m->knock_idx.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
	m->knock_user_off = off;
	m->knock_idx_ready = true;
	return 0;
}

struct KnockOut {
	int64_t *tally;                        // [n_variant + C][5]
	int32_t *H1, *H2;                      // optional [n_variant + C][n_samp]
	double *prob;
};

// The whole call on the device: genotypes, bootstrap counts, truth and the group table up once, the cohort's codes once,
// batches of at most batch_limit lanes, the tallies (and the raw outputs asked for) down once.  The entry runs it under
// with_handover_repair, as predict_oob_locked is.
static int oob_knock_locked(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num, const int32_t *truth,
	double call_threshold, const KnockOut &out)
{
	if (int rc = oob_hap_table(m)) return rc;
	if (int rc = knock_user_index(m)) return rc;
	StagedStreams *ss;
	if (int rc = staged_streams(m, &ss)) return rc;
	const hipStream_t st = ss->run;
	const size_t C = (size_t)m->view.n_classifier, n = (size_t)n_samp, S = (size_t)m->n_snp;
	const size_t n_variant = knock_variants(m), rows = n_variant + C;
	const size_t n_blk = (n + 63) / 64, n_pad0 = n_blk * 64;

	// the group table: the base groups, then the groups of every SNP in use
	std::vector<int2> table;
	for (size_t b = 0; b < n_blk; b++) table.push_back(make_int2(-1, (int)b));
	for (size_t s = 0; s < S; s++)
		if (m->knock_user_off[s + 1] > m->knock_user_off[s])
			for (size_t b = 0; b < n_blk; b++) table.push_back(make_int2((int)s, (int)b));
	const size_t n_group = table.size();

	int lim = batch_limit(m);
	if (const char *e = getenv("HIBAG_KNOCK_BATCH")) lim = std::min(lim, std::max(64, atoi(e)) / 64 * 64);   // (diagnostic: smaller batches)
	const int force_rescan = getenv("HIBAG_OOB_RESCAN") && atoi(getenv("HIBAG_OOB_RESCAN")) != 0;           // (diagnostic, as for hibag_hip_predict_oob)
	const size_t lim_g = (size_t)lim / 64, pad_max = std::min(lim_g, n_group) * 64;

	// inputs: samp_num [C][n], truth [n][2], the table
	const size_t i_samp = 0, i_truth = i_samp + C * n * 4, i_table = (i_truth + n * 8 + 7) / 8 * 8, in_bytes = i_table + n_group * sizeof(int2);
	// a batch's picks [C][pad_max] and the base calls [C][n_pad0]
	const size_t r_h1 = 0, r_h2 = r_h1 + C * pad_max * 4, r_prob = (r_h2 + C * pad_max * 4 + 7) / 8 * 8, r_b1 = r_prob + C * pad_max * 8,
		r_b2 = r_b1 + C * n_pad0 * 4, res_bytes = r_b2 + C * n_pad0 * 4;
	// outputs: the tallies, then the raw outputs asked for
	const size_t o_tally = 0, o_prob = o_tally + rows * 5 * 8, o_h1 = o_prob + (out.prob ? rows * n * 8 : 0),
		o_h2 = o_h1 + (out.H1 ? rows * n * 4 : 0), out_bytes = o_h2 + (out.H1 ? rows * n * 4 : 0);
	if (int rc = m->ws_geno.reserve(std::max<size_t>(n * S * sizeof(int32_t), 4))) return rc;
	if (int rc = m->knock_base.reserve(std::max<size_t>(S * n_pad0, 1))) return rc;
	if (int rc = m->knock_in.reserve(in_bytes)) return rc;
	if (int rc = m->knock_res.reserve(res_bytes)) return rc;
	if (int rc = m->knock_out.reserve(out_bytes)) return rc;
	char *in = m->knock_in.as<char>(), *res = m->knock_res.as<char>(), *o = m->knock_out.as<char>();

	if (int rc = workspace_enter(m, st)) return rc;
	WorkspaceGuard guard{m, st};
	guard.enqueued = true;
	HIP_TRY(hipMemcpyAsync(m->ws_geno.p, geno, n * S * sizeof(int32_t), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(in + i_samp, samp_num, C * n * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(in + i_truth, truth, n * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(in + i_table, table.data(), n_group * sizeof(int2), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(o + o_tally, 0, rows * 5 * 8, st));
	if (out.prob) HIP_TRY(hipMemsetAsync(o + o_prob, 0, rows * n * 8, st));
	if (out.H1) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(o + o_h1), (int)0x80000000, 2 * rows * n, st));
	m->timer.begin(HIBAG_HIP_K_PACK, st);
	hibag_launch_knock_base(m->view, m->ws_geno.as<int32_t>(), n_samp, m->knock_base.as<uint8_t>(), st);
	m->timer.end(st);

	HibagKnockView K;
	K.group = (const int2 *)(in + i_table);
	K.n_cohort = n_samp; K.n_pad0 = (int)n_pad0;
	K.base = m->knock_base.as<uint8_t>();
	K.samp_num = (const int32_t *)(in + i_samp); K.truth = (const int32_t *)(in + i_truth);
	K.user_off = m->knock_idx.as<int>(); K.user_cls = K.user_off + S + 1;
	K.user_var = K.user_cls + std::max<size_t>((size_t)m->knock_user_off[S], 1);
	K.base_h1 = (int32_t *)(res + r_b1); K.base_h2 = (int32_t *)(res + r_b2);
	K.tally = (long long *)(o + o_tally);
	K.n_variant = (int)n_variant;
	K.use_threshold = std::isfinite(call_threshold) ? 1 : 0;
	K.threshold = K.use_threshold ? call_threshold : 0.0;
	K.H1 = out.H1 ? (int32_t *)(o + o_h1) : nullptr; K.H2 = out.H1 ? (int32_t *)(o + o_h2) : nullptr;
	K.prob = out.prob ? (double *)(o + o_prob) : nullptr;
	const char *d_hap = m->oob_hap.as<char>();
	for (size_t g0 = 0; g0 < n_group; g0 += lim_g) {
		const size_t ng = std::min(lim_g, n_group - g0);
		HibagBatchView B;
		if (int rc = make_batch(m, (int)(ng * 64), true, B)) return rc;
		HibagOobOut O;
		O.samp_num = nullptr;                          // (k_oob_weight's; the picks do not read it)
		O.h1 = (int32_t *)(res + r_h1); O.h2 = (int32_t *)(res + r_h2); O.prob = (double *)(res + r_prob);
		O.ld = (size_t)B.n_pad;
		O.hap_bits = (const uint64_t *)d_hap; O.hap_freq = (const double *)(d_hap + m->oob_freq_at);
		O.hap_off = (const int *)(d_hap + m->oob_off_at); O.hla_start = (const int *)(d_hap + m->oob_start_at);
		K.g0 = (int)g0;
		const int n_base = g0 < n_blk ? (int)std::min(ng, n_blk - g0) : 0;
		m->timer.begin(HIBAG_HIP_K_TOTAL, st);
		hibag_launch_knock(m->view, B, K, m->ws_codes.as<uint8_t>(), O, n_base, force_rescan, m->side, st);
		m->timer.end(st);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out.tally, o + o_tally, rows * 5 * 8, hipMemcpyDeviceToHost, st));
	if (out.prob) HIP_TRY(hipMemcpyAsync(out.prob, o + o_prob, rows * n * 8, hipMemcpyDeviceToHost, st));
	if (out.H1) {
		HIP_TRY(hipMemcpyAsync(out.H1, o + o_h1, rows * n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(out.H2, o + o_h2, rows * n * 4, hipMemcpyDeviceToHost, st));
	}
	if (int rc = guard.leave()) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
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
	const KnockOut out{tally, H1, H2, prob};
	return with_handover_repair(&m, 1, [&]() { return oob_knock_locked(m, geno, n_samp, samp_num, truth, call_threshold, out); });
}

} // extern "C"
