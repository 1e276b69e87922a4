// hibag_whole.hip -- the entries that take a small (training-sized) cohort through the device in ONE call: the frame they
// share (WholeCall, hibag_internal.h: stream, reserves, workspace chaining, uploads, batches, downloads, the final
// synchronisation), the diagnostic batch knobs, the model tables built at a first call (the plain haplotype table, the
// SNP-users index), and the two drivers whose kernels are the batch driver's own: hibag_hip_predict_oob and
// hibag_hip_predict_masked.  hibag_hip_oob_knock (hibag_knock.hip) and hibag_hip_predict_prefix (hibag_prefix.hip) run on
// the same frame.

#include "hibag_internal.h"

namespace hibag_detail {

// ---------------------------------------------------------------------------
// The frame

int WholeCall::open(int n_samp)
{
	StagedStreams *ss;
	if (int rc = staged_streams(m, &ss)) return rc;
	st = ss->run;
	geno_bytes = (size_t)n_samp * (size_t)m->n_snp * sizeof(int32_t);
	if (int rc = m->ws_geno.reserve(std::max<size_t>(geno_bytes, 4))) return rc;
	if (int rc = m->ws_in.reserve(std::max<size_t>(in.bytes, 8))) return rc;
	if (int rc = m->ws_out.reserve(std::max<size_t>(out.bytes, 8))) return rc;
	if (int rc = m->ws_scratch.reserve(std::max<size_t>(scratch.bytes, 8))) return rc;
	in.base = m->ws_in.as<char>(); out.base = m->ws_out.as<char>(); scratch.base = m->ws_scratch.as<char>();
	geno.d_geno = m->ws_geno.as<int32_t>();
	if (int rc = workspace_enter(m, st)) return rc;
	guard.m = m; guard.st = st; guard.enqueued = true;
	return 0;
}

int WholeCall::close(std::initializer_list<Download> downloads)
{
	HIP_TRY(hipGetLastError());
	for (const Download &d : downloads)
		if (int rc = download(d.dst, d.src, d.bytes)) return rc;
	if (int rc = guard.leave()) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

int batch_cap(const char *env_name, int lim)
{
	const char *e = getenv(env_name);
	return e ? std::max(64, std::min(lim, std::max(64, atoi(e))) / 64 * 64) : lim;
}

int oob_force_rescan()
{
	const char *e = getenv("HIBAG_OOB_RESCAN");
	return e && atoi(e) != 0;
}

// ---------------------------------------------------------------------------
// Model tables built at the first call that needs them

// The plain haplotype table of every classifier on the device (HibagOobOut): what oob_rescan walks.
int oob_hap_table(hibag_hip_model *m)
{
	if (m->oob_hap_ready) return 0;
	const int C = (int)m->cls.size(), nh = m->n_hla;
	std::vector<uint64_t> bits;
	std::vector<double> freq;
	std::vector<int> off(std::max(C, 1), 0), start((size_t)std::max(C, 1) * (nh + 1), 0);
	for (int c = 0; c < C; c++) {
		const HostClassifier &k = m->cls[c];
		off[c] = (int)freq.size();
		int *st = &start[(size_t)c * (nh + 1)];
		for (int h : k.hla) st[h + 1]++;                       // (haplotypes are grouped by allele, as the model's builder takes them)
		for (int h = 0; h < nh; h++) st[h + 1] += st[h];
		bits.insert(bits.end(), k.bits.begin(), k.bits.end());
		freq.insert(freq.end(), k.freq.begin(), k.freq.end());
	}
	if (freq.empty()) { bits.assign(2, 0); freq.assign(1, 0.0); }
	const size_t b_bits = bits.size() * sizeof(uint64_t), b_freq = freq.size() * sizeof(double), b_off = off.size() * sizeof(int);
	m->oob_freq_at = b_bits;
	m->oob_off_at = m->oob_freq_at + b_freq;
	m->oob_start_at = m->oob_off_at + b_off;
	if (int rc = m->oob_hap.reserve(m->oob_start_at + start.size() * sizeof(int))) return rc;
	char *d = m->oob_hap.as<char>();
	HIP_TRY(hipMemcpy(d, bits.data(), b_bits, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d + m->oob_freq_at, freq.data(), b_freq, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d + m->oob_off_at, off.data(), b_off, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d + m->oob_start_at, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice));
	m->oob_hap_ready = true;
	return 0;
}

void oob_hap_view(const hibag_hip_model *m, HibagOobOut &O)
{
	const char *d = m->oob_hap.as<char>();
	O.hap_bits = (const uint64_t *)d; O.hap_freq = (const double *)(d + m->oob_freq_at);
	O.hap_off = (const int *)(d + m->oob_off_at); O.hla_start = (const int *)(d + m->oob_start_at);
}

// The inverted index SNP -> (classifier, variant) of the model on the device, users in model order: [n_snp + 1] offsets,
// the users' classifiers, their variant numbers (one variant per classifier and position in its SNP list, in the model's
// own CSR order); the two lists have one spare slot in a model without users.  HibagMaskView reads the first two parts
// (k_mask_counts), HibagKnockView all three.
int snp_users_index(hibag_hip_model *m)
{
	if (m->snp_users_ready) return 0;
	const int S = std::max(m->n_snp, 0);
	std::vector<int> off((size_t)S + 1, 0);
	for (const HostClassifier &k : m->cls) for (int v : k.snpidx) off[(size_t)v + 1]++;
	for (int v = 0; v < S; v++) off[(size_t)v + 1] += off[v];
	const size_t slots = std::max<size_t>((size_t)off[S], 1);
	std::vector<int> at(off.begin(), off.end() - 1), tab((size_t)S + 1 + 2 * slots, 0);
	std::copy(off.begin(), off.end(), tab.begin());
	int var = 0;
	for (size_t c = 0; c < m->cls.size(); c++)
		for (int v : m->cls[c].snpidx) {
			const size_t u = (size_t)at[v]++;
			tab[(size_t)S + 1 + u] = (int)c;
			tab[(size_t)S + 1 + slots + u] = var++;
		}
	if (int rc = m->snp_users.reserve(tab.size() * sizeof(int))) return rc;
	HIP_TRY(hipMemcpy(m->snp_users.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
	m->snp_users_off = off;
	m->snp_users_ready = true;
	return 0;
}

// ---------------------------------------------------------------------------
// hlaOutOfBag's per-classifier predictions (hibag_hip_predict_oob)

// Genotypes and bootstrap counts up once, batches of at most batch_limit samples (pack, one-classifier weights, pass 1
// with its record log, the picks), the [C][n_samp] results down once.
static int predict_oob_locked(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num,
	int32_t *H1, int32_t *H2, double *prob)
{
	if (int rc = oob_hap_table(m)) return rc;
	const size_t C = (size_t)m->view.n_classifier, n = (size_t)n_samp;
	WholeCall F(m);
	const size_t i_samp = F.in.take(C * n * 4);
	const size_t o_h1 = F.out.take(C * n * 4), o_h2 = F.out.take(C * n * 4), o_prob = F.out.take(C * n * 8);
	if (int rc = F.open(n_samp)) return rc;
	const hipStream_t st = F.st;
	if (int rc = F.upload_geno(geno)) return rc;
	if (int rc = F.upload(F.in.at<char>(i_samp), samp_num, C * n * 4)) return rc;
	const int force_rescan = oob_force_rescan();
	HibagOobOut O;
	O.ld = n;
	oob_hap_view(m, O);
	if (int rc = F.for_each_batch(n, (size_t)batch_cap("HIBAG_OOB_BATCH", batch_limit(m)), true, [&](HibagBatchView &B, size_t s0, int) {
		O.samp_num = F.in.at<int32_t>(i_samp) + s0;
		O.h1 = F.out.at<int32_t>(o_h1) + s0; O.h2 = F.out.at<int32_t>(o_h2) + s0; O.prob = F.out.at<double>(o_prob) + s0;
		enqueue_pack(m, B, F.geno, (int)s0, st);
		m->timer.begin(HIBAG_HIP_K_TOTAL, st, true);
		hibag_launch_oob(m->view, B, m->ws_codes.as<uint8_t>(), O, force_rescan, m->side, st);
		m->timer.end(st);
		debug_stage("out-of-bag batch", st);
		return 0;
	})) return rc;
	return F.close({{H1, F.out.at<char>(o_h1), C * n * 4}, {H2, F.out.at<char>(o_h2), C * n * 4}, {prob, F.out.at<char>(o_prob), C * n * 8}});
}

// ---------------------------------------------------------------------------
// A per-sample classifier mask (hibag_hip_predict_masked)

// Genotypes and mask up once, batches of at most batch_limit samples (pack, the sub-models' weights, passes 1 and 2 or the
// vote, finish), the outputs asked for down once.
static int predict_masked_locked(hibag_hip_model *m, const int32_t *geno, int n_samp, const uint8_t *use, int vote_method,
	const PredictOut &out)
{
	if (int rc = snp_users_index(m)) return rc;
	const size_t C = (size_t)m->view.n_classifier, n = (size_t)n_samp, S = (size_t)m->n_snp, P = (size_t)m->view.n_cell,
		nh = (size_t)m->n_hla;
	const int lim = batch_cap("HIBAG_MASK_BATCH", batch_limit(m));
	WholeCall F(m);
	const size_t i_use = F.in.take(C * n);
	const size_t o_h1 = F.out.take(n * 4), o_h2 = F.out.take(n * 4), o_mp = F.out.take(n * 8), o_mt = F.out.take(n * 8),
		o_ds = F.out.take(out.dosage ? n * nh * 8 : 0), o_pp = F.out.take(out.postprob ? n * P * 8 : 0);
	// a batch's per-sample SNP counts [n_snp][n_pad]
	const size_t x_cnt = F.scratch.take(std::max<size_t>(S, 1) * (size_t)round_up(std::min(lim, n_samp), HIBAG_WAVE) * sizeof(int32_t));
	if (int rc = F.open(n_samp)) return rc;
	const hipStream_t st = F.st;
	PredictOut d;                              // the outputs asked for, on the device
	if (out.H1) { d.H1 = F.out.at<int32_t>(o_h1); d.H2 = F.out.at<int32_t>(o_h2); }
	if (out.max_prob) d.max_prob = F.out.at<double>(o_mp);
	if (out.matching) d.matching = F.out.at<double>(o_mt);
	if (out.dosage) d.dosage = F.out.at<double>(o_ds);
	if (out.postprob) d.postprob = F.out.at<double>(o_pp);
	if (int rc = F.upload_geno(geno)) return rc;
	if (int rc = F.upload(F.in.at<char>(i_use), use, C * n)) return rc;
	HibagMaskView K;
	K.ld = n;
	K.user_off = m->snp_users.as<int>(); K.user_cls = K.user_off + S + 1;
	K.cnt = F.scratch.at<int32_t>(x_cnt);
	if (int rc = F.for_each_batch(n, (size_t)lim, vote_method == 2, [&](HibagBatchView &B, size_t s0, int) {
		K.use = F.in.at<uint8_t>(i_use) + s0;
		m->timer.begin(HIBAG_HIP_K_PACK, st);
		hibag_launch_pack(m->view, B, F.geno.d_geno + s0 * S, 0, nullptr, nullptr, m->ws_codes.as<uint8_t>(), st);
		hibag_launch_mask_weights(m->view, B, m->ws_codes.as<uint8_t>(), K, st);
		m->timer.end(st);
		run_core(m, B, vote_method, m->ws_part.as<double>(), st);
		m->timer.begin(HIBAG_HIP_K_FINISH, st, true);
		const PredictOut b = d.advanced(s0, nh, P);
		hibag_launch_finish(m->view, B, B.part, b.H1, b.H2, b.max_prob, b.matching, b.dosage, b.postprob, st);
		m->timer.end(st);
		debug_stage("masked batch", st);
		return 0;
	})) return rc;
	return F.close({{out.H1, d.H1, n * 4}, {out.H2, d.H2, n * 4}, {out.max_prob, d.max_prob, n * 8}, {out.matching, d.matching, n * 8},
		{out.dosage, d.dosage, n * nh * 8}, {out.postprob, d.postprob, n * P * 8}});
}

} // namespace hibag_detail

extern "C" {

int hibag_hip_predict_oob(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num,
	int32_t *H1, int32_t *H2, double *prob)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (!m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model not finalized");
	if (n_samp < 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_samp < 0");
	if (n_samp > 0 && !geno) return hibag_fail(HIBAG_HIP_EINVAL, "geno is NULL");
	if (n_samp > 0 && !samp_num) return hibag_fail(HIBAG_HIP_EINVAL, "samp_num is NULL");
	if (n_samp > 0 && (!H1 || !H2 || !prob)) return hibag_fail(HIBAG_HIP_EINVAL, "H1, H2 and prob are all required");
	if (!m->have_snpidx)
		return hibag_fail(HIBAG_HIP_ESTATE, "model was built without SNP indices: raw genotypes cannot be packed");
	if (n_samp == 0 || m->view.n_classifier == 0) return 0;
	std::lock_guard<std::mutex> g(m->lock);
	HIP_TRY(hipSetDevice(m->device));
	return with_handover_repair(&m, 1, [&]() { return predict_oob_locked(m, geno, n_samp, samp_num, H1, H2, prob); });
}

int hibag_hip_predict_masked(hibag_hip_model *m, const int32_t *geno, int n_samp, const uint8_t *use, int vote_method,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob)
{
	if (int rc = check_predict_args(m, geno, n_samp, vote_method, H1, H2)) return rc;
	if (n_samp > 0 && !use) return hibag_fail(HIBAG_HIP_EINVAL, "use is NULL");
	if (n_samp == 0) return 0;
	std::lock_guard<std::mutex> g(m->lock);
	HIP_TRY(hipSetDevice(m->device));
	const PredictOut out{H1, H2, max_prob, matching, dosage, postprob};
	return with_handover_repair(&m, 1, [&]() { return predict_masked_locked(m, geno, n_samp, use, vote_method, out); });
}

} // extern "C"
