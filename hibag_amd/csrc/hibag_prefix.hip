// hibag_prefix.hip -- host side of hibag_hip_predict_prefix: what hibag_hip_predict (vote by probability) returns for
// the model made of the first sizes[i] classifiers (hlaSubModelObj, R/HIBAG.R:1121-1129), for every i, from one pack
// and one pass 1 over all classifiers.  Kernels and the order they keep: hibag_k_prefix.h.
//
// The entry needs every classifier's cell sums kept by pass 1 (store mode 1, k_accum_cells' layout).  A model finalized
// that way is used as it is; for any other the entry builds, at its first call, a SECOND layout of the same classifiers
// with FinalizeOptions::STREAM -- a model object of its own with its own workspace, owned by the handle and freed with
// it -- so that nothing the model's other entries read or launch changes.
//
// The sub-models' classifier weights are stored, not formed on the fly: sum(sizes) rows of n_pad doubles per batch
// (k_prefix_weights), counted in the entry's own batch size.  Formed inside k_prefix_accum they would cost every
// (tile, size) wavefront the integer sums over the classifier's SNPs again -- n_tile times the work for rows that are
// read n_tile times from L2 instead.

#include "hibag_internal.h"
#include "hibag_k_prefix.h"

namespace hibag_detail {

// The layout the entry runs on: the model itself where pass 1 stores every cell sum, its second layout otherwise.
static int prefix_layout(hibag_hip_model *m, hibag_hip_model **out)
{
	if (m->store_mode == 1) { *out = m; return 0; }
	if (!m->prefix_layout) {
		hibag_hip_model *L = new (std::nothrow) hibag_hip_model;
		if (!L) return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
		try {
			L->device = m->device;
			L->n_hla = m->n_hla; L->n_snp = m->n_snp;
			L->have_snpidx = m->have_snpidx; L->use_mfma = m->use_mfma; L->use_fp4 = m->use_fp4;
			L->cls = m->cls;
			memcpy(L->tab, m->tab, sizeof(L->tab));
		} catch (...) { delete L; return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
		if (int rc = finalize_model_stream(L)) { delete L; return rc; }
		if (L->store_mode != 1) { delete L; return hibag_fail(HIBAG_HIP_ESTATE, "the second layout does not store every cell sum"); }
		m->prefix_layout = L;
	}
	*out = m->prefix_layout;
	return 0;
}

// Samples per batch of the entry: the layout's own limit, lowered so that the sub-models' weights and the tiles' maxima
// (8 bytes per size and classifier of it, 12 per size and tile) stay within 8 GB; HIBAG_PREFIX_BATCH (diagnostic) lowers it further.
static int prefix_batch(const hibag_hip_model *L, int64_t sum_sizes, int n_sizes)
{
	const double per_sample = 8.0 * (double)sum_sizes + 12.0 * (double)n_sizes * std::max(L->view.n_tile, 1);
	const int lim = std::min<double>(batch_limit(L), 8e9 / per_sample);
	return batch_cap("HIBAG_PREFIX_BATCH", std::max(64, lim / 64 * 64));
}

// The event pairs around every batch's k_prefix_accum on `st`.  The holder destroys them, and a run that fails on the way
// still waits for the stream first.
namespace {
struct EventPairs {
	hipStream_t st = nullptr;
	std::vector<hipEvent_t> ev;
	bool waited = false;                   // the stream has been synchronised behind the last record
	int add(hipEvent_t &a, hipEvent_t &b)
	{
		for (hipEvent_t *e : {&a, &b}) { HIP_TRY(hipEventCreate(e)); ev.push_back(*e); }
		return 0;
	}
	double ms() const
	{
		double sum = 0;
		for (size_t i = 0; i + 1 < ev.size(); i += 2) {
			float t = 0;
			if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) sum += t;
		}
		return sum;
	}
	~EventPairs()
	{
		if (!waited && st) (void)hipStreamSynchronize(st);
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
	}
};
} // namespace

// The whole call on the workspace of the layout L (WholeCall); the classifiers' SNP lists are read from the model itself.
static int predict_prefix_locked(hibag_hip_model *m, hibag_hip_model *L, const int32_t *geno, int n_samp, const int32_t *sizes, int n_sizes,
	int32_t *H1, int32_t *H2, double *prob, double *matching)
{
	const int C = L->view.n_classifier, S = L->n_snp, n_tile = L->view.n_tile;
	const size_t n = (size_t)n_samp, K = (size_t)n_sizes;

	// the sub-models' tables: sizes, first weight row, SNP counts (a prefix count over the classifiers' SNP lists)
	std::vector<int32_t> tab(2 * K + K * (size_t)std::max(S, 1), 0);
	int64_t sum_sizes = 0;
	{
		std::vector<int32_t> cnt(std::max(S, 1), 0);
		int c = 0;
		for (size_t i = 0; i < K; i++) {
			tab[i] = sizes[i];
			tab[K + i] = (int32_t)sum_sizes;
			sum_sizes += sizes[i];
			for (; c < sizes[i]; c++)
				for (int v : m->cls[c].snpidx) cnt[v]++;
			memcpy(&tab[2 * K + i * (size_t)S], cnt.data(), sizeof(int32_t) * (size_t)S);
		}
	}
	if (sum_sizes >= (int64_t)1 << 31) return hibag_fail(HIBAG_HIP_EINVAL, "sizes: too many classifiers in all");
	const int lim = prefix_batch(L, sum_sizes, n_sizes);
	const size_t pad_max = (size_t)round_up(std::min(lim, n_samp), HIBAG_WAVE);
	WholeCall F(L);
	EventPairs pairs;
	const size_t i_tab = F.in.take(tab.size() * sizeof(int32_t));
	// a batch's sub-model weights [sum of sizes][n_pad] and tile maxima with their cells [n_sizes][n_tile][n_pad]
	const size_t x_cw = F.scratch.take((size_t)sum_sizes * pad_max * sizeof(double)), x_best = F.scratch.take(K * n_tile * pad_max * sizeof(double)),
		x_cell = F.scratch.take(K * n_tile * pad_max * sizeof(int));
	const size_t o_h1 = F.out.take(K * n * 4), o_h2 = F.out.take(K * n * 4), o_prob = F.out.take(K * n * 8), o_mt = F.out.take(K * n * 8);
	if (int rc = F.open(n_samp)) return rc;
	const hipStream_t st = pairs.st = F.st;
	if (int rc = F.upload(F.in.at<char>(i_tab), tab.data(), tab.size() * sizeof(int32_t))) return rc;
	if (int rc = F.upload_geno(geno)) return rc;

	HibagPrefixView Q;
	Q.n_sizes = n_sizes;
	Q.sizes = F.in.at<int>(i_tab); Q.row0 = Q.sizes + K; Q.snp_weight = Q.sizes + 2 * K;
	Q.cw = F.scratch.at<double>(x_cw); Q.pbest = F.scratch.at<double>(x_best); Q.pcell = F.scratch.at<int>(x_cell);
	Q.ld = n;
	if (int rc = F.for_each_batch(n, (size_t)lim, false, [&](HibagBatchView &B, size_t s0, int) {
		Q.h1 = F.out.at<int32_t>(o_h1) + s0; Q.h2 = F.out.at<int32_t>(o_h2) + s0;
		Q.prob = F.out.at<double>(o_prob) + s0; Q.matching = F.out.at<double>(o_mt) + s0;
		enqueue_pack(L, B, F.geno, (int)s0, st);
		L->timer.begin(HIBAG_HIP_K_TOTAL, st, true);
		hibag_launch_total(L->view, B, st, L->side, false);
		L->timer.end(st);
		const unsigned n_group = (unsigned)(B.n_pad / HIBAG_WAVE);
		hipLaunchKernelGGL(k_prefix_weights, dim3(n_group, C), dim3(64), 0, st, L->view, B, Q, (const uint8_t *)L->ws_codes.as<uint8_t>());
		hipEvent_t a, b;
		if (int rc = pairs.add(a, b)) return rc;
		(void)hipEventRecord(a, st);
		const unsigned n_sq = (unsigned)((n_sizes + PREFIX_WAVES - 1) / PREFIX_WAVES);
		hipLaunchKernelGGL(k_prefix_accum, dim3(8u * ((n_group + 7) / 8) * (unsigned)n_tile * n_sq), dim3(PREFIX_WAVES * HIBAG_WAVE), 0, st, L->view, B, Q);
		(void)hipEventRecord(b, st);
		hipLaunchKernelGGL(k_prefix_finish, dim3(n_group, n_sizes), dim3(64), 0, st, L->view, B, Q);
		return 0;
	})) return rc;
	if (int rc = F.close({{H1, F.out.at<char>(o_h1), K * n * 4}, {H2, F.out.at<char>(o_h2), K * n * 4}, {prob, F.out.at<char>(o_prob), K * n * 8},
		{matching, F.out.at<char>(o_mt), K * n * 8}})) return rc;
	pairs.waited = true;
	m->pfx_accum_ms = pairs.ms();              // (only a completed run sets it; a repair's second run sets it again)
	return 0;
}

} // namespace hibag_detail

extern "C" {

int hibag_hip_predict_prefix(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *sizes, int n_sizes,
	int32_t *H1, int32_t *H2, double *prob, double *matching)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (!m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model not finalized");
	if (n_samp < 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_samp < 0");
	if (n_samp > 0 && !geno) return hibag_fail(HIBAG_HIP_EINVAL, "geno is NULL");
	if (!sizes || n_sizes < 1) return hibag_fail(HIBAG_HIP_EINVAL, "sizes is empty");
	const int C = (int)m->cls.size();
	for (int i = 0; i < n_sizes; i++) {
		if (sizes[i] < 1 || sizes[i] > C)
			return hibag_fail(HIBAG_HIP_EINVAL, "sizes[%d] = %d is outside 1 .. %d (the model's classifiers)", i, sizes[i], C);
		if (i > 0 && sizes[i] <= sizes[i - 1])
			return hibag_fail(HIBAG_HIP_EINVAL, "sizes must be strictly ascending (sizes[%d] = %d follows %d)", i, sizes[i], sizes[i - 1]);
	}
	if (n_samp > 0 && (!H1 || !H2 || !prob || !matching)) return hibag_fail(HIBAG_HIP_EINVAL, "H1, H2, prob and matching are all required");
	if (!m->have_snpidx)
		return hibag_fail(HIBAG_HIP_ESTATE, "model was built without SNP indices: raw genotypes cannot be packed");
	if (!m->snp_weight_override.empty())
		return hibag_fail(HIBAG_HIP_EINVAL, "the model carries another model's SNP counts (a classifier shard): its sub-models are not defined");
	if (n_samp == 0) return 0;
	std::lock_guard<std::mutex> g(m->lock);
	HIP_TRY(hipSetDevice(m->device));
	hibag_hip_model *L = nullptr;
	if (int rc = prefix_layout(m, &L)) return rc;
	// (a failed hand-over is repaired as in predict_staged_locked; the hand-overs are those of the layout the entry runs on)
	return with_handover_repair(&L, 1, [&]() { return predict_prefix_locked(m, L, geno, n_samp, sizes, n_sizes, H1, H2, prob, matching); });
}

int hibag_hip_predict_prefix_ms(const hibag_hip_model *m, double *accum_ms)
{
	if (!m || !accum_ms) return hibag_fail(HIBAG_HIP_EINVAL, "NULL argument");
	*accum_ms = m->pfx_accum_ms;
	return 0;
}

} // extern "C"
