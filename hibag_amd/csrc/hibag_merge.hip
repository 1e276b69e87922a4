// hibag_merge.hip -- host side of hlaPredictMerge: the merge of k models' posteriors (hlaPredMerge, R/HIBAG.R:825-1023) as a
// device operation, and the driver that runs the k predictions and the merge behind them without the posteriors leaving
// the device.  Kernels and the order of the arithmetic: hibag_k_merge.h.
//
//   hibag_hip_merge_plan_new     the maps source cell -> merged row of the k models, inverted into gather lists, on the device
//   hibag_hip_merge_device       the merge of k sample-major posterior matrices already on the device (enqueue only)
//   hibag_hip_predict_merge[_bed]  cohort up, per chunk of samples: k x (pack, pass 1, pass 2) + the merge on one stream,
//                                the requested outputs down.  The merge reads each model's un-normalised ensemble sums
//                                (its workspace's `part`, cell-major) and normalises on the fly: the k posterior matrices
//                                are never written (DESIGN.md section 11 has the measurement behind that choice).

#include "hibag_internal.h"
#include "hibag_k_merge.h"

struct hibag_hip_merge_plan {
	int device = 0;
	int n_models = 0, n_hla = 0, n_row = 0;
	std::vector<int> n_cell;
	DevBuf d_off, d_ent;                       // the gather lists
	DevBuf acc, total, out, dosage, geno, idx, bed;     // scratch (grow-only)
	hipStream_t st = nullptr;                  // the host-pointer entries' stream
	std::mutex lock;

	~hibag_hip_merge_plan()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamDestroy(st);
		for (DevBuf *b : {&d_off, &d_ent, &acc, &total, &out, &dosage, &geno, &idx, &bed}) b->release();
	}
};

namespace hibag_detail {

// Samples per chunk: the merged matrix [n_row][n_pad] (the only buffer of the merge that grows with rows x samples: the
// models' posteriors are read from their own workspaces) stays within HIBAG_HIP_MERGE_BUDGET_BYTES, and a chunk is one
// batch of every model.  HIBAG_MERGE_CHUNK (samples, rounded down to 64) asks for smaller chunks (tests of the chunking).
static int merge_chunk(const hibag_hip_merge_plan *q, hibag_hip_model *const *models)
{
	long long lim = (long long)(HIBAG_HIP_MERGE_BUDGET_BYTES / (sizeof(double) * (size_t)std::max(q->n_row, 1)));
	for (int i = 0; models && i < q->n_models; i++) lim = std::min<long long>(lim, batch_limit(models[i]));
	lim = std::min<long long>(lim, 1 << 17);
	if (const char *e = getenv("HIBAG_MERGE_CHUNK")) lim = std::min<long long>(lim, std::max(64, atoi(e)));
	return (int)std::max<long long>(64, lim / 64 * 64);
}

// The merge of one chunk: n samples, sources as S says, outputs in device memory (any may be null; the matrices of a merge
// are row-major, dosage [n_hla][ld] and postprob [n_row][ld], here with this chunk's sample 0 at column 0 -- so
// PredictOut::advanced(s0, 1, 1) is the set s0 samples on).
static int merge_enqueue(hibag_hip_merge_plan *q, const HibagMergeSrc &S, bool part, int n, const PredictOut &d, size_t ld, hipStream_t st)
{
	const int n_pad = round_up(n, 64);
	if (int rc = q->acc.reserve((size_t)q->n_row * n_pad * sizeof(double))) return rc;
	if (int rc = q->total.reserve((size_t)n_pad * sizeof(double))) return rc;
	HibagMergePlanView Q{q->d_off.as<int>(), q->d_ent.as<uint32_t>(), q->n_hla, q->n_row};
	double *acc = q->acc.as<double>(), *total = q->total.as<double>();
	const dim3 g_rows(n_pad / 64, (q->n_row + MRG_ROWS - 1) / MRG_ROWS);
	if (part) hipLaunchKernelGGL(k_merge_rows<true>, g_rows, dim3(64 * MRG_ROW_WAVES), 0, st, Q, S, n, n_pad, acc, d.matching);
	else hipLaunchKernelGGL(k_merge_rows<false>, g_rows, dim3(64 * MRG_ROW_WAVES), 0, st, Q, S, n, n_pad, acc, d.matching);
	hipLaunchKernelGGL(k_merge_total, dim3(n_pad / 64), dim3(64), 0, st, q->n_row, n_pad, (const double *)acc, total);
	hipLaunchKernelGGL(k_merge_call, dim3(n_pad / 64), dim3(64 * MRG_SEG), 0, st, q->n_hla, q->n_row, n, n_pad, acc,
		(const double *)total, d.H1, d.H2, d.max_prob);
	if (d.dosage)
		hipLaunchKernelGGL(k_merge_dosage, dim3(n_pad / 64, (q->n_hla + MRG_SEG - 1) / MRG_SEG), dim3(64 * MRG_SEG), 0, st,
			q->n_hla, n, n_pad, (const double *)acc, d.dosage, ld);
	HIP_TRY(hipGetLastError());
	if (d.postprob)
		HIP_TRY(hipMemcpy2DAsync(d.postprob, ld * sizeof(double), acc, (size_t)n_pad * sizeof(double), (size_t)n * sizeof(double),
			(size_t)q->n_row, hipMemcpyDeviceToDevice, st));
	return 0;
}

static int check_plan_call(const hibag_hip_merge_plan *q, const double *weight, const PredictOut &out)
{
	if (!q) return hibag_fail(HIBAG_HIP_EINVAL, "merge plan is NULL");
	if (!weight) return hibag_fail(HIBAG_HIP_EINVAL, "weight is NULL");
	for (int i = 0; i < q->n_models; i++)
		if (!(weight[i] >= 0)) return hibag_fail(HIBAG_HIP_EINVAL, "weight[%d] is negative or NaN", i);
	if ((out.H1 == nullptr) != (out.H2 == nullptr)) return hibag_fail(HIBAG_HIP_EINVAL, "H1 and H2 must be given together");
	return 0;
}

// Where the cohort of hibag_hip_predict_merge comes from.
struct MergeCohort {
	const int32_t *geno = nullptr;             // host matrix ...
	int snp_major = 0;                         // ... [n_geno_snp][ld] if set, else [n_samp][n_geno_snp]
	size_t ld = 0;
	int n_geno_snp = 0;
	const char *bed_fn = nullptr;              // or a PLINK BED file of n_bed_snp SNPs (n_samp = its samples)
	int n_bed_snp = 0;
};

static int predict_merge_locked(hibag_hip_merge_plan *q, hibag_hip_model *const *models, const MergeCohort &co, int n_samp,
	const int32_t *const *snp_col, const int32_t *const *flip, int vote_method, const double *weight, int use_matching,
	const PredictOut &out)
{
	const int k = q->n_models;
	hipStream_t st = q->st;
	// per model: column (or BED row) of each of its SNPs in the cohort, and the flips
	std::vector<size_t> idx_at(k);
	std::vector<int32_t> idx;
	BedImage img;
	try {
		std::vector<int32_t> want;
		for (int i = 0; i < k; i++) {
			idx_at[i] = idx.size();
			const int S = models[i]->n_snp;
			for (int j = 0; j < S; j++) idx.push_back(snp_col && snp_col[i] ? snp_col[i][j] : j);
			for (int j = 0; j < S; j++) idx.push_back(flip && flip[i] ? (flip[i][j] != 0) : 0);
			idx.push_back(0);                  // (never an empty upload)
		}
		for (int i = 0; i < k; i++)
			for (int j = 0; j < models[i]->n_snp; j++) {
				int32_t &c = idx[idx_at[i] + j];
				if (c < 0) c = -1;
				if (c >= (co.bed_fn ? co.n_bed_snp : co.n_geno_snp))
					return hibag_fail(HIBAG_HIP_EINVAL, "snp_col[%d][%d] = %d outside the %d SNPs of the cohort", i, j, c,
						co.bed_fn ? co.n_bed_snp : co.n_geno_snp);
			}
		if (co.bed_fn) {
			// one image of the file for the SNPs of all k models
			for (int i = 0; i < k; i++) want.insert(want.end(), idx.begin() + idx_at[i], idx.begin() + idx_at[i] + models[i]->n_snp);
			if (int rc = load_bed(co.bed_fn, n_samp, co.n_bed_snp, want.data(), (int)want.size(), img)) return rc;
			size_t at = 0;
			for (int i = 0; i < k; i++)
				for (int j = 0; j < models[i]->n_snp; j++) idx[idx_at[i] + j] = img.index[at++];
		}
	} catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
	if (int rc = q->idx.reserve(idx.size() * sizeof(int32_t))) return rc;
	HIP_TRY(hipMemcpyAsync(q->idx.p, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
	// the cohort, whole
	if (co.bed_fn) {
		if (int rc = q->bed.reserve(std::max<size_t>(img.rows.size(), 1))) return rc;
		HIP_TRY(hipMemcpyAsync(q->bed.p, img.rows.data(), img.rows.size(), hipMemcpyHostToDevice, st));
	} else {
		const size_t rows = co.snp_major ? (size_t)co.n_geno_snp : (size_t)n_samp, w = co.snp_major ? (size_t)n_samp : (size_t)co.n_geno_snp;
		if (int rc = q->geno.reserve(std::max<size_t>(rows * w, 1) * sizeof(int32_t))) return rc;
		if (!co.snp_major || co.ld == w) HIP_TRY(hipMemcpyAsync(q->geno.p, co.geno, rows * w * sizeof(int32_t), hipMemcpyHostToDevice, st));
		else HIP_TRY(hipMemcpy2DAsync(q->geno.p, w * sizeof(int32_t), co.geno, co.ld * sizeof(int32_t), w * sizeof(int32_t), rows, hipMemcpyHostToDevice, st));
	}
	HIP_TRY(hipStreamSynchronize(st));          // (`idx` and `img` are pageable host memory of this frame)

	const int chunk = merge_chunk(q, models);
	const size_t cpad = (size_t)round_up(std::min(chunk, n_samp), 64), nh = (size_t)q->n_hla;
	// device outputs of a chunk: H1, H2 (int32), prob, matching -- 24 bytes per sample -- and the dosage matrix
	if (int rc = q->out.reserve(cpad * 24)) return rc;
	if (out.dosage) if (int rc = q->dosage.reserve(nh * cpad * sizeof(double))) return rc;
	PredictOut d;                              // a chunk's outputs on the device: what is asked for (the posterior is the merge's own q->acc)
	if (out.H1) { d.H1 = q->out.as<int32_t>(); d.H2 = d.H1 + cpad; }
	if (out.max_prob) d.max_prob = (double *)(q->out.as<int32_t>() + 2 * cpad);
	if (out.matching) d.matching = (double *)(q->out.as<int32_t>() + 2 * cpad) + cpad;
	if (out.dosage) d.dosage = q->dosage.as<double>();
	// one guard per model: whatever way the call ends, work it has enqueued on a model's shared workspace is chained in front
	// of that model's next call on another stream
	WorkspaceGuard guard[HIBAG_MERGE_MAX_MODELS];
	for (int i = 0; i < k; i++) {
		if (int rc = workspace_enter(models[i], st)) return rc;
		guard[i].m = models[i]; guard[i].st = st;
	}

	PackSource cohort;
	if (co.bed_fn) { cohort.d_bed = q->bed.as<uint8_t>(); cohort.mode = img.mode; cohort.stride = img.stride; }
	else {
		cohort.d_geno = q->geno.as<int32_t>();
		if (co.snp_major) cohort.ld = (size_t)n_samp;
		else cohort.row_len = co.n_geno_snp;
	}
	for (int s0 = 0; s0 < n_samp; s0 += chunk) {
		const int n = std::min(chunk, n_samp - s0), n_pad = round_up(n, 64);
		HibagMergeSrc S{};
		S.n_models = k;
		S.use_matching = use_matching != 0;
		for (int i = 0; i < k; i++) {
			hibag_hip_model *m = models[i];
			HibagBatchView B;
			if (int rc = make_batch(m, n, vote_method == 2, B)) return rc;
			guard[i].enqueued = true;
			PackSource src = cohort;               // the cohort as this model reads it: its own SNP map
			src.d_col = src.d_row = q->idx.as<int32_t>() + idx_at[i];
			src.d_flip = src.d_col + m->n_snp;
			enqueue_pack(m, B, src, s0, st);
			run_core(m, B, vote_method, m->ws_part.as<double>(), st);
			S.src[i] = m->ws_part.as<double>();
			S.n_cell[i] = m->view.n_cell;
			S.w[i] = weight[i];
		}
		if (int rc = merge_enqueue(q, S, true, n, d, (size_t)n_pad, st)) return rc;
		// down: only what was asked for (the matrices are [row][n_samp] on the host, [row][n_pad] here)
		const PredictOut h = out.advanced((size_t)s0, 1, 1);
		if (h.H1) {
			HIP_TRY(hipMemcpyAsync(h.H1, d.H1, (size_t)n * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(h.H2, d.H2, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		}
		if (h.max_prob) HIP_TRY(hipMemcpyAsync(h.max_prob, d.max_prob, (size_t)n * 8, hipMemcpyDeviceToHost, st));
		if (h.matching) HIP_TRY(hipMemcpyAsync(h.matching, d.matching, (size_t)n * 8, hipMemcpyDeviceToHost, st));
		if (h.dosage)
			HIP_TRY(hipMemcpy2DAsync(h.dosage, (size_t)n_samp * 8, d.dosage, (size_t)n_pad * 8, (size_t)n * 8, nh, hipMemcpyDeviceToHost, st));
		if (h.postprob)
			HIP_TRY(hipMemcpy2DAsync(h.postprob, (size_t)n_samp * 8, q->acc.p, (size_t)n_pad * 8, (size_t)n * 8, (size_t)q->n_row,
				hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	for (int i = 0; i < k; i++) guard[i].left = true;      // (the stream has run dry: nothing is left to chain behind)
	return 0;
}

static int predict_merge(hibag_hip_merge_plan *q, hibag_hip_model *const *models, const MergeCohort &co, int n_samp,
	const int32_t *const *snp_col, const int32_t *const *flip, int vote_method, const double *weight, int use_matching,
	const PredictOut &out)
{
	if (int rc = check_plan_call(q, weight, out)) return rc;
	if (!models) return hibag_fail(HIBAG_HIP_EINVAL, "models is NULL");
	const void *src = co.bed_fn ? (const void *)co.bed_fn : (const void *)co.geno;
	for (int i = 0; i < q->n_models; i++) {
		if (int rc = check_predict_args(models[i], src, n_samp, vote_method, out.H1, out.H2)) return rc;
		if (models[i]->view.n_cell != q->n_cell[i])
			return hibag_fail(HIBAG_HIP_EINVAL, "model %d has %d allele pairs, the merge plan was made for %d", i, models[i]->view.n_cell, q->n_cell[i]);
		if (models[i]->device != q->device)
			return hibag_fail(HIBAG_HIP_EINVAL, "model %d is on device %d, the merge plan on device %d: the models of one merge share a device", i,
				models[i]->device, q->device);
		for (int j = 0; j < i; j++)
			if (models[j] == models[i])
				return hibag_fail(HIBAG_HIP_EINVAL, "models %d and %d are the same handle: each model has one workspace (hibag_hip_model_replicate makes another)", j, i);
	}
	if (!co.bed_fn) {
		if (co.n_geno_snp <= 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_geno_snp must be positive");
		if (co.snp_major && co.ld < (size_t)n_samp) return hibag_fail(HIBAG_HIP_EINVAL, "ld = %zu is smaller than n_samp = %d", co.ld, n_samp);
		for (int i = 0; i < q->n_models; i++)
			if (!(snp_col && snp_col[i]) && models[i]->n_snp > co.n_geno_snp)
				return hibag_fail(HIBAG_HIP_EINVAL, "snp_col[%d] is NULL but the cohort has %d SNPs for the model's %d", i, co.n_geno_snp, models[i]->n_snp);
	}
	if (n_samp == 0) return 0;
	std::lock_guard<std::mutex> g(q->lock);
	// the models' locks in address order (two merges over the same models in another order must not wait for each other)
	std::vector<hibag_hip_model *> order(models, models + q->n_models);
	std::sort(order.begin(), order.end());
	for (hibag_hip_model *m : order) m->lock.lock();
	struct Unlock { std::vector<hibag_hip_model *> &v; ~Unlock() { for (hibag_hip_model *m : v) m->lock.unlock(); } } unlock{order};
	HIP_TRY(hipSetDevice(q->device));
	if (!q->st) HIP_TRY(hipStreamCreateWithFlags(&q->st, hipStreamNonBlocking));
	// (a model's outputs poisoned by a failed hand-over: repaired as in predict_staged_locked, for all the models at once)
	return with_handover_repair(models, q->n_models, [&]() {
		return predict_merge_locked(q, models, co, n_samp, snp_col, flip, vote_method, weight, use_matching, out);
	});
}

} // namespace hibag_detail

extern "C" {

hibag_hip_merge_plan *hibag_hip_merge_plan_new(int n_models, const int32_t *n_src_cell, const int32_t *const *row_of_cell,
	int n_merged_hla, int device)
{
	if (n_models < 1 || n_models > HIBAG_MERGE_MAX_MODELS) {
		hibag_fail(HIBAG_HIP_EINVAL, "a merge takes 1 to %d models, not %d", HIBAG_MERGE_MAX_MODELS, n_models);
		return nullptr;
	}
	if (!n_src_cell || !row_of_cell || n_merged_hla < 1 || n_merged_hla > 5000) {
		hibag_fail(HIBAG_HIP_EINVAL, "bad merge plan (n_merged_hla = %d)", n_merged_hla);
		return nullptr;
	}
	if (device < 0 || device >= hibag_hip_device_count()) {
		hibag_fail(HIBAG_HIP_ENODEV, "no HIP device %d", device);
		return nullptr;
	}
	const int n_row = n_merged_hla * (n_merged_hla + 1) / 2;
	hibag_hip_merge_plan *q = nullptr;
	try {
		q = new hibag_hip_merge_plan;
		q->device = device; q->n_models = n_models; q->n_hla = n_merged_hla; q->n_row = n_row;
		// counting sort of (model, cell) by merged row: model order, then ascending cell, inside every row
		std::vector<int> off(n_row + 1, 0);
		for (int i = 0; i < n_models; i++) {
			if (n_src_cell[i] < 1 || n_src_cell[i] >= (1 << 24) || !row_of_cell[i]) {
				hibag_fail(HIBAG_HIP_EINVAL, "model %d of the merge plan has %d allele pairs", i, n_src_cell[i]);
				delete q;
				return nullptr;
			}
			q->n_cell.push_back(n_src_cell[i]);
			for (int j = 0; j < n_src_cell[i]; j++) {
				const int r = row_of_cell[i][j];
				if (r < 0 || r >= n_row) {
					hibag_fail(HIBAG_HIP_EINVAL, "row_of_cell[%d][%d] = %d outside the %d merged rows", i, j, r, n_row);
					delete q;
					return nullptr;
				}
				off[r + 1]++;
			}
		}
		for (int r = 0; r < n_row; r++) off[r + 1] += off[r];
		std::vector<uint32_t> ent((size_t)std::max(off[n_row], 1));
		std::vector<int> at(off.begin(), off.end() - 1);
		for (int i = 0; i < n_models; i++)
			for (int j = 0; j < n_src_cell[i]; j++) ent[at[row_of_cell[i][j]]++] = (uint32_t)i << 24 | (uint32_t)j;
		auto up = [&]() -> int {
			HIP_TRY(hipSetDevice(device));
			if (int rc = q->d_off.reserve(off.size() * sizeof(int))) return rc;
			if (int rc = q->d_ent.reserve(ent.size() * sizeof(uint32_t))) return rc;
			HIP_TRY(hipMemcpy(q->d_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
			HIP_TRY(hipMemcpy(q->d_ent.p, ent.data(), ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
			return 0;
		};
		if (up()) { delete q; return nullptr; }
	} catch (...) {
		delete q;
		hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
		return nullptr;
	}
	return q;
}

void hibag_hip_merge_plan_free(hibag_hip_merge_plan *q) { delete q; }

int hibag_hip_merge_device(hibag_hip_merge_plan *q, const double *const *d_postprob, const double *const *d_matching,
	const double *weight, int use_matching, int n_samp, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_matching_out,
	double *d_dosage, double *d_postprob_out, size_t ld_out, void *stream)
{
	const PredictOut out{d_H1, d_H2, d_prob, d_matching_out, d_dosage, d_postprob_out};
	if (int rc = check_plan_call(q, weight, out)) return rc;
	if (!d_postprob || !d_matching) return hibag_fail(HIBAG_HIP_EINVAL, "d_postprob / d_matching is NULL");
	for (int i = 0; i < q->n_models; i++)
		if (!d_postprob[i] || !d_matching[i]) return hibag_fail(HIBAG_HIP_EINVAL, "d_postprob[%d] / d_matching[%d] is NULL", i, i);
	if (n_samp < 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_samp < 0");
	if ((d_dosage || d_postprob_out) && ld_out < (size_t)n_samp) return hibag_fail(HIBAG_HIP_EINVAL, "ld_out = %zu is smaller than n_samp = %d", ld_out, n_samp);
	if (n_samp == 0) return 0;
	std::lock_guard<std::mutex> g(q->lock);
	HIP_TRY(hipSetDevice(q->device));
	const int chunk = merge_chunk(q, nullptr);
	for (int s0 = 0; s0 < n_samp; s0 += chunk) {
		const int n = std::min(chunk, n_samp - s0);
		HibagMergeSrc S{};
		S.n_models = q->n_models;
		S.use_matching = use_matching != 0;
		for (int i = 0; i < q->n_models; i++) {
			S.src[i] = d_postprob[i] + (size_t)s0 * q->n_cell[i];
			S.mt[i] = d_matching[i] + s0;
			S.n_cell[i] = q->n_cell[i];
			S.w[i] = weight[i];
		}
		if (int rc = merge_enqueue(q, S, false, n, out.advanced((size_t)s0, 1, 1), ld_out, (hipStream_t)stream)) return rc;
	}
	return 0;
}

int hibag_hip_predict_merge(hibag_hip_merge_plan *q, hibag_hip_model *const *models, const int32_t *geno, int snp_major, size_t ld,
	int n_samp, int n_geno_snp, const int32_t *const *snp_col, const int32_t *const *flip, int vote_method,
	const double *weight, int use_matching, int32_t *H1, int32_t *H2, double *prob, double *matching, double *dosage,
	double *postprob)
{
	MergeCohort co;
	co.geno = geno; co.snp_major = snp_major; co.ld = ld; co.n_geno_snp = n_geno_snp;
	return predict_merge(q, models, co, n_samp, snp_col, flip, vote_method, weight, use_matching, {H1, H2, prob, matching, dosage, postprob});
}

int hibag_hip_predict_merge_bed(hibag_hip_merge_plan *q, hibag_hip_model *const *models, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *const *snp_col, const int32_t *const *flip, int vote_method, const double *weight, int use_matching,
	int32_t *H1, int32_t *H2, double *prob, double *matching, double *dosage, double *postprob)
{
	if (!bed_fn) return hibag_fail(HIBAG_HIP_EINVAL, "bed file name is NULL");
	if (!snp_col) return hibag_fail(HIBAG_HIP_EINVAL, "snp_col is NULL");
	for (int i = 0; q && i < q->n_models; i++) if (!snp_col[i]) return hibag_fail(HIBAG_HIP_EINVAL, "snp_col[%d] is NULL", i);
	MergeCohort co;
	co.bed_fn = bed_fn; co.n_bed_snp = n_snp;
	return predict_merge(q, models, co, n_samp, snp_col, flip, vote_method, weight, use_matching, {H1, H2, prob, matching, dosage, postprob});
}

} // extern "C"
