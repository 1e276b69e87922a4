// hibag_assoc.hip -- host side of hlaAssocTest (R/Association.R): the handle behind `hibag_hip_assoc` and the entries of
// include/hibag_hip.h that use it.  Kernels: hibag_k_assoc.h and k_ld_gram<1> of hibag_k_ld.h; definitions: DESIGN.md
// section 20.
//
// hibag_hip_assoc_new keeps the samples with two known alleles, builds the int8 feature rows of every test once on the
// device the creating thread had selected, and runs the observed labelling through the same Gram and statistic kernels
// as the permutations.  hibag_hip_assoc_permute then works in panels of permutations: label rows (k_assoc_permute), one
// Gram features x labels, one pass over it (k_assoc_stat).  A handle has one stream and is used by one host thread at a time.
//
// hibag_hip_assoc_glm (hlaAssocGlm; kernels: hibag_k_glm.h) fits one logistic regression per test on
// the same feature rows, with the kept samples' labels that the handle keeps in `y` (the `labels` panel is overwritten by
// every permutation call).

#include "hibag_internal.h"
#include "hibag_k_assoc.h"
#include "hibag_k_glm.h"

using hibag_detail::DevBuf;

struct hibag_hip_assoc {
	int device = 0;
	AssocDims D;
	int n_case = 0, rows = 0, kp = 0;
	hipStream_t st = nullptr;
	DevBuf feat, row_sum, stat_obs;              // int8 [rows][kp], int32 [rows], double [n_test]
	DevBuf labels, gram, max_stat, count;        // per-call panel: int8 [pp][kp], int32 [rows][pp]; double [n_perm]; uint64 [n_test]
	DevBuf y;                                    // int8 [kp]: the kept samples' labels, zero padding (hibag_hip_assoc_glm)
	DevBuf glm_in, glm_img, glm_wt, glm_fits, glm_out; // hibag_hip_assoc_glm: covariates and weights as given, the operand image, the padded weights, GlmFit [n_fit], the outputs
	std::vector<int32_t> h_row_sum;              // the feature rows' sums [rows]
	std::vector<double> h_stat;                  // the observed statistics and tables, made once by hibag_hip_assoc_new
	std::vector<int64_t> h_table;

	~hibag_hip_assoc()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamSynchronize(st);
		for (DevBuf *b : {&feat, &row_sum, &stat_obs, &labels, &gram, &max_stat, &count, &y, &glm_in, &glm_img, &glm_wt, &glm_fits, &glm_out}) b->release();
		if (st) (void)hipStreamDestroy(st);
	}
};

namespace {

constexpr int kMaxSamples = 1 << 24;             // every integer of the statistics fits int64, every converted product is exact in double
constexpr int kMaxTests = 32767;                 // two feature rows per test at most, a grid dimension of rows
constexpr size_t kPanelBytes = (size_t)64 << 20; // default size of a panel's label operand and of its int32 Gram, whichever is larger

size_t pad_to(size_t x, size_t m) { return (x + m - 1) / m * m; }

// permutations of one panel: HIBAG_ASSOC_PANEL_PERMS (read per call), else about kPanelBytes per buffer in whole tiles
int panel_perms(const hibag_hip_assoc *h, int64_t n_perm)
{
	const char *e = getenv("HIBAG_ASSOC_PANEL_PERMS");
	long pp = e && *e ? strtol(e, nullptr, 10) : 0;
	if (pp <= 0) {
		const size_t per = std::max<size_t>((size_t)h->kp, sizeof(int32_t) * (size_t)h->rows);
		pp = (long)(kPanelBytes / per) / HIBAG_LD_TILE * HIBAG_LD_TILE;
		pp = std::max<long>(pp, HIBAG_LD_TILE);
	}
	return (int)std::min<int64_t>(std::min<long>(pp, 1 << 22), n_perm);
}

// C [rows][n_lab] (row stride n_lab) = features x labels
void launch_gram(const hibag_hip_assoc *h, const int8_t *labels, int n_lab, int32_t *C)
{
	LdGramOut O;
	O.out32 = C;
	O.ld = (size_t)n_lab;
	const dim3 grid((n_lab + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE, (h->rows + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE);
	hipLaunchKernelGGL(k_ld_gram<1>, grid, dim3(256), 0, h->st, h->feat.as<int8_t>(), h->rows, labels, n_lab, h->kp, O);
}

// the label rows of permutations p0 .. p0 + n_lab - 1 into h->labels
int enqueue_labels(hibag_hip_assoc *h, uint64_t seed, uint64_t p0, int n_lab)
{
	hipLaunchKernelGGL(k_assoc_permute, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, h->D.n, h->n_case, h->kp, seed, p0, n_lab,
		h->labels.as<int8_t>());
	HIP_TRY(hipGetLastError());
	return 0;
}

// what hibag_hip_assoc_new does on the device: features, then the observed labelling as a panel of one
int build(hibag_hip_assoc *h, const std::vector<int32_t> &a1, const std::vector<int32_t> &a2, const std::vector<int8_t> &y,
	const std::vector<int32_t> &group_of, int n_allele, const std::vector<int32_t> &part, const std::vector<int32_t> &lev)
{
	const int n = h->D.n, T = h->D.n_test, rows = h->rows, kp = h->kp;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
	DevBuf d_a, d_g, d_t;                        // alleles [2][n], the partitions, part / level of every test: needed by k_assoc_features only
	struct Release { DevBuf &a, &b, &c; ~Release() { a.release(); b.release(); c.release(); } } rel{d_a, d_g, d_t};
	if (h->feat.reserve((size_t)rows * kp) || h->row_sum.reserve(sizeof(int32_t) * rows) || h->stat_obs.reserve(sizeof(double) * T) ||
		h->labels.reserve((size_t)kp) || h->y.reserve((size_t)kp) || h->gram.reserve(sizeof(int32_t) * rows) ||
		d_a.reserve(sizeof(int32_t) * 2 * std::max(n, 1)) || d_g.reserve(sizeof(int32_t) * group_of.size()) ||
		d_t.reserve(sizeof(int32_t) * 2 * T))
		return HIBAG_HIP_ENOMEM;
	int32_t *da = d_a.as<int32_t>(), *dt = d_t.as<int32_t>();
	if (n) {
		HIP_TRY(hipMemcpyAsync(da, a1.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(da + n, a2.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st));
	}
	HIP_TRY(hipMemcpyAsync(d_g.p, group_of.data(), sizeof(int32_t) * group_of.size(), hipMemcpyHostToDevice, h->st));
	HIP_TRY(hipMemcpyAsync(dt, part.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, h->st));
	HIP_TRY(hipMemcpyAsync(dt + T, lev.data(), sizeof(int32_t) * T, hipMemcpyHostToDevice, h->st));
	HIP_TRY(hipMemsetAsync(h->row_sum.p, 0, sizeof(int32_t) * rows, h->st));
	hipLaunchKernelGGL(k_assoc_features, dim3((kp + 1023) / 1024, rows), dim3(256), 0, h->st, da, da + n, h->D, d_g.as<int32_t>(),
		n_allele, dt, dt + T, kp, h->feat.as<int8_t>(), h->row_sum.as<int32_t>());
	HIP_TRY(hipGetLastError());

	// the observed labelling: y over the kept samples, zero padding
	std::vector<int8_t> row((size_t)kp, 0);
	std::copy(y.begin(), y.end(), row.begin());
	HIP_TRY(hipMemcpyAsync(h->labels.p, row.data(), (size_t)kp, hipMemcpyHostToDevice, h->st));
	HIP_TRY(hipMemcpyAsync(h->y.p, row.data(), (size_t)kp, hipMemcpyHostToDevice, h->st));
	launch_gram(h, h->labels.as<int8_t>(), 1, h->gram.as<int32_t>());
	hipLaunchKernelGGL(k_assoc_stat, dim3(1), dim3(64), 0, h->st, h->gram.as<int32_t>(), (size_t)1, 1, h->D, h->row_sum.as<int32_t>(),
		h->stat_obs.as<double>(), (double *)nullptr, (const double *)nullptr, (unsigned long long *)nullptr);
	HIP_TRY(hipGetLastError());
	std::vector<int32_t> x((size_t)rows), r((size_t)rows);
	h->h_stat.resize((size_t)T);
	HIP_TRY(hipMemcpyAsync(x.data(), h->gram.p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(r.data(), h->row_sum.p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(h->h_stat.data(), h->stat_obs.p, sizeof(double) * T, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipStreamSynchronize(h->st));
	h->h_row_sum = r;

	// the tables, rows (none, carrier) or (none, het, hom) x columns (control, case), from the exact sums
	h->h_table.assign((size_t)T * 6, 0);
	const int64_t N = h->D.N, c1 = h->D.c1;
	for (int t = 0; t < T; t++) {
		int64_t *tab = &h->h_table[(size_t)t * 6];
		if (h->D.model == ASSOC_GENOTYPE) {
			const int64_t r_het = r[2 * t], r_hom = r[2 * t + 1], x_het = x[2 * t], x_hom = x[2 * t + 1];
			const int64_t r_non = N - r_het - r_hom, x_non = c1 - x_het - x_hom;
			tab[0] = r_non - x_non; tab[1] = x_non;
			tab[2] = r_het - x_het; tab[3] = x_het;
			tab[4] = r_hom - x_hom; tab[5] = x_hom;
		} else {
			const int64_t r1 = r[t], a = x[t], r2 = N - r1;
			tab[0] = r2 - (c1 - a); tab[1] = c1 - a;
			tab[2] = r1 - a; tab[3] = a;
		}
	}
	return 0;
}

} // namespace

extern "C" {

hibag_hip_assoc *hibag_hip_assoc_new(const int32_t *allele1, const int32_t *allele2, const int32_t *y, int n_samp, int n_allele,
	const int32_t *group_of, int n_part, int model)
{
	if (!allele1 || !allele2 || !y || n_samp <= 0 || n_allele <= 0 || n_part < 0 || (n_part > 0 && !group_of)) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: need allele1, allele2, y, n_samp > 0, n_allele > 0 and group_of for n_part > 0 "
			"(got %d samples, %d alleles, %d partitions)", n_samp, n_allele, n_part);
		return nullptr;
	}
	if (n_samp > kMaxSamples) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: %d samples; at most 2^24 keep the statistics' integers exact in double", n_samp);
		return nullptr;
	}
	if (model < ASSOC_DOMINANT || model > ASSOC_GENOTYPE) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: model %d; 0 dominant, 1 additive, 2 recessive, 3 genotype", model);
		return nullptr;
	}
	if (n_allele > kMaxTests) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: more than %d tests", kMaxTests);
		return nullptr;
	}
	// the kept samples, in order: both alleles known
	std::vector<int32_t> a1, a2;
	std::vector<int8_t> yk;
	int n_case = 0;
	for (int s = 0; s < n_samp; s++) {
		const int32_t v[2] = {allele1[s], allele2[s]};
		for (int32_t a : v)
			if (a != HIBAG_HIP_NA_INTEGER && (a < 0 || a >= n_allele)) {
				hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: sample %d has allele index %d, outside [0, %d) and not NA", s, a, n_allele);
				return nullptr;
			}
		if (y[s] != 0 && y[s] != 1) {
			hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: y[%d] = %d; the label is 0 (control) or 1 (case)", s, y[s]);
			return nullptr;
		}
		if (v[0] == HIBAG_HIP_NA_INTEGER || v[1] == HIBAG_HIP_NA_INTEGER) continue;
		a1.push_back(v[0]); a2.push_back(v[1]); yk.push_back((int8_t)y[s]);
		n_case += y[s];
	}
	// the partitions with the identity in front, and the tests: the alleles, then every level of every partition
	std::vector<int32_t> table((size_t)(n_part + 1) * n_allele), part, lev;
	for (int a = 0; a < n_allele; a++) { table[a] = a; part.push_back(0); lev.push_back(a); }
	for (int q = 0; q < n_part; q++) {
		int32_t top = -1;
		for (int a = 0; a < n_allele; a++) {
			const int32_t g = group_of[(size_t)q * n_allele + a];
			if (g < 0 || g >= kMaxTests) {
				hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: group_of[%d][%d] = %d is outside [0, %d)", q, a, g, kMaxTests);
				return nullptr;
			}
			table[(size_t)(q + 1) * n_allele + a] = g;
			top = std::max(top, g);
		}
		if (part.size() + (size_t)top + 1 > (size_t)kMaxTests) { part.resize((size_t)kMaxTests + 1); break; }
		for (int32_t l = 0; l <= top; l++) { part.push_back(q + 1); lev.push_back(l); }
	}
	if (part.size() > (size_t)kMaxTests) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_new: more than %d tests", kMaxTests);
		return nullptr;
	}
	hibag_hip_assoc *h = new (std::nothrow) hibag_hip_assoc;
	if (!h) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	h->device = hibag_selected_device();
	h->D.model = model;
	h->D.n = (int)a1.size();
	h->D.n_test = (int)part.size();
	const int unit = model == ASSOC_ADDITIVE ? 2 : 1;
	h->D.N = (long long)unit * h->D.n;
	h->D.c1 = (long long)unit * n_case;
	h->n_case = n_case;
	h->rows = (model == ASSOC_GENOTYPE ? 2 : 1) * h->D.n_test;
	h->kp = (int)std::max<size_t>(pad_to((size_t)h->D.n, HIBAG_LD_KPAD), HIBAG_LD_KPAD);
	if (build(h, a1, a2, yk, table, n_allele, part, lev) != 0) { delete h; return nullptr; }
	return h;
}

void hibag_hip_assoc_free(hibag_hip_assoc *h) { delete h; }

int hibag_hip_assoc_n_tests(const hibag_hip_assoc *h) { return h ? h->D.n_test : hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_n_tests: null handle"); }

int hibag_hip_assoc_observed(hibag_hip_assoc *h, double *stat, int64_t *table)
{
	if (!h || !stat || !table) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_observed: null argument");
	std::copy(h->h_stat.begin(), h->h_stat.end(), stat);
	std::copy(h->h_table.begin(), h->h_table.end(), table);
	return 0;
}

int hibag_hip_assoc_permute(hibag_hip_assoc *h, uint64_t seed, uint64_t perm0, int64_t n_perm, double *max_stat, int64_t *count_point)
{
	if (!h || n_perm < 0 || !count_point || (n_perm > 0 && !max_stat))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_permute: null argument or n_perm < 0");
	if (perm0 < 1 || perm0 + (uint64_t)n_perm < perm0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_permute: permutations are numbered from 1 (0 is the observed labelling) and stay below 2^64");
	const int T = h->D.n_test;
	std::fill(count_point, count_point + T, (int64_t)0);
	if (n_perm == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = panel_perms(h, n_perm);
	if (h->labels.reserve((size_t)pp * h->kp) || h->gram.reserve(sizeof(int32_t) * (size_t)h->rows * pp) ||
		h->max_stat.reserve(sizeof(double) * (size_t)n_perm) || h->count.reserve(sizeof(unsigned long long) * T))
		return HIBAG_HIP_ENOMEM;
	HIP_TRY(hipMemsetAsync(h->count.p, 0, sizeof(unsigned long long) * T, h->st));
	for (int64_t done = 0; done < n_perm; done += pp) {
		const int n_lab = (int)std::min<int64_t>(pp, n_perm - done);
		int e = enqueue_labels(h, seed, perm0 + (uint64_t)done, n_lab);
		if (e) { (void)hipStreamSynchronize(h->st); return e; }
		launch_gram(h, h->labels.as<int8_t>(), n_lab, h->gram.as<int32_t>());
		hipLaunchKernelGGL(k_assoc_stat, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, h->gram.as<int32_t>(), (size_t)n_lab, n_lab, h->D,
			h->row_sum.as<int32_t>(), (double *)nullptr, h->max_stat.as<double>() + done, h->stat_obs.as<double>(),
			h->count.as<unsigned long long>());
		if (hipGetLastError() != hipSuccess) {
			(void)hipStreamSynchronize(h->st);
			return hibag_fail(HIBAG_HIP_ENODEV, "hibag_hip_assoc_permute: a kernel launch failed");
		}
	}
	static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
	HIP_TRY(hipMemcpyAsync(max_stat, h->max_stat.p, sizeof(double) * (size_t)n_perm, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(count_point, h->count.p, sizeof(int64_t) * T, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipStreamSynchronize(h->st));
	return 0;
}

int hibag_hip_assoc_labels(hibag_hip_assoc *h, uint64_t seed, uint64_t perm0, int n, int8_t *out)
{
	if (!h || n < 0 || (n > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_labels: null argument or n < 0");
	if (perm0 < 1 || perm0 + (uint64_t)n < perm0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_labels: permutations are numbered from 1 (0 is the observed labelling) and stay below 2^64");
	if (n == 0 || h->D.n == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = panel_perms(h, n);
	if (h->labels.reserve((size_t)pp * h->kp)) return HIBAG_HIP_ENOMEM;
	for (int done = 0; done < n; done += pp) {
		const int n_lab = std::min(pp, n - done);
		int e = enqueue_labels(h, seed, perm0 + (uint64_t)done, n_lab);
		if (e) { (void)hipStreamSynchronize(h->st); return e; }
		// the rows without their padding; the next panel overwrites the buffer, so this one is on the host first
		HIP_TRY(hipMemcpy2DAsync(out + (size_t)done * h->D.n, (size_t)h->D.n, h->labels.p, (size_t)h->kp, (size_t)h->D.n, (size_t)n_lab,
			hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
	}
	return 0;
}

int hibag_hip_assoc_n_kept(const hibag_hip_assoc *h) { return h ? h->D.n : hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_n_kept: null handle"); }

int hibag_hip_assoc_feature_rows(hibag_hip_assoc *h, int row0, int n_rows, int8_t *out)
{
	if (!h || n_rows < 0 || (n_rows > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_feature_rows: null argument or n_rows < 0");
	if (row0 < 0 || row0 > h->rows || n_rows > h->rows - row0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_feature_rows: rows %d .. %d + %d are outside the handle's %d", row0, row0, n_rows, h->rows);
	if (n_rows == 0 || h->D.n == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipMemcpy2DAsync(out, (size_t)h->D.n, h->feat.as<int8_t>() + (size_t)row0 * h->kp, (size_t)h->kp, (size_t)h->D.n, (size_t)n_rows,
		hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipStreamSynchronize(h->st));
	return 0;
}

int hibag_hip_assoc_glm(hibag_hip_assoc *h, const double *covar, int n_covar, const double *weight, int maxit, double epsilon,
	double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags)
{
	if (!h || !coef || !se || !deviance || !iterations || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: null argument");
	if (n_covar < 0 || n_covar > HIBAG_HIP_GLM_MAX_COVAR || (n_covar > 0 && !covar))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: %d covariates; 0 .. %d, with covar", n_covar, HIBAG_HIP_GLM_MAX_COVAR);
	if (maxit < 1) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: maxit = %d; at least 1", maxit);
	if (!(epsilon > 0)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: epsilon must be > 0");
	static_assert(GLM_COV0 + HIBAG_HIP_GLM_MAX_COVAR == GLM_SLOTS - 1, "intercept, two h slots, the covariates, then z");
	const int n = h->D.n, T = h->D.n_test, kp = h->kp, q = n_covar, n_fit = T + 1;
	for (size_t i = 0; i < (size_t)q * n; i++)
		if (!std::isfinite(covar[i]))
			return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: covariate %zu of kept sample %zu is not finite", i / n, i % n);
	if (weight)
		for (int i = 0; i < n; i++)
			if (!std::isfinite(weight[i]) || weight[i] < 0)
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: weight[%d] = %g; weights are finite and >= 0", i, weight[i]);

	// the fits: which feature rows stand behind slots 1 and 2, decided from the integer row sums
	std::vector<GlmFit> fits((size_t)n_fit);
	const std::vector<int32_t> &r = h->h_row_sum;
	for (int t = 0; t < T; t++) {
		GlmFit &f = fits[(size_t)t];
		if (h->D.model == ASSOC_GENOTYPE) {
			const int64_t het = r[2 * t], hom = r[2 * t + 1];
			f.row_a = het > 0 ? 2 * t : -1;
			f.row_b = hom > 0 ? 2 * t + 1 : -1;
			if ((het == 0 && hom == 0) || het + hom == n) f.row_a = -2;
		} else {
			const int64_t top = (int64_t)(h->D.model == ASSOC_ADDITIVE ? 2 : 1) * n;
			f.row_a = (r[t] == 0 || r[t] == top) ? -2 : t;
			f.row_b = -1;
		}
	}
	fits[(size_t)T] = GlmFit{-1, -1};

	HIP_TRY(hipSetDevice(h->device));
	const size_t in_doubles = (size_t)q * n + (weight ? (size_t)n : 0);
	const size_t out_bytes = (size_t)n_fit * (2 * GLM_SLOTS * sizeof(double) + sizeof(double) + 2 * sizeof(int32_t));
	if (h->glm_in.reserve(sizeof(double) * std::max<size_t>(in_doubles, 1)) || h->glm_img.reserve(sizeof(double) * GLM_SLOTS * (size_t)kp) ||
		h->glm_wt.reserve(sizeof(double) * (size_t)kp) || h->glm_fits.reserve(sizeof(GlmFit) * (size_t)n_fit) || h->glm_out.reserve(out_bytes))
		return HIBAG_HIP_ENOMEM;
	double *d_cov = h->glm_in.as<double>(), *d_w = weight ? d_cov + (size_t)q * n : nullptr;
	if (q) HIP_TRY(hipMemcpyAsync(d_cov, covar, sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, h->st));
	if (weight) HIP_TRY(hipMemcpyAsync(d_w, weight, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->st));
	HIP_TRY(hipMemcpyAsync(h->glm_fits.p, fits.data(), sizeof(GlmFit) * (size_t)n_fit, hipMemcpyHostToDevice, h->st));
	hipLaunchKernelGGL(k_glm_image, dim3((unsigned)(((size_t)kp * GLM_SLOTS + 255) / 256)), dim3(256), 0, h->st, d_cov, d_w, n, q, kp,
		h->glm_img.as<double>(), h->glm_wt.as<double>());
	HIP_TRY(hipGetLastError());
	double *d_coef = h->glm_out.as<double>(), *d_se = d_coef + (size_t)n_fit * GLM_SLOTS, *d_dev = d_se + (size_t)n_fit * GLM_SLOTS;
	int32_t *d_it = (int32_t *)(d_dev + n_fit), *d_fl = d_it + n_fit;
	hipLaunchKernelGGL(k_glm_fit, dim3(n_fit), dim3(GLM_WAVES * 64), 0, h->st, h->glm_img.as<double>(), h->glm_wt.as<double>(),
		h->y.as<int8_t>(), h->feat.as<int8_t>(), h->glm_fits.as<GlmFit>(), n, kp, q, maxit, epsilon, d_coef, d_se, d_dev, d_it, d_fl);
	if (hipGetLastError() != hipSuccess) {
		(void)hipStreamSynchronize(h->st);
		return hibag_fail(HIBAG_HIP_ENODEV, "hibag_hip_assoc_glm: a kernel launch failed");
	}
	HIP_TRY(hipMemcpyAsync(coef, d_coef, sizeof(double) * (size_t)n_fit * GLM_SLOTS, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(se, d_se, sizeof(double) * (size_t)n_fit * GLM_SLOTS, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(deviance, d_dev, sizeof(double) * (size_t)n_fit, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(iterations, d_it, sizeof(int32_t) * (size_t)n_fit, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipMemcpyAsync(flags, d_fl, sizeof(int32_t) * (size_t)n_fit, hipMemcpyDeviceToHost, h->st));
	HIP_TRY(hipStreamSynchronize(h->st));
	return 0;
}

} // extern "C"
