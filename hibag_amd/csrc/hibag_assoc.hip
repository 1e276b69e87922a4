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
//
// hibag_hip_assoc_glm_sets (hlaAssocOmnibus; kernels: hibag_k_glmw.h) fits one regression per SET of
// feature rows -- all residues of a position at once -- over a 32-slot design, with aliased columns dropped; it shares the
// buffers and the driver (`GlmCall`) of hibag_hip_assoc_glm.
//
// hibag_hip_assoc_glm_terms (hlaAssocInteract; kernels: hibag_k_glmt.h) fits one regression per record of
// up to three TERMS -- a feature row, or the product of two, formed while the samples are walked -- on the same buffers and
// driver; hibag_hip_assoc_row_gram gives the exact co-carriage sums of feature rows from k_ld_gram<1>.
//
// hibag_hip_assoc_cox (hlaAssocSurv; kernels: hibag_k_cox.h) fits one Cox regression per test on a handle
// whose samples come in time order; it uses `GlmCall`'s argument checks and the regression buffers, with launches of its own
// (the base model first, whose coefficients the tests start from).
//
// hibag_hip_assoc_quant_* (hlaAssocQuant; kernels: hibag_k_quant.h) test a quantitative trait on the
// same feature rows, through a handle of their own that borrows this one; hibag_hip_assoc_score_* (hlaAssocScore, DESIGN.md
// section 28; kernels: hibag_k_score.h) run covariate-adjusted score tests with multiplier resampling the same way; both are
// at the end of the file.  The permutation and resampling sides share one panel driver (`panel_perms`, `check_perm_range`,
// `for_each_panel`, `PermOut`, `download_panels`), and every function that enqueues work on host memory follows one drain
// rule (`enqueued`): the first namespace below.

#include "hibag_internal.h"
#include "hibag_k_assoc.h"
#include "hibag_k_glm.h"
#include "hibag_k_glmw.h"
#include "hibag_k_glmt.h"
#include "hibag_k_cox.h"
#include "hibag_k_quant.h"
#include "hibag_k_score.h"
#include "hibag_k_rscore.h"

using hibag_detail::DevBuf;

namespace {

struct TempBuf : DevBuf { ~TempBuf() { release(); } };   // a buffer of one function's frame

// The drain rule.  HIP_TRY returns on the spot, and what an entry has enqueued by then may still read from, or write into,
// memory of the frame that is left or of the caller.  So every function that enqueues such work does it inside `body`, which
// ends with its own wait for the stream; when `body` fails part-way, the stream is drained before the frame goes away.
// Host memory that a copy touches is therefore declared OUTSIDE `body`: its own locals are gone before the drain.
template <class Body> int enqueued(hipStream_t st, Body body)
{
	const int rc = body();
	if (rc) (void)hipStreamSynchronize(st);
	return rc;
}

// Permutations of one panel of a call for `n`: the variable `env` (read per call), else `budget` bytes at `per_perm` bytes a
// permutation in whole tiles, one tile at least; never above 2^22.  `whole_tiles` (the quantitative side, whose kernels work
// on whole tiles): the variable's value and the call's count are rounded to whole tiles too, else taken as they are.
int panel_perms(const char *env, size_t budget, size_t per_perm, int tile, bool whole_tiles, int64_t n)
{
	const char *e = getenv(env);
	long pp = e && *e ? strtol(e, nullptr, 10) : 0;
	const bool given = pp > 0;
	if (!given) pp = (long)(budget / per_perm);
	pp = std::min<long>(pp, 1 << 22);
	if (whole_tiles || !given) pp = std::max<long>(pp / tile * tile, tile);
	return (int)std::min<int64_t>(pp, whole_tiles ? (n + tile - 1) / tile * tile : n);
}

// permutations perm0 .. perm0 + n - 1 of `entry`; `observed` is what permutation 0 stands for
int check_perm_range(const char *entry, const char *observed, uint64_t perm0, uint64_t n)
{
	if (perm0 < 1 || perm0 + n < perm0)
		return hibag_fail(HIBAG_HIP_EINVAL, "%s: permutations are numbered from 1 (0 is the observed %s) and stay below 2^64", entry, observed);
	return 0;
}

// panel(done, n_lab) for the panels of `pp` that cover [0, n)
template <class Panel> int for_each_panel(int64_t n, int pp, Panel panel)
{
	for (int64_t done = 0; done < n; done += pp)
		if (int rc = panel(done, (int)std::min<int64_t>(pp, n - done))) return rc;
	return 0;
}

// `n` rows of `width` bytes to `out`: made panel by panel by make(done, n_lab) at `src` (row pitch `pitch`) and copied without
// their padding; the next panel overwrites the buffer, so each one is on the host first
template <class Make> int download_panels(hipStream_t st, int n, int pp, const void *src, size_t pitch, size_t width, void *out, Make make)
{
	return enqueued(st, [&]() -> int {
		return for_each_panel(n, pp, [&](int64_t done, int n_lab) -> int {
			if (int rc = make(done, n_lab)) return rc;
			HIP_TRY(hipMemcpy2DAsync((char *)out + (size_t)done * width, width, src, pitch, width, (size_t)n_lab, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			return 0;
		});
	});
}

// What a permutation call accumulates on the device: every permutation's largest statistic (`width` of them for an entry that
// keeps several maxima per permutation) and, per test, the number of permutations at or above the observed statistic.
struct PermOut {
	DevBuf max_stat, count;                      // double [n_perm][width]; uint64 [n_test]

	int reserve(int64_t n_perm, int T, int width = 1)
	{
		return max_stat.reserve(sizeof(double) * (size_t)n_perm * std::max(width, 1)) || count.reserve(sizeof(unsigned long long) * (size_t)std::max(T, 1));
	}
	void release() { max_stat.release(); count.release(); }

	// one call: the counts zeroed, panel(done, n_lab) for every panel of `pp`, both outputs on the host
	template <class Panel> int run(hipStream_t st, int T, int64_t n_perm, int pp, double *h_max, int64_t *h_count, Panel panel, int width = 1)
	{
		static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts are copied as they are");
		return enqueued(st, [&]() -> int {
			HIP_TRY(hipMemsetAsync(count.p, 0, sizeof(unsigned long long) * (size_t)T, st));
			if (int rc = for_each_panel(n_perm, pp, panel)) return rc;
			if (width > 0) HIP_TRY(hipMemcpyAsync(h_max, max_stat.p, sizeof(double) * (size_t)n_perm * width, hipMemcpyDeviceToHost, st));
			if (T > 0) HIP_TRY(hipMemcpyAsync(h_count, count.p, sizeof(int64_t) * (size_t)T, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			return 0;
		});
	}
};

} // namespace

struct hibag_hip_assoc {
	int device = 0;
	AssocDims D;
	int n_case = 0, rows = 0, kp = 0;
	hipStream_t st = nullptr;
	DevBuf feat, row_sum, stat_obs;              // int8 [rows][kp], int32 [rows], double [n_test]
	DevBuf labels, gram;                         // per-call panel: int8 [pp][kp], int32 [rows][pp]
	PermOut out;                                 // per permutation call
	DevBuf y;                                    // int8 [kp]: the kept samples' labels, zero padding (hibag_hip_assoc_glm)
	DevBuf glm_in, glm_img, glm_wt, glm_fits, glm_out; // hibag_hip_assoc_glm: covariates and weights as given, the operand image, the padded weights, GlmFit [n_fit], the outputs
	DevBuf cox_time, cox_tab, cox_scr;           // hibag_hip_assoc_cox: the times as given, the block table (int32 [5 kp + 1]), the fits' scratch (3 kp doubles each)
	std::vector<int32_t> h_row_sum;              // the feature rows' sums [rows]
	std::vector<double> h_stat;                  // the observed statistics and tables, made once by hibag_hip_assoc_new
	std::vector<int64_t> h_table;

	~hibag_hip_assoc()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamSynchronize(st);
		for (DevBuf *b : {&feat, &row_sum, &stat_obs, &labels, &gram, &y, &glm_in, &glm_img, &glm_wt, &glm_fits, &glm_out, &cox_time, &cox_tab, &cox_scr}) b->release();
		out.release();
		if (st) (void)hipStreamDestroy(st);
	}
};

namespace {

constexpr int kMaxSamples = 1 << 24;             // every integer of the statistics fits int64, every converted product is exact in double
constexpr int kMaxTests = 32767;                 // two feature rows per test at most, a grid dimension of rows
constexpr size_t kPanelBytes = (size_t)64 << 20; // default size of a panel's label operand and of its int32 Gram, whichever is larger

size_t pad_to(size_t x, size_t m) { return (x + m - 1) / m * m; }

int assoc_panel_perms(const hibag_hip_assoc *h, int64_t n)
{
	return panel_perms("HIBAG_ASSOC_PANEL_PERMS", kPanelBytes, std::max<size_t>((size_t)h->kp, sizeof(int32_t) * (size_t)h->rows), HIBAG_LD_TILE,
		false, n);
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

// The regression driver: what hibag_hip_assoc_glm, hibag_hip_assoc_glm_sets and hibag_hip_assoc_glm_terms share.  An entry checks its arguments
// (`check_control`, what is its own, `check_values`, in the order the messages have always had), decides its fit records
// from the row sums, and hands them to `run` with its slot count and the launches of its two kernels.
struct GlmOut { double *coef, *se, *dev; int32_t *it, *fl, *df; };   // the device's outputs, carved from glm_out

struct GlmCall {
	const char *entry;
	hibag_hip_assoc *h;
	const double *covar; int q;                  // [q][n]
	const double *weight;                        // [n] or null
	int maxit; double epsilon;
	double *coef, *se, *deviance;                // the caller's [n_fit][slots] twice, [n_fit]
	int32_t *iterations, *flags, *df_h;          // the caller's [n_fit]; df_h: null for an entry without it

	int check_control(int max_covar) const
	{
		if (q < 0 || q > max_covar || (q > 0 && !covar)) return hibag_fail(HIBAG_HIP_EINVAL, "%s: %d covariates; 0 .. %d, with covar", entry, q, max_covar);
		if (maxit < 1) return hibag_fail(HIBAG_HIP_EINVAL, "%s: maxit = %d; at least 1", entry, maxit);
		if (!(epsilon > 0)) return hibag_fail(HIBAG_HIP_EINVAL, "%s: epsilon must be > 0", entry);
		return 0;
	}

	int check_values() const
	{
		const int n = h->D.n;
		for (size_t i = 0; i < (size_t)q * n; i++)
			if (!std::isfinite(covar[i])) return hibag_fail(HIBAG_HIP_EINVAL, "%s: covariate %zu of kept sample %zu is not finite", entry, i / n, i % n);
		if (weight)
			for (int i = 0; i < n; i++)
				if (!std::isfinite(weight[i]) || weight[i] < 0)
					return hibag_fail(HIBAG_HIP_EINVAL, "%s: weight[%d] = %g; weights are finite and >= 0", entry, i, weight[i]);
		return 0;
	}

	// Uploads the covariates, the weights and the `n_fit` fit records of `fit_bytes` each, has `image(d_cov, d_w)` build the
	// operand image and `fit(O)` run the fits into the outputs O, and downloads them.
	template <class Image, class Fit> int run(int slots, const void *fits, size_t fit_bytes, int n_fit, Image image, Fit fit) const
	{
		const int n = h->D.n, kp = h->kp;
		const hipStream_t st = h->st;
		HIP_TRY(hipSetDevice(h->device));
		const size_t in_doubles = (size_t)q * n + (weight ? (size_t)n : 0), nf = (size_t)n_fit;
		const size_t out_bytes = nf * (2 * slots * sizeof(double) + sizeof(double) + (df_h ? 3 : 2) * sizeof(int32_t));
		if (h->glm_in.reserve(sizeof(double) * std::max<size_t>(in_doubles, 1)) || h->glm_img.reserve(sizeof(double) * slots * (size_t)kp) ||
			h->glm_wt.reserve(sizeof(double) * (size_t)kp) || h->glm_fits.reserve(fit_bytes * nf) || h->glm_out.reserve(out_bytes))
			return HIBAG_HIP_ENOMEM;
		double *d_cov = h->glm_in.as<double>(), *d_w = weight ? d_cov + (size_t)q * n : nullptr;
		GlmOut O;
		O.coef = h->glm_out.as<double>(); O.se = O.coef + nf * slots; O.dev = O.se + nf * slots;
		O.it = (int32_t *)(O.dev + nf); O.fl = O.it + nf; O.df = df_h ? O.fl + nf : nullptr;
		return enqueued(h->st, [&]() -> int {
			if (q) HIP_TRY(hipMemcpyAsync(d_cov, covar, sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, st));
			if (weight) HIP_TRY(hipMemcpyAsync(d_w, weight, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(h->glm_fits.p, fits, fit_bytes * nf, hipMemcpyHostToDevice, st));
			image(d_cov, d_w);
			HIP_TRY(hipGetLastError());
			fit(O);
			if (hipGetLastError() != hipSuccess) return hibag_fail(HIBAG_HIP_ENODEV, "%s: a kernel launch failed", entry);
			HIP_TRY(hipMemcpyAsync(coef, O.coef, sizeof(double) * nf * slots, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(se, O.se, sizeof(double) * nf * slots, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(deviance, O.dev, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(iterations, O.it, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(flags, O.fl, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
			if (df_h) HIP_TRY(hipMemcpyAsync(df_h, O.df, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			return 0;
		});
	}
};

// C [na][nb] on the host: C[i][j] = the sum over the samples of feature rows a0 + i and b0 + j, exact (k_ld_gram<1> on the
// handle's rows as both operands; the padding columns hold zeros).  The rows are inside the handle.
int rows_gram(hibag_hip_assoc *h, int a0, int na, int b0, int nb, int32_t *out)
{
	if (h->gram.reserve(sizeof(int32_t) * (size_t)na * nb)) return HIBAG_HIP_ENOMEM;
	return enqueued(h->st, [&]() -> int {
		LdGramOut O;
		O.out32 = h->gram.as<int32_t>();
		O.ld = (size_t)nb;
		const dim3 grid((nb + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE, (na + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE);
		hipLaunchKernelGGL(k_ld_gram<1>, grid, dim3(256), 0, h->st, h->feat.as<int8_t>() + (size_t)a0 * h->kp, na,
			h->feat.as<int8_t>() + (size_t)b0 * h->kp, nb, h->kp, O);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(out, h->gram.p, sizeof(int32_t) * (size_t)na * nb, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	});
}

constexpr int kMaxGramRows = 8192;               // hibag_hip_assoc_row_gram: 256 MiB of int32 at most
constexpr int kGramBlock = 2048;                 // hibag_hip_assoc_glm_terms: the products' sums come in blocks of rows x rows
constexpr int kMaxTermFits = 1 << 20;
constexpr size_t kCoxScratchBytes = (size_t)256 << 20; // hibag_hip_assoc_cox: the fits of one launch share this much scratch, one fit at least

// what hibag_hip_assoc_new does on the device: features, then the observed labelling as a panel of one
int build(hibag_hip_assoc *h, const std::vector<int32_t> &a1, const std::vector<int32_t> &a2, const std::vector<int8_t> &y,
	const std::vector<int32_t> &group_of, int n_allele, const std::vector<int32_t> &part, const std::vector<int32_t> &lev)
{
	const int n = h->D.n, T = h->D.n_test, rows = h->rows, kp = h->kp;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
	TempBuf d_a, d_g, d_t;                       // alleles [2][n], the partitions, part / level of every test: needed by k_assoc_features only
	if (h->feat.reserve((size_t)rows * kp) || h->row_sum.reserve(sizeof(int32_t) * rows) || h->stat_obs.reserve(sizeof(double) * T) ||
		h->labels.reserve((size_t)kp) || h->y.reserve((size_t)kp) || h->gram.reserve(sizeof(int32_t) * rows) ||
		d_a.reserve(sizeof(int32_t) * 2 * std::max(n, 1)) || d_g.reserve(sizeof(int32_t) * group_of.size()) ||
		d_t.reserve(sizeof(int32_t) * 2 * T))
		return HIBAG_HIP_ENOMEM;
	int32_t *da = d_a.as<int32_t>(), *dt = d_t.as<int32_t>();
	std::vector<int8_t> row((size_t)kp, 0);      // the observed labelling: y over the kept samples, zero padding
	std::copy(y.begin(), y.end(), row.begin());
	std::vector<int32_t> x((size_t)rows), r((size_t)rows);
	h->h_stat.resize((size_t)T);
	if (int rc = enqueued(h->st, [&]() -> int {
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
		HIP_TRY(hipMemcpyAsync(h->labels.p, row.data(), (size_t)kp, hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(h->y.p, row.data(), (size_t)kp, hipMemcpyHostToDevice, h->st));
		launch_gram(h, h->labels.as<int8_t>(), 1, h->gram.as<int32_t>());
		hipLaunchKernelGGL(k_assoc_stat, dim3(1), dim3(64), 0, h->st, h->gram.as<int32_t>(), (size_t)1, 1, h->D, h->row_sum.as<int32_t>(),
			h->stat_obs.as<double>(), (double *)nullptr, (const double *)nullptr, (unsigned long long *)nullptr);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(x.data(), h->gram.p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(r.data(), h->row_sum.p, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(h->h_stat.data(), h->stat_obs.p, sizeof(double) * T, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	})) return rc;
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
	if (int rc = check_perm_range("hibag_hip_assoc_permute", "labelling", perm0, (uint64_t)n_perm)) return rc;
	const int T = h->D.n_test;
	std::fill(count_point, count_point + T, (int64_t)0);
	if (n_perm == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = assoc_panel_perms(h, n_perm);
	if (h->labels.reserve((size_t)pp * h->kp) || h->gram.reserve(sizeof(int32_t) * (size_t)h->rows * pp) || h->out.reserve(n_perm, T))
		return HIBAG_HIP_ENOMEM;
	return h->out.run(h->st, T, n_perm, pp, max_stat, count_point, [&](int64_t done, int n_lab) -> int {
		if (int e = enqueue_labels(h, seed, perm0 + (uint64_t)done, n_lab)) return e;
		launch_gram(h, h->labels.as<int8_t>(), n_lab, h->gram.as<int32_t>());
		hipLaunchKernelGGL(k_assoc_stat, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, h->gram.as<int32_t>(), (size_t)n_lab, n_lab, h->D,
			h->row_sum.as<int32_t>(), (double *)nullptr, h->out.max_stat.as<double>() + done, h->stat_obs.as<double>(),
			h->out.count.as<unsigned long long>());
		if (hipGetLastError() != hipSuccess) return hibag_fail(HIBAG_HIP_ENODEV, "hibag_hip_assoc_permute: a kernel launch failed");
		return 0;
	});
}

int hibag_hip_assoc_labels(hibag_hip_assoc *h, uint64_t seed, uint64_t perm0, int n, int8_t *out)
{
	if (!h || n < 0 || (n > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_labels: null argument or n < 0");
	if (int rc = check_perm_range("hibag_hip_assoc_labels", "labelling", perm0, (uint64_t)n)) return rc;
	if (n == 0 || h->D.n == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = assoc_panel_perms(h, n);
	if (h->labels.reserve((size_t)pp * h->kp)) return HIBAG_HIP_ENOMEM;
	return download_panels(h->st, n, pp, h->labels.p, (size_t)h->kp, (size_t)h->D.n, out,
		[&](int64_t done, int n_lab) -> int { return enqueue_labels(h, seed, perm0 + (uint64_t)done, n_lab); });
}

int hibag_hip_assoc_n_kept(const hibag_hip_assoc *h) { return h ? h->D.n : hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_n_kept: null handle"); }

int hibag_hip_assoc_feature_rows(hibag_hip_assoc *h, int row0, int n_rows, int8_t *out)
{
	if (!h || n_rows < 0 || (n_rows > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_feature_rows: null argument or n_rows < 0");
	if (row0 < 0 || row0 > h->rows || n_rows > h->rows - row0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_feature_rows: rows %d .. %d + %d are outside the handle's %d", row0, row0, n_rows, h->rows);
	if (n_rows == 0 || h->D.n == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	return download_panels(h->st, n_rows, n_rows, h->feat.as<int8_t>() + (size_t)row0 * h->kp, (size_t)h->kp, (size_t)h->D.n, out,
		[](int64_t, int) -> int { return 0; });             // the rows are there already: one panel, nothing to make
}

int hibag_hip_assoc_glm(hibag_hip_assoc *h, const double *covar, int n_covar, const double *weight, int maxit, double epsilon,
	double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags)
{
	if (!h || !coef || !se || !deviance || !iterations || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm: null argument");
	static_assert(GLM_COV0 + HIBAG_HIP_GLM_MAX_COVAR == GLM_SLOTS - 1, "intercept, two h slots, the covariates, then z");
	const GlmCall call{"hibag_hip_assoc_glm", h, covar, n_covar, weight, maxit, epsilon, coef, se, deviance, iterations, flags, nullptr};
	if (int rc = call.check_control(HIBAG_HIP_GLM_MAX_COVAR)) return rc;
	if (int rc = call.check_values()) return rc;
	const int n = h->D.n, T = h->D.n_test, kp = h->kp, q = n_covar, n_fit = T + 1;

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

	return call.run(GLM_SLOTS, fits.data(), sizeof(GlmFit), n_fit,
		[&](const double *d_cov, const double *d_w) {
			hipLaunchKernelGGL(k_glm_image, dim3((unsigned)(((size_t)kp * GLM_SLOTS + 255) / 256)), dim3(256), 0, h->st, d_cov, d_w, n, q, kp,
				h->glm_img.as<double>(), h->glm_wt.as<double>());
		},
		[&](const GlmOut &O) {
			hipLaunchKernelGGL(k_glm_fit, dim3(n_fit), dim3(GLM_WAVES * 64), 0, h->st, h->glm_img.as<double>(), h->glm_wt.as<double>(),
				h->y.as<int8_t>(), h->feat.as<int8_t>(), h->glm_fits.as<GlmFit>(), n, kp, q, maxit, epsilon, O.coef, O.se, O.dev, O.it, O.fl);
		});
}

int hibag_hip_assoc_row_sums(hibag_hip_assoc *h, int32_t *out)
{
	if (!h || !out) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_row_sums: null argument");
	std::copy(h->h_row_sum.begin(), h->h_row_sum.end(), out);
	return 0;
}

int hibag_hip_assoc_cox_segment(int n_kept, int *step, int *segment)
{
	if (n_kept <= 0 || n_kept > kMaxSamples || !step || !segment)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_cox_segment: n_kept = %d outside 1 .. 2^24, or a null pointer", n_kept);
	static_assert(HIBAG_LD_KPAD % (COX_STEP * COX_WAVES) == 0, "the segments of k_cox_fit are whole steps and equal");
	*step = COX_STEP;
	*segment = (int)(pad_to((size_t)n_kept, HIBAG_LD_KPAD) / COX_WAVES);
	return 0;
}

int hibag_hip_assoc_cox(hibag_hip_assoc *h, const double *time, const double *covar, int n_covar, int ties, int maxit, double epsilon,
	const double *start, double *coef, double *se, double *loglik, double *score, int32_t *iterations, int32_t *flags)
{
	const char *me = "hibag_hip_assoc_cox";
	if (!h || !time || !coef || !se || !loglik || !score || !iterations || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "%s: null argument", me);
	static_assert(COX_COV0 + HIBAG_HIP_COX_MAX_COVAR < COX_ONE, "two h slots, the covariates, then the constant");
	static_assert(sizeof(CoxFit) == 2 * sizeof(int), "CoxFit records are uploaded as they are");
	const GlmCall call{me, h, covar, n_covar, nullptr, maxit, epsilon, coef, se, loglik, iterations, flags, nullptr};
	if (int rc = call.check_control(HIBAG_HIP_COX_MAX_COVAR)) return rc;
	if (ties != COX_TIES_EFRON && ties != COX_TIES_BRESLOW) return hibag_fail(HIBAG_HIP_EINVAL, "%s: ties = %d; 0 efron, 1 breslow", me, ties);
	if (int rc = call.check_values()) return rc;
	const int n = h->D.n, T = h->D.n_test, kp = h->kp, q = n_covar, n_fit = T + 1;
	for (int i = 0; i < n; i++) {
		if (!std::isfinite(time[i]) || time[i] < 0) return hibag_fail(HIBAG_HIP_EINVAL, "%s: time[%d] = %g; times are finite and >= 0", me, i, time[i]);
		if (i > 0 && time[i] > time[i - 1])
			return hibag_fail(HIBAG_HIP_EINVAL, "%s: time[%d] > time[%d]; the kept samples come in time order, latest first", me, i, i - 1);
	}
	std::vector<double> beta0((size_t)COX_SLOTS, 0.0), base((size_t)COX_SLOTS, 0.0);      // where the base model starts; where the tests do
	if (start)
		for (int j = 0; j < q; j++) {
			if (!std::isfinite(start[j])) return hibag_fail(HIBAG_HIP_EINVAL, "%s: start[%d] is not finite", me, j);
			beta0[(size_t)COX_COV0 + j] = start[j];
		}

	// the fits, the base model first: which feature rows stand behind slots 0 and 1
	std::vector<CoxFit> fits((size_t)n_fit);
	const std::vector<int32_t> &r = h->h_row_sum;
	fits[0] = CoxFit{h->n_case > 0 ? -1 : -2, -1};
	for (int t = 0; t < T; t++) {
		CoxFit &f = fits[(size_t)t + 1];
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
		if (h->n_case == 0) f.row_a = -2;
	}

	HIP_TRY(hipSetDevice(h->device));
	const hipStream_t st = h->st;
	const size_t nf = (size_t)n_fit, per_fit = sizeof(double) * 3 * (size_t)kp;
	const int batch = (int)std::min<size_t>(nf, std::max<size_t>(kCoxScratchBytes / per_fit, 1));
	if (h->glm_in.reserve(sizeof(double) * std::max<size_t>((size_t)q * n, 1)) || h->glm_img.reserve(sizeof(double) * COX_SLOTS * (size_t)kp) ||
		h->glm_fits.reserve(sizeof(CoxFit) * nf) || h->glm_out.reserve(nf * ((2 * COX_SLOTS + 2) * sizeof(double) + 2 * sizeof(int32_t)) + sizeof(double) * COX_SLOTS) ||
		h->cox_time.reserve(sizeof(double) * (size_t)n) || h->cox_tab.reserve(sizeof(int32_t) * (5 * (size_t)kp + 1)) ||
		h->cox_scr.reserve(per_fit * (size_t)batch))
		return HIBAG_HIP_ENOMEM;
	double *d_cov = h->glm_in.as<double>(), *d_time = h->cox_time.as<double>(), *d_img = h->glm_img.as<double>();
	double *o_coef = h->glm_out.as<double>(), *o_se = o_coef + nf * COX_SLOTS, *o_ll = o_se + nf * COX_SLOTS, *o_sc = o_ll + nf, *d_start = o_sc + nf;
	int32_t *o_it = (int32_t *)(d_start + COX_SLOTS), *o_fl = o_it + nf;
	int32_t *t_blk = h->cox_tab.as<int32_t>(), *t_first = t_blk + kp, *t_dk = t_first + kp + 1, *t_scan = t_dk + kp;
	const CoxTable tab{t_blk, t_first, t_dk};
	int32_t base_fl = 0;
	const std::vector<CoxFit> none(nf, CoxFit{-2, -1});
	auto launch_fits = [&](int f0, int count) {
		hipLaunchKernelGGL(k_cox_fit, dim3(count), dim3(COX_WAVES * 64), 0, st, d_img, h->y.as<int8_t>(), h->feat.as<int8_t>(),
			h->glm_fits.as<CoxFit>() + f0, tab, d_start, n, kp, q, ties, maxit, epsilon, h->cox_scr.as<double>(), o_coef + (size_t)f0 * COX_SLOTS,
			o_se + (size_t)f0 * COX_SLOTS, o_ll + f0, o_sc + f0, o_it + f0, o_fl + f0);
	};
	return enqueued(st, [&]() -> int {
		if (q) HIP_TRY(hipMemcpyAsync(d_cov, covar, sizeof(double) * (size_t)q * n, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_time, time, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(h->glm_fits.p, fits.data(), sizeof(CoxFit) * nf, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_start, beta0.data(), sizeof(double) * COX_SLOTS, hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_cox_image, dim3((unsigned)(((size_t)kp * COX_SLOTS + 255) / 256) + 1), dim3(256), 0, st, d_cov, d_time,
			h->y.as<int8_t>(), n, q, kp, d_img, t_blk, t_first, t_dk, t_scan);
		HIP_TRY(hipGetLastError());
		// the base model, whose coefficients the tests start from
		launch_fits(0, 1);
		if (hipGetLastError() != hipSuccess) return hibag_fail(HIBAG_HIP_ENODEV, "%s: a kernel launch failed", me);
		HIP_TRY(hipMemcpyAsync(base.data(), o_coef, sizeof(double) * COX_SLOTS, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(&base_fl, o_fl, sizeof(int32_t), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if (base_fl & COX_FLAG_RANK) {
			// no base model, no start: every test is reported like it
			HIP_TRY(hipMemcpyAsync(h->glm_fits.p, none.data(), sizeof(CoxFit) * nf, hipMemcpyHostToDevice, st));
			HIP_TRY(hipStreamSynchronize(st));
		}
		for (double &v : base) if (std::isnan(v)) v = 0.0;
		HIP_TRY(hipMemcpyAsync(d_start, base.data(), sizeof(double) * COX_SLOTS, hipMemcpyHostToDevice, st));
		for (int f0 = 1; f0 < n_fit; f0 += batch) {
			launch_fits(f0, std::min(batch, n_fit - f0));
			if (hipGetLastError() != hipSuccess) return hibag_fail(HIBAG_HIP_ENODEV, "%s: a kernel launch failed", me);
		}
		HIP_TRY(hipMemcpyAsync(coef, o_coef, sizeof(double) * nf * COX_SLOTS, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(se, o_se, sizeof(double) * nf * COX_SLOTS, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(loglik, o_ll, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(score, o_sc, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(iterations, o_it, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(flags, o_fl, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return 0;
	});
}

int hibag_hip_assoc_glm_sets(hibag_hip_assoc *h, const int32_t *set_start, const int32_t *set_rows, int n_sets, const double *covar,
	int n_covar, const double *weight, int maxit, double epsilon, double *coef, double *se, double *deviance, int32_t *iterations,
	int32_t *flags, int32_t *df_h)
{
	if (!h || !coef || !se || !deviance || !iterations || !flags || !df_h)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: null argument");
	static_assert(GLMW_SLOTS == HIBAG_HIP_GLM_WIDE_SLOTS && GLMW_MAX_ROWS == GLMW_SLOTS - 2, "intercept, the h slots and covariates, then z");
	static_assert(GLM_FLAG_ALIASED == HIBAG_HIP_GLM_ALIASED && GLM_FLAG_TOO_WIDE == HIBAG_HIP_GLM_TOO_WIDE, "the header's flags");
	static_assert(sizeof(GlmWideFit) == sizeof(int) * (2 + GLMW_MAX_ROWS), "uploaded as it is");
	const GlmCall call{"hibag_hip_assoc_glm_sets", h, covar, n_covar, weight, maxit, epsilon, coef, se, deviance, iterations, flags, df_h};
	if (int rc = call.check_control(GLMW_MAX_ROWS - 1)) return rc;
	if (n_sets < 0 || n_sets > kMaxTests || !set_start || set_start[0] != 0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: need 0 <= n_sets <= %d and set_start with set_start[0] = 0", kMaxTests);
	for (int t = 0; t < n_sets; t++)
		if (set_start[t + 1] < set_start[t])
			return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: set_start is not monotone at set %d", t);
	if (set_start[n_sets] > 0 && !set_rows) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: set_rows is null");
	const int n = h->D.n, kp = h->kp, q = n_covar, n_fit = n_sets + 1, room = GLMW_MAX_ROWS - q;
	if (int rc = call.check_values()) return rc;

	// the fits: a set's rows behind slots 1, 2, ... in the order given; what cannot be fitted is decided from the integer row
	// sums.  H, the h slots of the call's layout, is the largest set that is fitted.
	std::vector<GlmWideFit> fits((size_t)n_fit);
	std::vector<int> seen((size_t)h->rows, -1);
	const std::vector<int32_t> &r = h->h_row_sum;
	int H = 0;
	for (int t = 0; t < n_sets; t++) {
		GlmWideFit &f = fits[(size_t)t];
		const int32_t *rows = set_rows + set_start[t];
		const int m = set_start[t + 1] - set_start[t];
		for (int j = 0; j < m; j++) {
			if (rows[j] < 0 || rows[j] >= h->rows)
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: set %d names row %d, outside the handle's %d", t, rows[j], h->rows);
			if (seen[(size_t)rows[j]] == t)
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_sets: set %d names row %d twice", t, rows[j]);
			seen[(size_t)rows[j]] = t;
		}
		f.n_rows = -1;
		f.flags0 = GLM_FLAG_RANK;
		std::fill(f.rows, f.rows + GLMW_MAX_ROWS, -1);
		if (m > room) { f.flags0 |= GLM_FLAG_TOO_WIDE; continue; }
		int carried = 0;
		for (int j = 0; j < m; j++) carried += r[(size_t)rows[j]] > 0;
		if (carried == 0) continue;
		f.n_rows = m;
		f.flags0 = carried < m ? GLM_FLAG_ALIASED : 0;
		for (int j = 0; j < m; j++) f.rows[j] = r[(size_t)rows[j]] > 0 ? rows[j] : -1;
		H = std::max(H, m);
	}
	GlmWideFit &base = fits[(size_t)n_sets];
	base.n_rows = 0;
	base.flags0 = 0;
	std::fill(base.rows, base.rows + GLMW_MAX_ROWS, -1);

	return call.run(GLMW_SLOTS, fits.data(), sizeof(GlmWideFit), n_fit,
		[&](const double *d_cov, const double *d_w) {
			hipLaunchKernelGGL(k_glm_image_wide, dim3((unsigned)(((size_t)kp * GLMW_SLOTS + 255) / 256)), dim3(256), 0, h->st, d_cov, d_w, n, q, H,
				kp, h->glm_img.as<double>(), h->glm_wt.as<double>());
		},
		[&](const GlmOut &O) {
			hipLaunchKernelGGL(k_glm_fit_wide, dim3(n_fit), dim3(GLM_WAVES * 64), 0, h->st, h->glm_img.as<double>(), h->glm_wt.as<double>(),
				h->y.as<int8_t>(), h->feat.as<int8_t>(), h->glm_fits.as<GlmWideFit>(), n, kp, q, H, maxit, epsilon, O.coef, O.se, O.dev, O.it,
				O.fl, O.df);
		});
}

int hibag_hip_assoc_row_gram(hibag_hip_assoc *h, int row0, int n_rows, int32_t *out)
{
	if (!h || n_rows < 0 || (n_rows > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_row_gram: null argument or n_rows < 0");
	if (row0 < 0 || row0 > h->rows || n_rows > h->rows - row0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_row_gram: rows %d .. %d + %d are outside the handle's %d", row0, row0, n_rows, h->rows);
	if (n_rows > kMaxGramRows) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_row_gram: %d rows; at most %d in a call", n_rows, kMaxGramRows);
	if (n_rows == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	return rows_gram(h, row0, n_rows, row0, n_rows, out);
}

int hibag_hip_assoc_glm_terms(hibag_hip_assoc *h, const int32_t *terms, int n_fits, const double *covar, int n_covar, const double *weight,
	int maxit, double epsilon, double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags, int32_t *df_h)
{
	if (!h || !coef || !se || !deviance || !iterations || !flags || !df_h)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_terms: null argument");
	static_assert(GLMT_COV0 + HIBAG_HIP_GLM_TERMS_MAX_COVAR == GLM_SLOTS - 1 && GLMT_MAX_COVAR == HIBAG_HIP_GLM_TERMS_MAX_COVAR,
		"intercept, three term slots, the covariates, then z");
	static_assert(sizeof(GlmTermsFit) == sizeof(int) * (2 * GLMT_TERMS + 2), "uploaded as it is");
	const GlmCall call{"hibag_hip_assoc_glm_terms", h, covar, n_covar, weight, maxit, epsilon, coef, se, deviance, iterations, flags, df_h};
	if (int rc = call.check_control(HIBAG_HIP_GLM_TERMS_MAX_COVAR)) return rc;
	if (n_fits < 0 || n_fits > kMaxTermFits || (n_fits > 0 && !terms))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_terms: need 0 <= n_fits <= 2^20 and terms with fits to read (n_fits = %d)", n_fits);
	const int n = h->D.n, kp = h->kp, q = n_covar, n_fit = n_fits + 1;

	// the records as given: every term a row of the handle, or a product of two, no term twice in a fit
	std::vector<GlmTermsFit> fits((size_t)n_fit);
	struct Product { int a, b; size_t fit; int term; };        // a <= b
	std::vector<Product> products;
	for (int t = 0; t < n_fits; t++) {
		GlmTermsFit &f = fits[(size_t)t];
		int key[GLMT_TERMS][2];
		for (int j = 0; j < GLMT_TERMS; j++) {
			const int a = terms[((size_t)t * GLMT_TERMS + j) * 2], b = terms[((size_t)t * GLMT_TERMS + j) * 2 + 1];
			if (a < -1 || a >= h->rows || b < -1 || b >= h->rows)
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_terms: fit %d term %d names rows (%d, %d), outside the handle's %d", t, j, a,
					b, h->rows);
			if (a < 0 && b >= 0)
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_terms: fit %d term %d has row_a = -1 with row_b = %d", t, j, b);
			key[j][0] = b < 0 ? a : std::min(a, b);
			key[j][1] = b < 0 ? -1 : std::max(a, b);
			for (int i = 0; i < j; i++)
				if (a >= 0 && key[i][0] == key[j][0] && key[i][1] == key[j][1])
					return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_glm_terms: fit %d names the term (%d, %d) twice", t, a, b);
			f.term[j][0] = a;
			f.term[j][1] = b;
			if (b >= 0) products.push_back(Product{key[j][0], key[j][1], (size_t)t, j});
		}
	}
	if (int rc = call.check_values()) return rc;
	HIP_TRY(hipSetDevice(h->device));

	// the terms' column sums: a row's from the row sums, a product's from the Gram of its rows'
	// blocks -- integers, so "nobody carries both" is decided exactly
	std::vector<int32_t> psum(products.size());
	{
		std::vector<size_t> order(products.size());
		for (size_t i = 0; i < order.size(); i++) order[i] = i;
		auto block = [&](size_t i) { return std::make_pair(products[i].a / kGramBlock, products[i].b / kGramBlock); };
		std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return block(x) < block(y); });
		std::vector<int32_t> C;
		for (size_t at = 0; at < order.size();) {
			// of the block only the rows between the lowest and the highest that its products name, each way
			const auto blk = block(order[at]);
			int a0 = h->rows, a1 = -1, b0 = h->rows, b1 = -1;
			for (size_t e = at; e < order.size() && block(order[e]) == blk; e++) {
				const Product &pr = products[order[e]];
				a0 = std::min(a0, pr.a); a1 = std::max(a1, pr.a);
				b0 = std::min(b0, pr.b); b1 = std::max(b1, pr.b);
			}
			const int na = a1 - a0 + 1, nb = b1 - b0 + 1;
			C.resize((size_t)na * nb);
			if (int rc = rows_gram(h, a0, na, b0, nb, C.data())) return rc;
			for (; at < order.size() && block(order[at]) == blk; at++) {
				const Product &pr = products[order[at]];
				psum[order[at]] = C[(size_t)(pr.a - a0) * nb + (pr.b - b0)];
			}
		}
	}
	const std::vector<int32_t> &r = h->h_row_sum;
	for (size_t i = 0; i < products.size(); i++)
		if (psum[i] == 0) fits[products[i].fit].term[products[i].term][0] = -2;      // (marked; cleared below)
	for (int t = 0; t < n_fits; t++) {
		GlmTermsFit &f = fits[(size_t)t];
		int left = 0, out = 0;
		for (int j = 0; j < GLMT_TERMS; j++) {
			int *tm = f.term[j];
			if (tm[0] == -1) continue;
			if (tm[0] == -2 || (tm[1] < 0 && r[(size_t)tm[0]] == 0)) { tm[0] = tm[1] = -1; out++; }
			else left++;
		}
		f.fitted = left > 0;
		f.flags0 = left > 0 ? (out ? GLM_FLAG_ALIASED : 0) : GLM_FLAG_RANK;
	}
	fits[(size_t)n_fits] = GlmTermsFit{{{-1, -1}, {-1, -1}, {-1, -1}}, 1, 0};

	return call.run(GLM_SLOTS, fits.data(), sizeof(GlmTermsFit), n_fit,
		[&](const double *d_cov, const double *d_w) {
			hipLaunchKernelGGL(k_glm_image_terms, dim3((unsigned)(((size_t)kp * GLM_SLOTS + 255) / 256)), dim3(256), 0, h->st, d_cov, d_w, n, q,
				kp, h->glm_img.as<double>(), h->glm_wt.as<double>());
		},
		[&](const GlmOut &O) {
			hipLaunchKernelGGL(k_glm_fit_terms, dim3(n_fit), dim3(GLM_WAVES * 64), 0, h->st, h->glm_img.as<double>(), h->glm_wt.as<double>(),
				h->y.as<int8_t>(), h->feat.as<int8_t>(), h->glm_fits.as<GlmTermsFit>(), n, kp, q, maxit, epsilon, O.coef, O.se, O.dev, O.it,
				O.fl, O.df);
		});
}

} // extern "C"

// ---- hlaAssocQuant (kernels: hibag_k_quant.h) ---------------------------------------------------
// A quantitative trait on the tests of an association handle.  hibag_hip_assoc_quant_new orthonormalises the basis (the
// constant and the covariates) and takes the residual trait on the host, uploads both, and has the device sum the classes,
// project the feature rows on the basis and run the observed trait -- permutation 0, the identity -- through the kernels of
// the permutations.  hibag_hip_assoc_quant_permute then works in panels of permutations: rows (k_quant_perm), residual panel
// and rr (k_quant_project), one FP64 Gram features x residuals (k_quant_gram), one pass over it (k_quant_stat).  The handle
// borrows the association handle: its feature rows, its stream, its one-host-thread rule.

struct hibag_hip_quant {
	hibag_hip_assoc *h = nullptr;                // borrowed; outlives this handle
	int nb = 0;                                  // basis rows: the constant and the covariates
	double ybar = 0, h_rr = 0, gram_ms = 0;
	DevBuf basis, yt, yc, tests, stat_obs;       // double [nb][kp], [kp], [kp]; QuantTest [n_test]; double [n_test]
	DevBuf perm, panel, rr, gram;                // per-call panel: int32 [pp][kp], double [pp / 16][kp / 4][64], [pp], [rows][pp]
	PermOut out;                                 // per permutation call
	std::vector<int64_t> h_cnt;                  // [n_test][3]
	std::vector<double> h_S1, h_S2, h_proj, h_g, h_stat; // [n_test][3] twice, [rows][nb], [rows], [n_test]
	std::vector<int32_t> h_flags;                // [n_test]
	std::vector<hipEvent_t> ev;                  // pairs around the Gram launches of the last permutation call

	~hibag_hip_quant()
	{
		if (!h) return;
		(void)hipSetDevice(h->device);
		if (h->st) (void)hipStreamSynchronize(h->st);
		for (DevBuf *b : {&basis, &yt, &yc, &tests, &stat_obs, &perm, &panel, &rr, &gram}) b->release();
		out.release();
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
	}
};

namespace {

constexpr size_t kQuantPanelBytes = (size_t)256 << 20;   // default size of a panel's residual operand

int quant_panel_perms(const hibag_hip_quant *q, int64_t n)
{
	return panel_perms("HIBAG_QUANT_PANEL_PERMS", kQuantPanelBytes, sizeof(double) * (size_t)q->h->kp, QUANT_TILE, true, n);
}

int quant_reserve_panel(hibag_hip_quant *q, int pp)
{
	const hibag_hip_assoc *h = q->h;
	if (q->perm.reserve(sizeof(int32_t) * (size_t)pp * h->kp) || q->panel.reserve(sizeof(double) * (size_t)pp * h->kp) ||
		q->rr.reserve(sizeof(double) * (size_t)pp) || q->gram.reserve(sizeof(double) * (size_t)h->rows * pp))
		return HIBAG_HIP_ENOMEM;
	return 0;
}

// permutations p0 .. p0 + n_lab - 1 (n_lab <= the reserved panel) through the four kernels; the Gram has row stride ldc
int quant_enqueue_panel(hibag_hip_quant *q, uint64_t seed, uint64_t p0, int n_lab, size_t ldc, double *stat_out, double *max_out,
	const double *stat_obs, unsigned long long *count, hipEvent_t e0, hipEvent_t e1)
{
	hibag_hip_assoc *h = q->h;
	const int n = h->D.n, kp = h->kp, tiles = (n_lab + QUANT_TILE - 1) / QUANT_TILE;
	hipLaunchKernelGGL(k_quant_perm, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, n, kp, seed, p0, n_lab, q->perm.as<int32_t>());
	hipLaunchKernelGGL(k_quant_project, dim3(tiles), dim3(256), 0, h->st, q->perm.as<int32_t>(), kp, n_lab, n, kp, q->yt.as<double>(),
		q->basis.as<double>(), q->nb, q->panel.as<double>(), q->rr.as<double>());
	if (e0) HIP_TRY(hipEventRecord(e0, h->st));
	hipLaunchKernelGGL(k_quant_gram, dim3(tiles, (h->rows + QUANT_TILE - 1) / QUANT_TILE), dim3(QUANT_GRAM_WAVES * 64), 0, h->st,
		h->feat.as<int8_t>(), h->rows, kp, q->panel.as<double>(), q->gram.as<double>(), ldc);
	if (e1) HIP_TRY(hipEventRecord(e1, h->st));
	hipLaunchKernelGGL(k_quant_stat, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, q->gram.as<double>(), ldc, q->rr.as<double>(), n_lab,
		q->tests.as<QuantTest>(), h->D.n_test, stat_out, max_out, stat_obs, count);
	HIP_TRY(hipGetLastError());
	return 0;
}

// the basis: the constant, then the covariates, orthonormalised by modified Gram-Schmidt applied twice -- under the inner
// product sum_i (w_i a_i) b_i where `w` is given (hlaAssocScore), else the plain one.  Returns the column that is in the span
// of the earlier ones, or -1.
int quant_orthonormalise(const double *covar, int n, int nb, std::vector<double> &Q, const double *w = nullptr)
{
	Q.assign((size_t)nb * n, 0.0);
	std::vector<double> v((size_t)n);
	for (int k = 0; k < nb; k++) {
		double zz = 0.0;
		for (int i = 0; i < n; i++) {
			v[i] = k == 0 ? 1.0 : covar[(size_t)(k - 1) * n + i];
			zz += w ? (w[i] * v[i]) * v[i] : v[i] * v[i];
		}
		for (int pass = 0; pass < 2; pass++)
			for (int j = 0; j < k; j++) {
				const double *qj = &Q[(size_t)j * n];
				double c = 0.0;
				for (int i = 0; i < n; i++) c += w ? (w[i] * qj[i]) * v[i] : qj[i] * v[i];
				for (int i = 0; i < n; i++) v[i] -= c * qj[i];
			}
		double ss = 0.0;
		for (int i = 0; i < n; i++) ss += w ? (w[i] * v[i]) * v[i] : v[i] * v[i];
		const double s = sqrt(ss);
		if (!(s > 1e-9 * sqrt(zz))) return k;
		for (int i = 0; i < n; i++) Q[(size_t)k * n + i] = v[i] / s;
	}
	return -1;
}

// the tests' constants from the class counts and the projections
void quant_tests(const hibag_hip_quant *q, std::vector<QuantTest> &tests, std::vector<int32_t> &flags)
{
	const hibag_hip_assoc *h = q->h;
	const int T = h->D.n_test, nb = q->nb;
	const int64_t n = h->D.n;
	const double nan = std::nan("");
	auto sum_sq = [&](int row) {
		double a = 0.0;
		for (int k = 0; k < nb; k++) a += q->h_proj[(size_t)row * nb + k] * q->h_proj[(size_t)row * nb + k];
		return a;
	};
	tests.assign((size_t)T, QuantTest{-1, -1, nan, nan, nan, nan, nan});
	flags.assign((size_t)T, QUANT_FLAG_RANK);
	for (int t = 0; t < T; t++) {
		const int64_t *c = &q->h_cnt[(size_t)t * 3];
		QuantTest &qt = tests[(size_t)t];
		int row = t;
		double xx;
		if (h->D.model == ASSOC_GENOTYPE) {
			if ((c[1] == 0 && c[2] == 0) || c[0] == 0) continue;
			if (c[1] > 0 && c[2] > 0) {
				const double xx1 = (double)c[1], xx2 = (double)c[2];
				const double a11 = xx1 - sum_sq(2 * t), a22 = xx2 - sum_sq(2 * t + 1);
				double a = 0.0;
				for (int k = 0; k < nb; k++) a += q->h_proj[(size_t)(2 * t) * nb + k] * q->h_proj[(size_t)(2 * t + 1) * nb + k];
				const double a12 = -a;
				if (!(a11 > 1e-11 * xx1) || !(a22 > 1e-11 * xx2)) continue;
				const double det = a11 * a22 - a12 * a12;
				if (!(det > 1e-11 * (a11 * a22))) continue;
				qt = QuantTest{2 * t, 2 * t + 1, (double)(n - nb - 2), a11, a22, a12, det};
				flags[(size_t)t] = 0;
				continue;
			}
			row = c[1] > 0 ? 2 * t : 2 * t + 1;
			xx = (double)(c[1] + c[2]);
		} else {
			if (c[0] == n || c[1] == n || c[2] == n) continue;
			xx = (double)(c[1] + 4 * c[2]);
		}
		const double sxx = xx - sum_sq(row);
		if (!(sxx > 1e-11 * xx)) continue;
		qt = QuantTest{row, -1, (double)(n - nb - 1), sxx, nan, nan, nan};
		flags[(size_t)t] = 0;
	}
}

// what hibag_hip_assoc_quant_new does on the device
int quant_build(hibag_hip_quant *q, const std::vector<double> &Q, const std::vector<double> &yt, const std::vector<double> &yc)
{
	hibag_hip_assoc *h = q->h;
	const int n = h->D.n, kp = h->kp, T = h->D.n_test, rows = h->rows, nb = q->nb;
	HIP_TRY(hipSetDevice(h->device));
	TempBuf d_cls, d_proj;                       // int64 [T][3] and double [T][3] twice; double [rows][nb]
	if (q->basis.reserve(sizeof(double) * (size_t)nb * kp) || q->yt.reserve(sizeof(double) * (size_t)kp) ||
		q->yc.reserve(sizeof(double) * (size_t)kp) || q->tests.reserve(sizeof(QuantTest) * (size_t)T) ||
		q->stat_obs.reserve(sizeof(double) * (size_t)T) || d_cls.reserve((size_t)T * 3 * (sizeof(long long) + 2 * sizeof(double))) ||
		d_proj.reserve(sizeof(double) * (size_t)rows * nb) || quant_reserve_panel(q, QUANT_TILE))
		return HIBAG_HIP_ENOMEM;
	std::vector<double> img((size_t)(nb + 2) * kp, 0.0);      // the padded rows: basis, residual trait, centred trait
	for (int k = 0; k < nb; k++) std::copy(&Q[(size_t)k * n], &Q[(size_t)k * n] + n, &img[(size_t)k * kp]);
	std::copy(yt.begin(), yt.end(), &img[(size_t)nb * kp]);
	std::copy(yc.begin(), yc.end(), &img[(size_t)(nb + 1) * kp]);
	q->h_cnt.resize((size_t)T * 3); q->h_S1.resize((size_t)T * 3); q->h_S2.resize((size_t)T * 3);
	q->h_proj.resize((size_t)rows * nb); q->h_g.resize((size_t)rows); q->h_stat.resize((size_t)T);
	std::vector<QuantTest> tests;
	return enqueued(h->st, [&]() -> int {
		HIP_TRY(hipMemcpyAsync(q->basis.p, img.data(), sizeof(double) * (size_t)nb * kp, hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(q->yt.p, &img[(size_t)nb * kp], sizeof(double) * (size_t)kp, hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(q->yc.p, &img[(size_t)(nb + 1) * kp], sizeof(double) * (size_t)kp, hipMemcpyHostToDevice, h->st));
		long long *d_cnt = d_cls.as<long long>();
		double *d_S1 = (double *)(d_cnt + (size_t)T * 3), *d_S2 = d_S1 + (size_t)T * 3;
		hipLaunchKernelGGL(k_quant_classes, dim3(T), dim3(256), 0, h->st, h->feat.as<int8_t>(), kp, n, h->D.model == ASSOC_GENOTYPE ? 1 : 0,
			q->yc.as<double>(), d_cnt, d_S1, d_S2);
		hipLaunchKernelGGL(k_quant_proj, dim3(rows), dim3(256), 0, h->st, h->feat.as<int8_t>(), kp, n, q->basis.as<double>(), nb,
			d_proj.as<double>());
		HIP_TRY(hipGetLastError());
		static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as they are");
		HIP_TRY(hipMemcpyAsync(q->h_cnt.data(), d_cnt, sizeof(int64_t) * (size_t)T * 3, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(q->h_S1.data(), d_S1, sizeof(double) * (size_t)T * 3, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(q->h_S2.data(), d_S2, sizeof(double) * (size_t)T * 3, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(q->h_proj.data(), d_proj.p, sizeof(double) * (size_t)rows * nb, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		quant_tests(q, tests, q->h_flags);
		HIP_TRY(hipMemcpyAsync(q->tests.p, tests.data(), sizeof(QuantTest) * (size_t)T, hipMemcpyHostToDevice, h->st));
		// the observed trait: permutation 0, a panel of its own
		if (int e = quant_enqueue_panel(q, 0, 0, 1, QUANT_TILE, q->stat_obs.as<double>(), nullptr, nullptr, nullptr, nullptr, nullptr)) return e;
		HIP_TRY(hipMemcpy2DAsync(q->h_g.data(), sizeof(double), q->gram.p, sizeof(double) * QUANT_TILE, sizeof(double), (size_t)rows,
			hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(&q->h_rr, q->rr.p, sizeof(double), hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(q->h_stat.data(), q->stat_obs.p, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	});
}

} // namespace

extern "C" {

hibag_hip_quant *hibag_hip_assoc_quant_new(hibag_hip_assoc *h, const double *y, const double *covar, int n_covar)
{
	if (!h || !y) { hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: null handle or y"); return nullptr; }
	if (n_covar < 0 || n_covar > HIBAG_HIP_GLM_MAX_COVAR || (n_covar > 0 && !covar)) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: %d covariates; 0 .. %d, with covar", n_covar, HIBAG_HIP_GLM_MAX_COVAR);
		return nullptr;
	}
	static_assert(QUANT_MAX_BASIS == HIBAG_HIP_GLM_MAX_COVAR + 1, "the constant and the covariates");
	const int n = h->D.n, nb = n_covar + 1;
	for (int i = 0; i < n; i++)
		if (!std::isfinite(y[i])) { hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: y of kept sample %d is not finite", i); return nullptr; }
	for (size_t i = 0; i < (size_t)n_covar * n; i++)
		if (!std::isfinite(covar[i])) {
			hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: covariate %zu of kept sample %zu is not finite", i / n, i % n);
			return nullptr;
		}
	const int d = h->D.model == ASSOC_GENOTYPE ? 2 : 1;
	if (n - nb - d < 1) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: %d kept samples leave %d residual degrees of freedom with %d covariates; "
			"at least 1", n, n - nb - d, n_covar);
		return nullptr;
	}
	std::vector<double> Q;
	const int bad = quant_orthonormalise(covar, n, nb, Q);
	if (bad >= 0) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_new: the covariates are collinear (column %d lies in the span of the constant "
			"and the columns before it)", bad - 1);
		return nullptr;
	}
	// the residual trait and the centred trait
	std::vector<double> yt(y, y + n), yc((size_t)n);
	for (int k = 0; k < nb; k++) {
		const double *qk = &Q[(size_t)k * n];
		double c = 0.0;
		for (int i = 0; i < n; i++) c += qk[i] * yt[i];
		for (int i = 0; i < n; i++) yt[i] -= c * qk[i];
	}
	double sum = 0.0;
	for (int i = 0; i < n; i++) sum += y[i];
	hibag_hip_quant *q = new (std::nothrow) hibag_hip_quant;
	if (!q) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	q->h = h;
	q->nb = nb;
	q->ybar = sum / (double)n;
	for (int i = 0; i < n; i++) yc[i] = y[i] - q->ybar;
	if (quant_build(q, Q, yt, yc) != 0) { delete q; return nullptr; }
	return q;
}

void hibag_hip_assoc_quant_free(hibag_hip_quant *q) { delete q; }

int hibag_hip_assoc_quant_classes(hibag_hip_quant *q, int64_t *cnt, double *S1, double *S2, double *ybar)
{
	if (!q || !cnt || !S1 || !S2 || !ybar) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_classes: null argument");
	std::copy(q->h_cnt.begin(), q->h_cnt.end(), cnt);
	std::copy(q->h_S1.begin(), q->h_S1.end(), S1);
	std::copy(q->h_S2.begin(), q->h_S2.end(), S2);
	*ybar = q->ybar;
	return 0;
}

int hibag_hip_assoc_quant_observed(hibag_hip_quant *q, double *proj, double *g, double *rr, double *stat, int32_t *flags)
{
	if (!q || !proj || !g || !rr || !stat || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_observed: null argument");
	std::copy(q->h_proj.begin(), q->h_proj.end(), proj);
	std::copy(q->h_g.begin(), q->h_g.end(), g);
	*rr = q->h_rr;
	std::copy(q->h_stat.begin(), q->h_stat.end(), stat);
	std::copy(q->h_flags.begin(), q->h_flags.end(), flags);
	return 0;
}

int hibag_hip_assoc_quant_permute(hibag_hip_quant *q, uint64_t seed, uint64_t perm0, int64_t n_perm, double *max_stat, int64_t *count_point)
{
	if (!q || n_perm < 0 || !count_point || (n_perm > 0 && !max_stat))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_permute: null argument or n_perm < 0");
	if (int rc = check_perm_range("hibag_hip_assoc_quant_permute", "trait", perm0, (uint64_t)n_perm)) return rc;
	hibag_hip_assoc *h = q->h;
	const int T = h->D.n_test;
	std::fill(count_point, count_point + T, (int64_t)0);
	q->gram_ms = 0;
	if (n_perm == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = quant_panel_perms(q, n_perm);
	const size_t n_panel = (size_t)((n_perm + pp - 1) / pp);
	if (quant_reserve_panel(q, pp) || q->out.reserve(n_perm, T)) return HIBAG_HIP_ENOMEM;
	while (q->ev.size() < 2 * n_panel) {
		hipEvent_t e;
		HIP_TRY(hipEventCreate(&e));
		q->ev.push_back(e);
	}
	int rc = q->out.run(h->st, T, n_perm, pp, max_stat, count_point, [&](int64_t done, int n_lab) -> int {
		const size_t k = (size_t)(done / pp);
		return quant_enqueue_panel(q, seed, perm0 + (uint64_t)done, n_lab, (size_t)pp, nullptr, q->out.max_stat.as<double>() + done,
			q->stat_obs.as<double>(), q->out.count.as<unsigned long long>(), q->ev[2 * k], q->ev[2 * k + 1]);
	});
	if (rc) return rc;
	for (size_t j = 0; j < n_panel; j++) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, q->ev[2 * j], q->ev[2 * j + 1]));
		q->gram_ms += ms;
	}
	return 0;
}

int hibag_hip_assoc_quant_perm_rows(hibag_hip_quant *q, uint64_t seed, uint64_t perm0, int n, int32_t *out)
{
	if (!q || n < 0 || (n > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_perm_rows: null argument or n < 0");
	if (int rc = check_perm_range("hibag_hip_assoc_quant_perm_rows", "trait", perm0, (uint64_t)n)) return rc;
	if (n == 0) return 0;
	hibag_hip_assoc *h = q->h;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = quant_panel_perms(q, n), kp = h->kp, ns = h->D.n;
	if (q->perm.reserve(sizeof(int32_t) * (size_t)pp * kp)) return HIBAG_HIP_ENOMEM;
	return download_panels(h->st, n, pp, q->perm.p, sizeof(int32_t) * (size_t)kp, sizeof(int32_t) * (size_t)ns, out,
		[&](int64_t done, int n_lab) -> int {
			hipLaunchKernelGGL(k_quant_perm, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, ns, kp, seed, perm0 + (uint64_t)done, n_lab,
				q->perm.as<int32_t>());
			HIP_TRY(hipGetLastError());
			return 0;
		});
}

int hibag_hip_assoc_quant_gram_ms(const hibag_hip_quant *q, double *ms)
{
	if (!q || !ms) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_quant_gram_ms: null argument");
	*ms = q->gram_ms;
	return 0;
}

} // extern "C"

// ---- hlaAssocScore (kernels: hibag_k_score.h) ----------------------------------------------------
// Score tests of a case / control trait under the base model y ~ covariates, on the tests or sets of rows of an association
// handle.  hibag_hip_assoc_score_new fits the base model once with the regression driver above, takes the residuals, the
// weights and the weighted basis on the host, uploads them and has the device project the feature rows.
// hibag_hip_assoc_score_sets installs the sets: the device sums their weighted Grams, the host factorises them and uploads
// the factors, and the observed residuals -- replicate 0, all signs +1 -- go through the kernels of the replicates.
// hibag_hip_assoc_score_resample then works in panels of replicates with the panel driver of the permutation entries: the
// residual panel from the signs (k_score_coef, k_score_project), the FP64 Gram (k_quant_gram, as it is), one pass over it (k_score_stat).
// hibag_hip_assoc_rscore_sets installs sets over real-valued rows of its own instead (hlaAssocHaplo, DESIGN.md section 30;
// kernels: hibag_k_rscore.h): the same steps with k_rscore_proj, k_rscore_setgram and, per panel, k_rscore_gram.

struct hibag_hip_score {
	hibag_hip_assoc *h = nullptr;                // borrowed; outlives this handle
	int nb = 0, n_sets = -1, n_df = 0;           // basis rows; the installed sets (-1: none yet); their distinct degrees of freedom
	double b_coef[GLM_SLOTS], b_se[GLM_SLOTS], b_dev = 0; // the base model's fit
	int32_t b_it = 0, b_fl = 0;
	double ms[3] = {0, 0, 0};                    // project, Gram, statistic of the last resampling call
	DevBuf basis, e, w;                          // double [nb][kp], [kp], [kp]
	DevBuf sets, rows, factor, stat_obs;         // ScoreSet [n_sets], int32 kept rows, double packed factors, double [n_sets]
	DevBuf panel, gram, part;                    // per-call panel: double [pp / 16][kp / 4][64], [rows][pp], [segments][13][ldp]
	DevBuf X;                                    // hibag_hip_assoc_rscore_sets: double [x_rows][kp], zero on the padding samples
	int x_rows = 0;
	bool real = false;                           // the installed sets are over X, not over the handle's int8 rows
	size_t ldp = 0;
	PermOut out;                                 // per resampling call
	std::vector<double> h_proj, h_g, h_stat;     // [rows][nb], [rows], [n_sets]
	std::vector<double> h_xproj;                 // [x_rows][nb]: the projections of X
	std::vector<int32_t> h_df, h_flags;          // [n_sets]
	std::vector<hipEvent_t> ev;                  // four per panel of the last resampling call

	~hibag_hip_score()
	{
		if (!h) return;
		(void)hipSetDevice(h->device);
		if (h->st) (void)hipStreamSynchronize(h->st);
		for (DevBuf *b : {&basis, &e, &w, &sets, &rows, &factor, &stat_obs, &panel, &gram, &part, &X}) b->release();
		out.release();
		for (hipEvent_t x : ev) (void)hipEventDestroy(x);
	}
};

namespace {

int score_panel_perms(const hibag_hip_score *s, int64_t n)
{
	return panel_perms("HIBAG_SCORE_PANEL_PERMS", kQuantPanelBytes, sizeof(double) * (size_t)s->h->kp, QUANT_TILE, true, n);
}

int score_reserve_panel(hibag_hip_score *s, int pp)
{
	const hibag_hip_assoc *h = s->h;
	const size_t ldp = ((size_t)pp + SCORE_BLOCK - 1) / SCORE_BLOCK * SCORE_BLOCK, n_seg = ((size_t)std::max(h->D.n, 1) + SCORE_SEG - 1) / SCORE_SEG;
	if (s->panel.reserve(sizeof(double) * (size_t)pp * h->kp) || s->gram.reserve(sizeof(double) * (size_t)std::max(h->rows, s->x_rows) * pp) ||
		s->part.reserve(sizeof(double) * n_seg * QUANT_MAX_BASIS * ldp))
		return HIBAG_HIP_ENOMEM;
	s->ldp = std::max(s->ldp, ldp);                          // (the row stride of what is reserved; it only grows)
	return 0;
}

// replicates p0 .. p0 + n_lab - 1 (n_lab <= the reserved panel) through the three kernels; the Gram has row stride ldc;
// ev: four events around them, or null
int score_enqueue_panel(hibag_hip_score *s, uint64_t seed, uint64_t p0, int n_lab, size_t ldc, double *stat_out, double *max_out,
	const double *stat_obs, unsigned long long *count, const hipEvent_t *ev)
{
	hibag_hip_assoc *h = s->h;
	const int n = h->D.n, kp = h->kp, tiles = (n_lab + QUANT_TILE - 1) / QUANT_TILE;
	if (ev) HIP_TRY(hipEventRecord(ev[0], h->st));
	const unsigned n_blk = (unsigned)((n_lab + SCORE_BLOCK - 1) / SCORE_BLOCK);
	hipLaunchKernelGGL(k_score_coef, dim3(n_blk, (n + SCORE_SEG - 1) / SCORE_SEG), dim3(SCORE_THREADS), 0, h->st, seed, p0, n_lab, n, kp,
		s->e.as<double>(), s->w.as<double>(), s->basis.as<double>(), s->nb, s->part.as<double>(), s->ldp);
	hipLaunchKernelGGL(k_score_project, dim3(n_blk, (kp + SCORE_SEG - 1) / SCORE_SEG), dim3(SCORE_THREADS), 0, h->st, seed, p0, n_lab, n, kp,
		s->e.as<double>(), s->w.as<double>(), s->basis.as<double>(), s->nb, s->part.as<double>(), s->ldp, s->panel.as<double>());
	if (ev) HIP_TRY(hipEventRecord(ev[1], h->st));
	if (s->real)
		hipLaunchKernelGGL(k_rscore_gram, dim3(tiles, (s->x_rows + QUANT_TILE - 1) / QUANT_TILE), dim3(QUANT_GRAM_WAVES * 64), 0, h->st,
			s->X.as<double>(), s->x_rows, kp, s->panel.as<double>(), s->gram.as<double>(), ldc);
	else
		hipLaunchKernelGGL(k_quant_gram, dim3(tiles, (h->rows + QUANT_TILE - 1) / QUANT_TILE), dim3(QUANT_GRAM_WAVES * 64), 0, h->st,
			h->feat.as<int8_t>(), h->rows, kp, s->panel.as<double>(), s->gram.as<double>(), ldc);
	if (ev) HIP_TRY(hipEventRecord(ev[2], h->st));
	hipLaunchKernelGGL(k_score_stat, dim3((n_lab + 63) / 64), dim3(64), 0, h->st, s->gram.as<double>(), ldc, n_lab, s->sets.as<ScoreSet>(),
		s->n_sets, s->rows.as<int32_t>(), s->factor.as<double>(), s->n_df, stat_out, max_out, stat_obs, count);
	if (ev) HIP_TRY(hipEventRecord(ev[3], h->st));
	HIP_TRY(hipGetLastError());
	return 0;
}

} // namespace

extern "C" {

hibag_hip_score *hibag_hip_assoc_score_new(hibag_hip_assoc *h, const double *covar, int n_covar, const double *weight, int maxit,
	double epsilon)
{
	if (!h) { hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_new: null handle"); return nullptr; }
	static_assert(QUANT_MAX_BASIS == HIBAG_HIP_GLM_MAX_COVAR + 1, "the constant and the covariates");
	static_assert(SCORE_MAX_ROWS == HIBAG_HIP_SCORE_MAX_ROWS && SCORE_MAX_ROWS <= SCORE_SET_LD, "the header's set size");
	hibag_hip_score *s = new (std::nothrow) hibag_hip_score;
	if (!s) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	s->h = h;
	s->nb = n_covar + 1;
	const int n = h->D.n, kp = h->kp, q = n_covar, nb = n_covar + 1, rows = h->rows;

	// the base model: the d = 0 fit of section 23, one fit with the kernels of hibag_hip_assoc_glm
	const GlmCall call{"hibag_hip_assoc_score_new", h, covar, n_covar, weight, maxit, epsilon, s->b_coef, s->b_se, &s->b_dev, &s->b_it, &s->b_fl,
		nullptr};
	const GlmFit base{-1, -1};
	if (call.check_control(HIBAG_HIP_GLM_MAX_COVAR) || call.check_values() ||
		call.run(GLM_SLOTS, &base, sizeof(GlmFit), 1,
			[&](const double *d_cov, const double *d_w) {
				hipLaunchKernelGGL(k_glm_image, dim3((unsigned)(((size_t)kp * GLM_SLOTS + 255) / 256)), dim3(256), 0, h->st, d_cov, d_w, n, q, kp,
					h->glm_img.as<double>(), h->glm_wt.as<double>());
			},
			[&](const GlmOut &O) {
				hipLaunchKernelGGL(k_glm_fit, dim3(1), dim3(GLM_WAVES * 64), 0, h->st, h->glm_img.as<double>(), h->glm_wt.as<double>(),
					h->y.as<int8_t>(), h->feat.as<int8_t>(), h->glm_fits.as<GlmFit>(), n, kp, q, maxit, epsilon, O.coef, O.se, O.dev, O.it, O.fl);
			})) {
		delete s;
		return nullptr;
	}
	if (s->b_fl & GLM_FLAG_RANK) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_new: the covariates are collinear (the base model is rank-deficient)");
		delete s;
		return nullptr;
	}

	// residuals and weights from the base model's coefficients, in index order (section 28 item 2)
	std::vector<int8_t> y((size_t)kp);
	std::vector<double> img((size_t)(nb + 2) * kp, 0.0), Q;     // the padded rows: basis, e, w
	double *e = &img[(size_t)nb * kp], *w = e + kp;
	auto fail = [&]() { delete s; return (hibag_hip_score *)nullptr; };
	if (hipSetDevice(h->device) != hipSuccess || enqueued(h->st, [&]() -> int {
			HIP_TRY(hipMemcpyAsync(y.data(), h->y.p, (size_t)kp, hipMemcpyDeviceToHost, h->st));
			HIP_TRY(hipStreamSynchronize(h->st));
			return 0;
		})) return fail();
	for (int i = 0; i < n; i++) {
		double eta = s->b_coef[0];
		for (int k = 0; k < q; k++) eta += covar[(size_t)k * n + i] * s->b_coef[GLM_COV0 + k];
		double t = exp(eta);
		if (eta < -30.0) t = GLM_EPS;
		if (eta > 30.0) t = 1.0 / GLM_EPS;
		const double mu = t / (1.0 + t), v = mu * (1.0 - mu), wt = weight ? weight[i] : 1.0;
		w[i] = wt * v;
		e[i] = wt * ((y[i] ? 1.0 : 0.0) - mu);
	}
	const int bad = quant_orthonormalise(covar, n, nb, Q, w);
	if (bad >= 0) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_new: the covariates are collinear (column %d lies in the span of the constant "
			"and the columns before it under the base model's weights)", bad - 1);
		return fail();
	}
	for (int k = 0; k < nb; k++) std::copy(&Q[(size_t)k * n], &Q[(size_t)k * n] + n, &img[(size_t)k * kp]);

	TempBuf d_proj;
	s->h_proj.resize((size_t)rows * nb);
	if (s->basis.reserve(sizeof(double) * (size_t)nb * kp) || s->e.reserve(sizeof(double) * (size_t)kp) || s->w.reserve(sizeof(double) * (size_t)kp) ||
		d_proj.reserve(sizeof(double) * (size_t)rows * nb) || score_reserve_panel(s, QUANT_TILE))
		return fail();
	if (enqueued(h->st, [&]() -> int {
			HIP_TRY(hipMemcpyAsync(s->basis.p, img.data(), sizeof(double) * (size_t)nb * kp, hipMemcpyHostToDevice, h->st));
			HIP_TRY(hipMemcpyAsync(s->e.p, e, sizeof(double) * (size_t)kp, hipMemcpyHostToDevice, h->st));
			HIP_TRY(hipMemcpyAsync(s->w.p, w, sizeof(double) * (size_t)kp, hipMemcpyHostToDevice, h->st));
			hipLaunchKernelGGL(k_score_proj, dim3(rows), dim3(256), 0, h->st, h->feat.as<int8_t>(), kp, n, s->w.as<double>(), s->basis.as<double>(),
				nb, d_proj.as<double>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(s->h_proj.data(), d_proj.p, sizeof(double) * (size_t)rows * nb, hipMemcpyDeviceToHost, h->st));
			HIP_TRY(hipStreamSynchronize(h->st));
			return 0;
		})) return fail();
	return s;
}

void hibag_hip_assoc_score_free(hibag_hip_score *s) { delete s; }

int hibag_hip_assoc_score_base(hibag_hip_score *s, double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags)
{
	if (!s || !coef || !se || !deviance || !iterations || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_base: null argument");
	std::copy(s->b_coef, s->b_coef + GLM_SLOTS, coef);
	std::copy(s->b_se, s->b_se + GLM_SLOTS, se);
	*deviance = s->b_dev; *iterations = s->b_it; *flags = s->b_fl;
	return 0;
}

// hibag_hip_assoc_score_sets (X null: the sets name the handle's int8 rows) and hibag_hip_assoc_rscore_sets (X float64
// [m][n_kept]: the sets name its rows)
static int score_install(hibag_hip_score *s, const char *me, const double *X, int m_real, const int32_t *set_start, const int32_t *set_rows,
	int n_sets, double *proj, double *S, int32_t *kept)
{
	if (!s || !proj || (n_sets > 0 && (!S || !kept))) return hibag_fail(HIBAG_HIP_EINVAL, "%s: null argument", me);
	if (n_sets < 0 || n_sets > kMaxTests || !set_start || set_start[0] != 0)
		return hibag_fail(HIBAG_HIP_EINVAL, "%s: need 0 <= n_sets <= %d and set_start with set_start[0] = 0", me, kMaxTests);
	hibag_hip_assoc *h = s->h;
	const bool real = X != nullptr;
	const int n_rows = real ? m_real : h->rows;
	std::vector<int> seen((size_t)n_rows, -1);
	for (int t = 0; t < n_sets; t++) {
		const int m = set_start[t + 1] - set_start[t];
		if (m < 0) return hibag_fail(HIBAG_HIP_EINVAL, "%s: set_start is not monotone at set %d", me, t);
		if (m > SCORE_MAX_ROWS) return hibag_fail(HIBAG_HIP_EINVAL, "%s: set %d has %d rows; at most %d", me, t, m, SCORE_MAX_ROWS);
		if (m > 0 && !set_rows) return hibag_fail(HIBAG_HIP_EINVAL, "%s: set_rows is null", me);
		for (int j = 0; j < m; j++) {
			const int r = set_rows[set_start[t] + j];
			if (r < 0 || r >= n_rows)
				return hibag_fail(HIBAG_HIP_EINVAL, "%s: set %d names row %d, outside the handle's %d", me, t, r, n_rows);
			if (seen[(size_t)r] == t) return hibag_fail(HIBAG_HIP_EINVAL, "%s: set %d names row %d twice", me, t, r);
			seen[(size_t)r] = t;
		}
	}
	const int nb = s->nb, kp = h->kp, total = set_start[n_sets], ns = std::max(n_sets, 1);
	HIP_TRY(hipSetDevice(h->device));
	if (real) {
		// the rows, zero-padded to [m][kp], and their projections on the basis
		const int n = h->D.n;
		std::vector<double> img((size_t)m_real * kp, 0.0);
		for (int r = 0; r < m_real; r++)
			for (int i = 0; i < n; i++) {
				const double v = X[(size_t)r * n + i];
				if (!std::isfinite(v)) return hibag_fail(HIBAG_HIP_EINVAL, "%s: row %d has the value %g at sample %d; finite values", me, r, v, i);
				img[(size_t)r * kp + i] = v;
			}
		TempBuf d_proj;
		if (s->X.reserve(sizeof(double) * img.size()) || d_proj.reserve(sizeof(double) * (size_t)m_real * nb)) return HIBAG_HIP_ENOMEM;
		s->h_xproj.resize((size_t)m_real * nb);
		if (int rc = enqueued(h->st, [&]() -> int {
				HIP_TRY(hipMemcpyAsync(s->X.p, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice, h->st));
				hipLaunchKernelGGL(k_rscore_proj, dim3(m_real), dim3(256), 0, h->st, s->X.as<double>(), kp, n, s->w.as<double>(), s->basis.as<double>(),
					nb, d_proj.as<double>());
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipMemcpyAsync(s->h_xproj.data(), d_proj.p, sizeof(double) * (size_t)m_real * nb, hipMemcpyDeviceToHost, h->st));
				HIP_TRY(hipStreamSynchronize(h->st));
				return 0;
			})) { s->n_sets = -1; return rc; }
		s->x_rows = m_real;
	}
	s->real = real;
	s->n_sets = -1;                                            // (until the new sets stand)
	const std::vector<double> &h_proj = real ? s->h_xproj : s->h_proj;
	TempBuf d_start, d_rows, d_S;
	std::vector<double> S32((size_t)ns * SCORE_SET_LD * SCORE_SET_LD);
	if (d_start.reserve(sizeof(int32_t) * (size_t)(n_sets + 1)) || d_rows.reserve(sizeof(int32_t) * (size_t)std::max(total, 1)) ||
		d_S.reserve(sizeof(double) * S32.size()) || s->stat_obs.reserve(sizeof(double) * (size_t)ns))
		return HIBAG_HIP_ENOMEM;
	if (n_sets > 0)
		if (int rc = enqueued(h->st, [&]() -> int {
				HIP_TRY(hipMemcpyAsync(d_start.p, set_start, sizeof(int32_t) * (size_t)(n_sets + 1), hipMemcpyHostToDevice, h->st));
				if (total) HIP_TRY(hipMemcpyAsync(d_rows.p, set_rows, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, h->st));
				if (real)
					hipLaunchKernelGGL(k_rscore_setgram, dim3(n_sets), dim3(SCORE_GRAM_WAVES * 64), 0, h->st, s->X.as<double>(), kp, s->w.as<double>(),
						d_start.as<int32_t>(), d_rows.as<int32_t>(), d_S.as<double>());
				else
					hipLaunchKernelGGL(k_score_setgram, dim3(n_sets), dim3(SCORE_GRAM_WAVES * 64), 0, h->st, h->feat.as<int8_t>(), kp, s->w.as<double>(),
						d_start.as<int32_t>(), d_rows.as<int32_t>(), d_S.as<double>());
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipMemcpyAsync(S32.data(), d_S.p, sizeof(double) * (size_t)n_sets * SCORE_SET_LD * SCORE_SET_LD, hipMemcpyDeviceToHost, h->st));
				HIP_TRY(hipStreamSynchronize(h->st));
				return 0;
			})) return rc;

	// per set: V = S - P P', its Cholesky factor in column order with aliased columns dropped (section 28 item 4)
	std::vector<ScoreSet> sets((size_t)ns, ScoreSet{0, 0, 0, 0});
	std::vector<int32_t> krows;
	std::vector<double> factor;
	s->h_df.assign((size_t)n_sets, 0);
	s->h_flags.assign((size_t)n_sets, 0);
	const std::vector<int32_t> &rsum = h->h_row_sum;
	const bool base_failed = (s->b_fl & GLM_FLAG_MAXIT) != 0;
	size_t s_at = 0;
	for (int t = 0; t < n_sets; t++) {
		const int m = set_start[t + 1] - set_start[t];
		const int32_t *rw = set_rows + set_start[t];
		const double *St = &S32[(size_t)t * SCORE_SET_LD * SCORE_SET_LD];
		double V[SCORE_MAX_ROWS][SCORE_MAX_ROWS], L[SCORE_MAX_ROWS][SCORE_MAX_ROWS];
		for (int a = 0; a < m; a++)
			for (int b = 0; b <= a; b++) {
				const double sab = St[a * SCORE_SET_LD + b];
				double pp = 0.0;
				for (int k = 0; k < nb; k++) pp += h_proj[(size_t)rw[a] * nb + k] * h_proj[(size_t)rw[b] * nb + k];
				V[a][b] = V[b][a] = sab - pp;
				S[s_at + (size_t)a * m + b] = S[s_at + (size_t)b * m + a] = sab;
			}
		s_at += (size_t)m * m;
		int keep[SCORE_MAX_ROWS], d = 0, dropped = 0;             // the kept columns' positions in the set, in order
		int32_t mask = 0;
		for (int j = 0; j < m; j++) {
			// nobody carries it: decided from the integer row sum, for real rows from S_jj == 0
			if (real ? St[j * SCORE_SET_LD + j] == 0.0 : rsum[(size_t)rw[j]] == 0) { dropped++; continue; }
			double piv = V[j][j];
			for (int c = 0; c < d; c++) piv -= L[j][c] * L[j][c];
			if (!(piv > 1e-11 * St[j * SCORE_SET_LD + j])) { dropped++; continue; }
			L[j][d] = sqrt(piv);
			for (int i = j + 1; i < m; i++) {
				double v = V[i][j];
				for (int c = 0; c < d; c++) v -= L[i][c] * L[j][c];
				L[i][d] = v / L[j][d];
			}
			keep[d++] = j;
			mask |= (int32_t)1 << j;
		}
		kept[t] = mask;
		int32_t fl = d == 0 ? GLM_FLAG_RANK : dropped ? GLM_FLAG_ALIASED : 0;
		if (base_failed) { fl |= GLM_FLAG_MAXIT; d = 0; }
		s->h_flags[(size_t)t] = fl;
		s->h_df[(size_t)t] = d;
		sets[(size_t)t] = ScoreSet{(int)krows.size(), d, 0, (int)factor.size()};
		for (int a = 0; a < d; a++) {
			krows.push_back(rw[keep[a]]);
			for (int b = 0; b <= a; b++) factor.push_back(L[keep[a]][b]);
		}
	}
	// the slots of the distinct degrees of freedom, ascending
	int slot_of[SCORE_MAX_ROWS + 1];
	std::fill(slot_of, slot_of + SCORE_MAX_ROWS + 1, -1);
	for (int t = 0; t < n_sets; t++) slot_of[s->h_df[(size_t)t]] = 0;
	s->n_df = 0;
	for (int d = 1; d <= SCORE_MAX_ROWS; d++)
		if (slot_of[d] == 0) slot_of[d] = s->n_df++;
	for (int t = 0; t < n_sets; t++) sets[(size_t)t].slot = std::max(slot_of[sets[(size_t)t].d], 0);
	std::copy(h_proj.begin(), h_proj.end(), proj);

	s->n_sets = n_sets;
	s->h_g.assign((size_t)n_rows, 0.0);
	s->h_stat.assign((size_t)n_sets, std::nan(""));
	if (s->sets.reserve(sizeof(ScoreSet) * (size_t)ns) || s->rows.reserve(sizeof(int32_t) * std::max<size_t>(krows.size(), 1)) ||
		s->factor.reserve(sizeof(double) * std::max<size_t>(factor.size(), 1)) || score_reserve_panel(s, QUANT_TILE))
		return HIBAG_HIP_ENOMEM;
	return enqueued(h->st, [&]() -> int {
		HIP_TRY(hipMemcpyAsync(s->sets.p, sets.data(), sizeof(ScoreSet) * (size_t)ns, hipMemcpyHostToDevice, h->st));
		if (!krows.empty()) HIP_TRY(hipMemcpyAsync(s->rows.p, krows.data(), sizeof(int32_t) * krows.size(), hipMemcpyHostToDevice, h->st));
		if (!factor.empty()) HIP_TRY(hipMemcpyAsync(s->factor.p, factor.data(), sizeof(double) * factor.size(), hipMemcpyHostToDevice, h->st));
		// the observed residuals: replicate 0, a panel of its own
		if (int e = score_enqueue_panel(s, 0, 0, 1, QUANT_TILE, s->stat_obs.as<double>(), nullptr, nullptr, nullptr, nullptr)) return e;
		HIP_TRY(hipMemcpy2DAsync(s->h_g.data(), sizeof(double), s->gram.p, sizeof(double) * QUANT_TILE, sizeof(double), (size_t)n_rows,
			hipMemcpyDeviceToHost, h->st));
		if (n_sets) HIP_TRY(hipMemcpyAsync(s->h_stat.data(), s->stat_obs.p, sizeof(double) * (size_t)n_sets, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	});
}

int hibag_hip_assoc_score_sets(hibag_hip_score *s, const int32_t *set_start, const int32_t *set_rows, int n_sets, double *proj, double *S,
	int32_t *kept)
{
	return score_install(s, "hibag_hip_assoc_score_sets", nullptr, 0, set_start, set_rows, n_sets, proj, S, kept);
}

int hibag_hip_assoc_rscore_sets(hibag_hip_score *s, const double *rows, int m, const int32_t *set_start, const int32_t *set_rows,
	int n_sets, double *proj, double *S, int32_t *kept)
{
	const char *me = "hibag_hip_assoc_rscore_sets";
	if (!s || !rows) return hibag_fail(HIBAG_HIP_EINVAL, "%s: null argument", me);
	if (m < 1 || m > kMaxTests) return hibag_fail(HIBAG_HIP_EINVAL, "%s: m = %d; 1 .. %d rows", me, m, kMaxTests);
	return score_install(s, me, rows, m, set_start, set_rows, n_sets, proj, S, kept);
}

int hibag_hip_assoc_score_observed(hibag_hip_score *s, double *g, double *stat, int32_t *df, int32_t *flags)
{
	if (!s || !g || !stat || !df || !flags) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_observed: null argument");
	if (s->n_sets < 0) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_observed: no sets are installed (hibag_hip_assoc_score_sets)");
	std::copy(s->h_g.begin(), s->h_g.end(), g);
	std::copy(s->h_stat.begin(), s->h_stat.end(), stat);
	std::copy(s->h_df.begin(), s->h_df.end(), df);
	std::copy(s->h_flags.begin(), s->h_flags.end(), flags);
	return 0;
}

int hibag_hip_assoc_score_n_df(const hibag_hip_score *s)
{
	if (!s || s->n_sets < 0) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_n_df: null handle or no sets installed");
	return s->n_df;
}

int hibag_hip_assoc_score_resample(hibag_hip_score *s, uint64_t seed, uint64_t p0, int64_t n_perm, double *max_stat, int64_t *count_point)
{
	if (!s || n_perm < 0 || !count_point || (n_perm > 0 && !max_stat))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_resample: null argument or n_perm < 0");
	if (s->n_sets < 0) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_resample: no sets are installed (hibag_hip_assoc_score_sets)");
	if (int rc = check_perm_range("hibag_hip_assoc_score_resample", "residuals", p0, (uint64_t)n_perm)) return rc;
	hibag_hip_assoc *h = s->h;
	const int T = s->n_sets, n_df = s->n_df;
	std::fill(count_point, count_point + T, (int64_t)0);
	s->ms[0] = s->ms[1] = s->ms[2] = 0;
	if (n_perm == 0 || T == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = score_panel_perms(s, n_perm);
	const size_t n_panel = (size_t)((n_perm + pp - 1) / pp);
	if (score_reserve_panel(s, pp) || s->out.reserve(n_perm, T, n_df)) return HIBAG_HIP_ENOMEM;
	while (s->ev.size() < 4 * n_panel) {
		hipEvent_t x;
		HIP_TRY(hipEventCreate(&x));
		s->ev.push_back(x);
	}
	int rc = s->out.run(h->st, T, n_perm, pp, max_stat, count_point, [&](int64_t done, int n_lab) -> int {
		return score_enqueue_panel(s, seed, p0 + (uint64_t)done, n_lab, (size_t)pp, nullptr, s->out.max_stat.as<double>() + (size_t)done * n_df,
			s->stat_obs.as<double>(), s->out.count.as<unsigned long long>(), &s->ev[4 * (size_t)(done / pp)]);
	}, n_df);
	if (rc) return rc;
	for (size_t j = 0; j < n_panel; j++)
		for (int k = 0; k < 3; k++) {
			float ms = 0;
			HIP_TRY(hipEventElapsedTime(&ms, s->ev[4 * j + k], s->ev[4 * j + k + 1]));
			s->ms[k] += ms;
		}
	return 0;
}

int hibag_hip_assoc_score_signs(hibag_hip_score *s, uint64_t seed, uint64_t p0, int n, int8_t *out)
{
	if (!s || n < 0 || (n > 0 && !out)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_signs: null argument or n < 0");
	if (int rc = check_perm_range("hibag_hip_assoc_score_signs", "residuals", p0, (uint64_t)n)) return rc;
	hibag_hip_assoc *h = s->h;
	if (n == 0 || h->D.n == 0) return 0;
	HIP_TRY(hipSetDevice(h->device));
	const int pp = score_panel_perms(s, n), kp = h->kp, ns = h->D.n;
	if (s->panel.reserve(sizeof(double) * (size_t)pp * kp)) return HIBAG_HIP_ENOMEM;      // (the panel's room, as int8 [pp][kp])
	return download_panels(h->st, n, pp, s->panel.p, (size_t)kp, (size_t)ns, out, [&](int64_t done, int n_lab) -> int {
		hipLaunchKernelGGL(k_score_signs, dim3((ns + 255) / 256), dim3(256), 0, h->st, ns, (size_t)kp, seed, p0 + (uint64_t)done, n_lab,
			s->panel.as<int8_t>());
		HIP_TRY(hipGetLastError());
		return 0;
	});
}

int hibag_hip_assoc_score_ms(const hibag_hip_score *s, double *ms)
{
	if (!s || !ms) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_assoc_score_ms: null argument");
	std::copy(s->ms, s->ms + 3, ms);
	return 0;
}

} // extern "C"
