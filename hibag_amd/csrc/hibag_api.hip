// hibag_api.hip -- the small shared part of libhibag_hip.so's host side: the calling thread's error state and device
// selection, the kernel-target switch (hlaSetKernelTarget), and the TypeGPUExtProc-compatible plugin table.  The model is
// hibag_model.hip, the batch driver hibag_predict.hip (hibag_internal.h lists what they share).
//
// There is no CPU fallback here: every compute entry runs the HIP kernels or fails with an error code.

#include "hibag_internal.h"
#include "hibag_em.h"

namespace {

thread_local std::string g_last_error;
thread_local int g_device = 0;

} // namespace

// for the other translation units of the library
int hibag_selected_device() { return g_device; }        // the calling thread's hibag_hip_set_device() choice

int hibag_fail(int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_last_error = buf;
	return code;
}

// ===========================================================================
// C ABI: library-wide entries

extern "C" {

int hibag_hip_abi_version(void) { return HIBAG_HIP_ABI_VERSION; }

const char *hibag_hip_last_error(void) { return g_last_error.c_str(); }

int hibag_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return n;
}

int hibag_hip_set_device(int device)
{
	const int n = hibag_hip_device_count();
	if (device < 0 || device >= n)
		return hibag_fail(HIBAG_HIP_ENODEV, "HIP device %d not available (%d visible)", device, n);
	g_device = device;
	return 0;
}

int hibag_hip_get_device(void) { return g_device; }

int hibag_hip_set_kernel_target(const char *target, char *info, size_t info_len)
{
	if (!target || strcmp(target, "hip") != 0)
		return hibag_fail(HIBAG_HIP_EINVAL, "this library implements the kernel target \"hip\" only (got \"%s\")",
			target ? target : "(null)");
	const int n = hibag_hip_device_count();
	if (n <= 0 || g_device >= n) return hibag_fail(HIBAG_HIP_ENODEV, "no HIP device available");
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, g_device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return hibag_fail(HIBAG_HIP_ENODEV, "device %d is %s; the kernels are built for gfx950 only", g_device, prop.gcnArchName);
	if (info && info_len)
		snprintf(info, info_len, "HIP, %s, %s, %d CUs", prop.gcnArchName, prop.name, prop.multiProcessorCount);
	return 0;
}

} // extern "C"

// ===========================================================================
// HIBAG plugin table: layout-compatible with HLA_LIB::TypeGPUExtProc
// (inst/include/LibHLA_ext.h:358-388).  The host calls predict_init once per
// PredictHLA (src/LibHLA.cpp:2498-2523), predict_avg_prob once per sample with
// nthread = 1 (:2433-2441) and predict_done from a destructor (:2525-2531).
// A failure cannot be returned through these void signatures; like a C++
// plugin would, it throws `const char *`, which the host's CORE_CATCH turns
// into an R error (src/HIBAG.cpp:41-60).

namespace {

// The predict entries live in hibag_sample.hip (a per-sample form of the path: lane = allele-pair cell), the build entries in
// hibag_build.hip.  One model and one training state per process at a time, like the reference's single staging buffer.
const PluginTable g_plugin_table = {
	hibag_build_init, hibag_build_done, hibag_build_set_bootstrap, hibag_build_haplomatch,
	hibag_build_set_haplo_geno, hibag_build_acc_oob, hibag_build_acc_ib,
	hibag_sample_init, hibag_sample_done, hibag_sample_avg_prob,
};

} // namespace

extern "C" const void *hibag_hip_gpu_ext_proc(void) { return &g_plugin_table; }

// predict_avg_prob calls since the last predict_init whose full-width launch could not get all its workgroups resident (the
// device is shared) and that were therefore repeated on a single workgroup; 0 on a device the process has to itself.
extern "C" long long hibag_hip_plugin_degraded_calls(void) { return hibag_sample_degraded_calls(); }

// The loop an unmodified HIBAG runs around predict_avg_prob (src/LibHLA.cpp:2362-2411 with :2433-2441), in C like the host's: for
// every sample one call through the table with its packed genotypes and weights, then BestGuessEnsemble's scan of the posterior
// (:1549-1566: first strict maximum in cell order, -1 when nothing is positive).  Measurement and tests: the time of the n_samp
// calls as a compiled host sees them (no interpreter between the calls), and the per-sample best cell to check them with.
extern "C" int hibag_hip_test_time_avg_prob(const void *geno, const double *weight, int n_samp, int n_classifier, int n_cell,
	int32_t *best_cell, double *matching, double *seconds)
{
	if (!geno || !weight || n_samp < 0 || n_classifier < 0 || n_cell <= 0) return hibag_fail(HIBAG_HIP_EINVAL, "bad arguments");
	std::vector<double> prob;
	try { prob.assign((size_t)n_cell, 0.0); } catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
	const PluginGenotype *g = (const PluginGenotype *)geno;
	double match = 0;
	const auto t0 = std::chrono::steady_clock::now();
	try {
		for (int i = 0; i < n_samp; i++) {
			g_plugin_table.predict_avg_prob(g + (size_t)i * n_classifier, weight + (size_t)i * n_classifier, prob.data(), &match);
			double best = 0;
			int cell = -1;
			for (int p = 0; p < n_cell; p++)
				if (best < prob[p]) { best = prob[p]; cell = p; }
			if (best_cell) best_cell[i] = cell;
			if (matching) matching[i] = match;
		}
	} catch (const char *msg) {
		return hibag_fail(HIBAG_HIP_ENODEV, "%s", msg);
	}
	if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return 0;
}

// The batched scoring of one growth step (hibag_build_eval_batch, hibag_plugin.h) is C++-only and otherwise reached only from
// inside the training driver, where a step's width, candidates and route are whatever the greedy search makes them.  This
// entry runs one such step on the caller's own arrays, between an init and a done of its own: build_init, build_set_bootstrap,
// the cohort's genotype matrix if one is given (the candidates then travel as rows of it: the device-resident route; without
// it the host packs each candidate's column: the host-packed route), the scoring, build_done.  It REPLACES the calling
// thread's build state.  Tests only.
extern "C" int hibag_hip_test_build_eval_batch(int n_hla, int n_sample, const int *boot, const void *base_geno, int n_snp,
	int n_cand, const int *n_haplo, const void *haplo, const int32_t *columns, const int32_t *geno_snp_major, int n_matrix_snp,
	const int *cand_snp, int acc_floor, int *acc_oob, double *loss_ib)
{
	if (n_hla <= 0 || n_hla > 32767 || n_sample <= 0 || n_snp < 1 || n_snp > 128 || n_cand <= 0)
		return hibag_fail(HIBAG_HIP_EINVAL, "test_build_eval_batch: invalid sizes");
	if (!boot || !base_geno || !n_haplo || !haplo || !acc_oob || !loss_ib)
		return hibag_fail(HIBAG_HIP_EINVAL, "test_build_eval_batch: a required array is NULL");
	if (geno_snp_major ? (n_matrix_snp <= 0 || !cand_snp) : !columns)
		return hibag_fail(HIBAG_HIP_EINVAL, "test_build_eval_batch: a genotype matrix needs cand_snp, no matrix needs columns");
	try {
		std::vector<HibagBuildCandidate> cand((size_t)n_cand);
		const PluginHaplotype *hp = (const PluginHaplotype *)haplo;
		for (int c = 0; c < n_cand; c++) {
			if (n_haplo[c] < 0) return hibag_fail(HIBAG_HIP_EINVAL, "test_build_eval_batch: negative haplotype count");
			if (geno_snp_major && (cand_snp[c] < 0 || cand_snp[c] >= n_matrix_snp))
				return hibag_fail(HIBAG_HIP_EINVAL, "test_build_eval_batch: cand_snp[%d] = %d is no row of the matrix", c, cand_snp[c]);
			cand[c].haplo = hp;
			cand[c].n_haplo = n_haplo[c];
			cand[c].column = columns ? columns + (size_t)c * n_sample : nullptr;
			cand[c].snp = geno_snp_major ? cand_snp[c] : -1;
			hp += n_haplo[c];
		}
		struct Scope { ~Scope() { hibag_build_done(); } } scope;       // (also when one of the calls below throws)
		hibag_build_init(n_hla, n_sample);
		hibag_build_set_bootstrap(boot);
		if (geno_snp_major) hibag_build_set_genotypes(geno_snp_major, n_matrix_snp);
		hibag_build_eval_batch((const PluginGenotype *)base_geno, n_snp, cand.data(), n_cand, acc_floor, acc_oob, loss_ib);
	} catch (const char *msg) {
		return hibag_fail(HIBAG_HIP_ENODEV, "%s", msg);
	} catch (const std::bad_alloc &) {
		return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
	}
	return 0;
}

// The device EM fit of one growth step (hibag_em_fit_batch, hibag_em.h) is C++-only too and otherwise reached only through the
// greedy search, which shows the winner of every step and nothing else.  This entry runs it once on the caller's own arrays:
// the transposed lists come from the driver's own builder (hibag_em_transpose), the layout from the driver's own rule.
// Everything the kernel indexes with is checked BEFORE the device is touched, so no argument can make the kernel read or
// write out of bounds; the calling thread's EM arena is released on every way out.  Tests only.
extern "C" int hibag_hip_test_em_layout(int n_ib, int n_pair, int n_hap) { return hibag_em_layout(n_ib, n_pair, n_hap); }

extern "C" int hibag_hip_test_em_fit(int n_ib, int n_pair, int n_hap, int n_samp_total, const int *h1, const int *h2, const int *off,
	const int *boot, const double *cur_freq, int n_cand, const int8_t *geno, const double *afreq, double *out_freq, int *status,
	int *iters, int *layout)
{
	if (n_ib <= 0 || n_pair <= 0 || n_hap <= 0 || n_samp_total <= 0 || n_cand <= 0 || n_cand > 65535)
		return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: invalid sizes");
	if (n_hap & 1) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: n_hap = %d is odd (the list is a doubled one)", n_hap);
	if (!h1 || !h2 || !off || !boot || !cur_freq || !geno || !afreq || !out_freq || !status)
		return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: a required array is NULL");
	if (!hibag_em_fits(n_ib, n_pair, n_hap))
		return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: a step of %d samples, %d pairs, %d haplotypes does not fit the kernel", n_ib, n_pair, n_hap);
	if (off[0] != 0 || off[n_ib] != n_pair) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: off must start at 0 and end at n_pair");
	for (int i = 0; i < n_ib; i++) {
		if (off[i + 1] < off[i]) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: off decreases at sample %d", i);
		if (boot[i] < 1) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: boot[%d] = %d, an in-bag sample's count is at least 1", i, boot[i]);
	}
	for (int j = 0; j < n_pair; j++)
		if (h1[j] < 0 || h1[j] >= n_hap || h2[j] < 0 || h2[j] >= n_hap)
			return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: pair %d = (%d, %d) is outside the %d haplotypes", j, h1[j], h2[j], n_hap);
	for (size_t k = 0; k < (size_t)n_cand * n_ib; k++)
		if (geno[k] < 0 || geno[k] > 3) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: genotype %d at candidate %d, sample %d (0, 1, 2 or 3 = missing)",
			(int)geno[k], (int)(k / n_ib), (int)(k % n_ib));
	for (int c = 0; c < n_cand; c++)
		if (!(afreq[c] > 0 && afreq[c] < 1)) return hibag_fail(HIBAG_HIP_EINVAL, "test_em_fit: afreq[%d] = %g is not inside (0, 1)", c, afreq[c]);
	try {
		std::vector<int> hoff, hent, at;
		hibag_em_transpose(n_pair, n_hap, h1, h2, hoff, hent, at);
		std::vector<const int8_t *> gp((size_t)n_cand);
		for (int c = 0; c < n_cand; c++) gp[c] = geno + (size_t)c * n_ib;
		if (hipSetDevice(hibag_selected_device()) != hipSuccess)
			return hibag_fail(HIBAG_HIP_ENODEV, "test_em_fit: hipSetDevice(%d) failed", hibag_selected_device());
		struct Scope { ~Scope() { hibag_em_release(); } } scope;          // (also when the call below throws)
		const HibagEmPairs P{n_ib, n_pair, n_hap, n_samp_total, h1, h2, off, boot, hoff.data(), hent.data(), cur_freq};
		hibag_em_fit_batch(P, gp.data(), afreq, n_cand, out_freq, status, iters, layout);
	} catch (const char *msg) {
		return hibag_fail(HIBAG_HIP_ENODEV, "%s", msg);
	} catch (const std::bad_alloc &) {
		return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
	}
	return 0;
}
