// hibag_ld.hip -- host side of hlaGenoLD and hlaLDMatrix (R/HIBAG.R:1399-1446, :1453-1541): the device-resident genotype
// matrix behind `hibag_hip_ld_geno` and the entries of include/hibag_hip.h that use it.  Kernels: hibag_k_ld.h.
//
// The genotypes are packed once (k_ld_pack) into int8 codes [n_snp][kp] on the device that the creating thread had
// selected; every entry then builds the operands of its Gram from them on the device.  A handle is used by one host
// thread at a time.

#include "hibag_internal.h"
#include "hibag_k_ld.h"

using hibag_detail::DevBuf;
using hibag_detail::PinBuf;

struct hibag_hip_ld_geno {
	int device = 0;
	int n_snp = 0, n_samp = 0, kp = 0;
	hipStream_t st = nullptr, copy = nullptr;    // Gram kernels / panel copies of hlaLDMatrix
	DevBuf codes, n_valid, sum;
	DevBuf work[4];                              // per-call scratch: operands, indices, flags, sums
	DevBuf panel[2];
	PinBuf stage[2];
	double gram_ms = 0;                          // event time of the Gram kernels of the last hibag_hip_ld_matrix

	~hibag_hip_ld_geno()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamSynchronize(st);
		if (copy) (void)hipStreamSynchronize(copy);
		codes.release(); n_valid.release(); sum.release();
		for (auto &w : work) w.release();
		for (auto &p : panel) p.release();
		for (auto &p : stage) p.release();
		if (st) (void)hipStreamDestroy(st);
		if (copy) (void)hipStreamDestroy(copy);
	}
};

namespace {

constexpr int kMaxSamples = 1 << 24;             // every integer of the r^2 formula is exact in double below this
constexpr size_t kPanelBytes = (size_t)64 << 20; // default size of one r^2 panel (device buffer and pinned staging buffer)

size_t pad_to(size_t x, size_t m) { return (x + m - 1) / m * m; }

// rows of one hlaLDMatrix panel: HIBAG_LD_PANEL_ROWS (read per call), else about kPanelBytes of output in whole tiles
int panel_rows(int n_idx)
{
	const char *e = getenv("HIBAG_LD_PANEL_ROWS");
	long rows = e && *e ? strtol(e, nullptr, 10) : 0;
	if (rows <= 0) {
		rows = (long)(kPanelBytes / (sizeof(double) * (size_t)n_idx)) / HIBAG_LD_TILE * HIBAG_LD_TILE;
		rows = std::max<long>(rows, HIBAG_LD_TILE);
	}
	return (int)std::min<long>(rows, n_idx);
}

// memcpy on several host threads: the destination is usually fresh memory (numpy's empty result), whose first-touch
// page faults, not the bytes, bound a single-threaded copy
void copy_parallel(void *dst, const void *src, size_t bytes)
{
	constexpr size_t kChunk = (size_t)8 << 20;
	const int n = (int)std::min<size_t>(16, std::max<size_t>(1, bytes / kChunk));
	if (n == 1) { memcpy(dst, src, bytes); return; }
	std::vector<std::thread> th;
	const size_t per = (bytes + n - 1) / n;
	for (int i = 1; i < n; i++) {
		const size_t o = per * i;
		if (o < bytes) th.emplace_back(memcpy, (char *)dst + o, (const char *)src + o, std::min(per, bytes - o));
	}
	memcpy(dst, src, std::min(per, bytes));
	for (auto &t : th) t.join();
}

void launch_gram(bool raw, const int8_t *A, int ma, const int8_t *B, int mb, int kp, const LdGramOut &O, hipStream_t st)
{
	const dim3 grid((mb + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE, (ma + HIBAG_LD_TILE - 1) / HIBAG_LD_TILE);
	if (raw) hipLaunchKernelGGL(k_ld_gram<1>, grid, dim3(256), 0, st, A, ma, B, mb, kp, O);
	else hipLaunchKernelGGL(k_ld_gram<0>, grid, dim3(256), 0, st, A, ma, B, mb, kp, O);
}

} // namespace

extern "C" {

hibag_hip_ld_geno *hibag_hip_ld_geno_new(const int32_t *geno, int n_snp, int n_samp, int snp_major)
{
	if (!geno || n_snp <= 0 || n_samp <= 0) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_geno_new: need genotypes and n_snp, n_samp > 0 (got %d x %d)", n_snp, n_samp);
		return nullptr;
	}
	if (n_samp > kMaxSamples) {
		hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_geno_new: %d samples; at most 2^24 keep the LD sums exact in double", n_samp);
		return nullptr;
	}
	hibag_hip_ld_geno *g = new (std::nothrow) hibag_hip_ld_geno;
	if (!g) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	g->device = hibag_selected_device();
	g->n_snp = n_snp;
	g->n_samp = n_samp;
	g->kp = (int)pad_to((size_t)n_samp, HIBAG_LD_KPAD);
	const size_t cells = (size_t)n_snp * n_samp;
	auto body = [&]() -> int {
		HIP_TRY(hipSetDevice(g->device));
		HIP_TRY(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking));
		HIP_TRY(hipStreamCreateWithFlags(&g->copy, hipStreamNonBlocking));
		if (g->codes.reserve((size_t)n_snp * g->kp) || g->n_valid.reserve(sizeof(int32_t) * n_snp) ||
			g->sum.reserve(sizeof(int32_t) * n_snp) || g->work[0].reserve(sizeof(int32_t) * cells))
			return HIBAG_HIP_ENOMEM;
		HIP_TRY(hipMemcpyAsync(g->work[0].p, geno, sizeof(int32_t) * cells, hipMemcpyHostToDevice, g->st));
		HIP_TRY(hipMemsetAsync(g->n_valid.p, 0, sizeof(int32_t) * n_snp, g->st));
		HIP_TRY(hipMemsetAsync(g->sum.p, 0, sizeof(int32_t) * n_snp, g->st));
		const dim3 grid(g->kp / 64, (n_snp + 63) / 64);
		hipLaunchKernelGGL(k_ld_pack, grid, dim3(256), 0, g->st, g->work[0].as<int32_t>(), n_snp, n_samp, snp_major ? 1 : 0,
			g->kp, g->codes.as<int8_t>(), g->n_valid.as<int32_t>(), g->sum.as<int32_t>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(g->st));
		g->work[0].release();                    // the int32 copy is not needed any more
		return 0;
	};
	if (body() != 0) { delete g; return nullptr; }
	return g;
}

void hibag_hip_ld_geno_free(hibag_hip_ld_geno *g) { delete g; }

int hibag_hip_ld_snp_counts(hibag_hip_ld_geno *g, int32_t *n_valid, int64_t *sum)
{
	if (!g || !n_valid || !sum) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_snp_counts: null argument");
	HIP_TRY(hipSetDevice(g->device));
	std::vector<int32_t> s((size_t)g->n_snp);
	HIP_TRY(hipMemcpyAsync(n_valid, g->n_valid.p, sizeof(int32_t) * g->n_snp, hipMemcpyDeviceToHost, g->st));
	HIP_TRY(hipMemcpyAsync(s.data(), g->sum.p, sizeof(int32_t) * g->n_snp, hipMemcpyDeviceToHost, g->st));
	HIP_TRY(hipStreamSynchronize(g->st));
	for (int j = 0; j < g->n_snp; j++) sum[j] = s[j];
	return 0;
}

int hibag_hip_ld_matrix(hibag_hip_ld_geno *g, const int32_t *snp_idx, int n_idx, double *r2, int *n_complete)
{
	if (!g || n_idx < 0 || (n_idx > 0 && (!snp_idx || !r2)))
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_matrix: bad arguments");
	for (int i = 0; i < n_idx; i++)
		if (snp_idx[i] < 0 || snp_idx[i] >= g->n_snp)
			return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_matrix: snp_idx[%d] = %d is outside [0, %d)", i, snp_idx[i], g->n_snp);
	HIP_TRY(hipSetDevice(g->device));
	g->gram_ms = 0;
	if (n_idx == 0) { if (n_complete) *n_complete = g->n_samp; return 0; }

	// samples complete over the SNPs (R's use = "na.or.complete"), compacted on the host from the device's flags
	if (g->work[0].reserve(sizeof(int32_t) * n_idx) || g->work[1].reserve((size_t)g->n_samp)) return HIBAG_HIP_ENOMEM;
	HIP_TRY(hipMemcpyAsync(g->work[0].p, snp_idx, sizeof(int32_t) * n_idx, hipMemcpyHostToDevice, g->st));
	hipLaunchKernelGGL(k_ld_complete, dim3((g->n_samp + 255) / 256), dim3(256), 0, g->st, g->codes.as<int8_t>(), g->kp,
		g->n_samp, g->work[0].as<int32_t>(), n_idx, g->work[1].as<uint8_t>());
	HIP_TRY(hipGetLastError());
	std::vector<uint8_t> flag((size_t)g->n_samp);
	HIP_TRY(hipMemcpyAsync(flag.data(), g->work[1].p, flag.size(), hipMemcpyDeviceToHost, g->st));
	HIP_TRY(hipStreamSynchronize(g->st));
	std::vector<int32_t> samp;
	for (int s = 0; s < g->n_samp; s++)
		if (flag[s]) samp.push_back(s);
	const int n_c = (int)samp.size();
	if (n_complete) *n_complete = n_c;
	const size_t nn = (size_t)n_idx * n_idx;
	if (n_c < 2) {                               // cov.c: fewer than two complete cases -> every entry NA
		for (size_t e = 0; e < nn; e++) r2[e] = std::nan("");
		return 0;
	}

	// the operand: the SNPs' rows restricted to the complete samples, with Sx and Sxx
	const int kc = (int)pad_to((size_t)n_c, HIBAG_LD_KPAD);
	if (g->work[1].reserve(sizeof(int32_t) * n_c) || g->work[2].reserve((size_t)n_idx * kc) ||
		g->work[3].reserve(2 * sizeof(int32_t) * n_idx))
		return HIBAG_HIP_ENOMEM;
	int32_t *d_sx = g->work[3].as<int32_t>(), *d_sxx = d_sx + n_idx;
	int8_t *xc = g->work[2].as<int8_t>();
	HIP_TRY(hipMemcpyAsync(g->work[1].p, samp.data(), sizeof(int32_t) * n_c, hipMemcpyHostToDevice, g->st));
	hipLaunchKernelGGL(k_ld_compact, dim3(n_idx), dim3(256), 0, g->st, g->codes.as<int8_t>(), g->kp, g->work[0].as<int32_t>(),
		g->work[1].as<int32_t>(), n_c, kc, xc, d_sx, d_sxx);
	HIP_TRY(hipGetLastError());

	// row panels: Gram of panel p on `st` into panel[p & 1], its copy to stage[p & 1] on `copy`, the host's copy of the
	// stage into r2 two panels later -- the next panel's Gram overlaps this one's transfer
	const int rows = panel_rows(n_idx);
	const int n_panel = (n_idx + rows - 1) / rows;
	const size_t pbytes = sizeof(double) * (size_t)rows * n_idx;
	for (int b = 0; b < std::min(n_panel, 2); b++)
		if (g->panel[b].reserve(pbytes) || g->stage[b].reserve(pbytes)) return HIBAG_HIP_ENOMEM;
	const int n_ev = 2 * n_panel;
	std::vector<hipEvent_t> ev((size_t)n_ev + 4, nullptr);   // [2p], [2p + 1]: the Gram of panel p; then gram-done, copied x 2
	int rc = 0;
	auto body = [&]() -> int {
		for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
		hipEvent_t *done = &ev[n_ev], *copied = &ev[n_ev + 2];
		auto drain = [&](int p) -> int {            // panel p's bytes are on the host: move them into r2
			const int b = p & 1;
			HIP_TRY(hipEventSynchronize(copied[b]));
			const size_t r0 = (size_t)p * rows, nr = std::min<size_t>(rows, n_idx - r0);
			copy_parallel(r2 + r0 * n_idx, g->stage[b].p, sizeof(double) * nr * n_idx);
			return 0;
		};
		for (int p = 0; p < n_panel; p++) {
			const int b = p & 1;
			if (p >= 2) { int e = drain(p - 2); if (e) return e; }
			const int r0 = p * rows, nr = std::min(rows, n_idx - r0);
			LdGramOut O;
			O.out64 = g->panel[b].as<double>();
			O.row0 = r0;
			O.n = n_c;
			O.sx = d_sx;
			O.sxx = d_sxx;
			O.ld = (size_t)n_idx;
			HIP_TRY(hipEventRecord(ev[2 * p], g->st));
			launch_gram(false, xc + (size_t)r0 * kc, nr, xc, n_idx, kc, O, g->st);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(ev[2 * p + 1], g->st));
			HIP_TRY(hipEventRecord(done[b], g->st));
			HIP_TRY(hipStreamWaitEvent(g->copy, done[b], 0));
			HIP_TRY(hipMemcpyAsync(g->stage[b].p, O.out64, sizeof(double) * (size_t)nr * n_idx, hipMemcpyDeviceToHost, g->copy));
			HIP_TRY(hipEventRecord(copied[b], g->copy));
			// the next Gram into this buffer (panel p + 2) starts after this copy: drain(p) waits on the host first
		}
		for (int p = std::max(0, n_panel - 2); p < n_panel; p++) { int e = drain(p); if (e) return e; }
		HIP_TRY(hipStreamSynchronize(g->st));
		for (int p = 0; p < n_panel; p++) {
			float ms = 0;
			HIP_TRY(hipEventElapsedTime(&ms, ev[2 * p], ev[2 * p + 1]));
			g->gram_ms += ms;
		}
		return 0;
	};
	rc = body();
	if (rc) { (void)hipStreamSynchronize(g->st); (void)hipStreamSynchronize(g->copy); }
	for (auto &e : ev)
		if (e) (void)hipEventDestroy(e);
	return rc;
}

int hibag_hip_ld_gram_ms(hibag_hip_ld_geno *g, double *ms)
{
	if (!g || !ms) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_gram_ms: null argument");
	*ms = g->gram_ms;
	return 0;
}

int hibag_hip_ld_hla(hibag_hip_ld_geno *g, const int32_t *allele1, const int32_t *allele2, int n_allele, double *ld,
	double *r2_or_null)
{
	if (!g || !allele1 || !allele2 || !ld || n_allele < 0)
		return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_hla: bad arguments");
	if (n_allele > 60000) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_hla: %d alleles", n_allele);
	for (int s = 0; s < g->n_samp; s++) {
		const int32_t x[2] = {allele1[s], allele2[s]};
		for (int32_t v : x)
			if (v != HIBAG_HIP_NA_INTEGER && (v < 0 || v >= n_allele))
				return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_ld_hla: sample %d has allele index %d, outside [0, %d) and not NA",
					s, v, n_allele);
	}
	if (n_allele == 0) {                         // no allele: mean(numeric(0)) for every SNP
		for (int j = 0; j < g->n_snp; j++) ld[j] = std::nan("");
		return 0;
	}
	HIP_TRY(hipSetDevice(g->device));
	const int ma = 3 * g->n_snp, mb = 2 * n_allele + 1;
	const size_t n_r2 = r2_or_null ? (size_t)g->n_snp * n_allele : 0;
	if (g->work[0].reserve((size_t)ma * g->kp) || g->work[1].reserve((size_t)mb * g->kp) ||
		g->work[2].reserve(2 * sizeof(int32_t) * g->n_samp) || g->work[3].reserve(sizeof(int32_t) * (size_t)ma * mb) ||
		g->panel[0].reserve(sizeof(double) * (g->n_snp + n_r2)))
		return HIBAG_HIP_ENOMEM;
	int32_t *d_a = g->work[2].as<int32_t>();
	HIP_TRY(hipMemcpyAsync(d_a, allele1, sizeof(int32_t) * g->n_samp, hipMemcpyHostToDevice, g->st));
	HIP_TRY(hipMemcpyAsync(d_a + g->n_samp, allele2, sizeof(int32_t) * g->n_samp, hipMemcpyHostToDevice, g->st));
	const size_t words = (size_t)g->n_snp * (g->kp / 4);
	hipLaunchKernelGGL(k_ld_hla_snp_operand, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, g->st, g->codes.as<int8_t>(),
		g->n_snp, g->kp, g->work[0].as<int8_t>());
	hipLaunchKernelGGL(k_ld_hla_allele_operand, dim3(g->kp / 256 + 1, mb), dim3(256), 0, g->st, d_a, d_a + g->n_samp, g->n_samp,
		n_allele, g->kp, g->work[1].as<int8_t>());
	LdGramOut O;
	O.out32 = g->work[3].as<int32_t>();
	O.ld = (size_t)mb;
	launch_gram(true, g->work[0].as<int8_t>(), ma, g->work[1].as<int8_t>(), mb, g->kp, O, g->st);
	double *d_ld = g->panel[0].as<double>(), *d_r2 = r2_or_null ? d_ld + g->n_snp : nullptr;
	hipLaunchKernelGGL(k_ld_hla_finish, dim3((g->n_snp + 255) / 256), dim3(256), 0, g->st, O.out32, g->n_snp, n_allele, d_ld, d_r2);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(ld, d_ld, sizeof(double) * g->n_snp, hipMemcpyDeviceToHost, g->st));
	if (r2_or_null) HIP_TRY(hipMemcpyAsync(r2_or_null, d_r2, sizeof(double) * n_r2, hipMemcpyDeviceToHost, g->st));
	HIP_TRY(hipStreamSynchronize(g->st));
	return 0;
}

} // extern "C"
