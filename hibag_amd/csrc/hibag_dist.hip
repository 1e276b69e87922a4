// hibag_dist.hip -- host side of hlaDistance (R/HIBAG.R:1545-1570 around HIBAG_Distance, src/HIBAG.cpp:1284-1332):
// hibag_hip_model_distance.  Kernels and the order they keep: hibag_k_dist.h.
//
// The haplotype table is the one hibag_hip_predict_oob reads (oob_hap_table: packed bits, frequencies, per-classifier
// offsets and allele starts); on a model that was never finalized this call builds it.  The classifiers go through in
// chunks whose per-classifier triangles (n_hla (n_hla + 1) / 2 doubles each) fit a fixed budget: per chunk the host lists
// the non-empty cells, stage 1 (k_dist_cells) fills the chunk's triangles, NaN where a cell is empty, and stage 2
// (k_dist_fold) carries R's fold on to the next chunk or, after the last, writes the symmetric result.

#include "hibag_internal.h"
#include "hibag_k_dist.h"

namespace hibag_detail {

// Stage-1 workspace per chunk; HIBAG_DIST_CHUNK (classifiers per chunk) overrides it (tests of the chunked fold).
static const size_t DIST_TRI_BUDGET = (size_t)512 << 20;

// The non-empty cells of classifiers [c0, c1): those with more than HIBAG_DIST_LANE_MAX pairs in `big`, roughly largest
// first (by bit length: a wave each, the long chains start first); the others in `small`, exactly largest first (64 to a
// wave, lanes of similar length).  Counting sorts: O(cells).
static void dist_cells(const hibag_hip_model *m, int c0, int c1, std::vector<HibagDistCell> &big, std::vector<HibagDistCell> &small)
{
	const int nh = m->n_hla;
	std::vector<std::vector<HibagDistCell>> bucket_big(64), bucket_small(HIBAG_DIST_LANE_MAX + 1);
	std::vector<int> cnt(nh), present;
	for (int c = c0; c < c1; c++) {
		std::fill(cnt.begin(), cnt.end(), 0);
		for (int h : m->cls[c].hla) cnt[h]++;
		present.clear();
		for (int a = 0; a < nh; a++) if (cnt[a]) present.push_back(a);
		for (size_t x = 0; x < present.size(); x++)
			for (size_t y = x; y < present.size(); y++) {
				const int a = present[x], b = present[y];
				const int64_t na = cnt[a], np = a == b ? na * (na + 1) / 2 : na * cnt[b];
				const HibagDistCell cell{c, a, b, 0};
				if (np <= HIBAG_DIST_LANE_MAX) bucket_small[np].push_back(cell);
				else {
					int bl = 0;
					while ((np >> bl) > 1) bl++;
					bucket_big[bl].push_back(cell);
				}
			}
	}
	big.clear(); small.clear();
	for (int bl = 63; bl >= 0; bl--) big.insert(big.end(), bucket_big[bl].begin(), bucket_big[bl].end());
	for (int np = HIBAG_DIST_LANE_MAX; np >= 1; np--) small.insert(small.end(), bucket_small[np].begin(), bucket_small[np].end());
}

static int dist_nomem(const hibag_hip_model *m, const char *what, size_t bytes)
{
	(void)hipGetLastError();
	return hibag_fail(HIBAG_HIP_ENOMEM, "hlaDistance: n_hla = %d needs %.3g GB of device memory for %s, which could not be allocated",
		m->n_hla, (double)bytes / 1e9, what);
}

int model_distance_locked(hibag_hip_model *m, double *out, double *out_each)
{
	const int C = (int)m->cls.size(), nh = m->n_hla;
	const int64_t n_tri = (int64_t)nh * (nh + 1) / 2;
	const size_t tri_bytes = (size_t)n_tri * sizeof(double);

	// after whatever is outstanding on the model (device-pointer entries chain through ws_done)
	if (m->ws_pending && m->ws_done) HIP_TRY(hipEventSynchronize(m->ws_done));
	if (int rc = oob_hap_table(m)) return rc;
	if (!m->dist_st) HIP_TRY(hipStreamCreateWithFlags(&m->dist_st, hipStreamNonBlocking));
	for (hipEvent_t &e : m->dist_ev) if (!e) HIP_TRY(hipEventCreate(&e));
	const hipStream_t st = m->dist_st;

	int cc = (int)std::max<size_t>(1, std::min<size_t>((size_t)C, DIST_TRI_BUDGET / tri_bytes));
	if (const char *e = getenv("HIBAG_DIST_CHUNK")) cc = std::max(1, std::min(C, atoi(e)));
	const int n_chunk = (C + cc - 1) / cc;
	if (m->dist_tri.reserve(tri_bytes * cc)) return dist_nomem(m, "the per-classifier triangles", tri_bytes * cc);
	if (n_chunk > 1) {
		if (m->dist_acc.reserve(tri_bytes)) return dist_nomem(m, "the running sums", tri_bytes);
		if (m->dist_num.reserve((size_t)n_tri * sizeof(int))) return dist_nomem(m, "the running counts", (size_t)n_tri * sizeof(int));
	}
	const size_t out_bytes = (size_t)nh * nh * sizeof(double);
	if (m->dist_out.reserve(out_bytes)) return dist_nomem(m, "the result", out_bytes);

	const char *d_base = m->oob_hap.as<char>();
	HibagDistTables T;
	T.bits = (const uint64_t *)d_base;
	T.freq = (const double *)(d_base + m->oob_freq_at);
	T.off = (const int *)(d_base + m->oob_off_at);
	T.start = (const int *)(d_base + m->oob_start_at);
	T.n_hla = nh;

	std::vector<HibagDistCell> big, small;
	std::vector<double> each;                    // one chunk's triangles on the host (out_each only)
	double ms_total = 0;
	for (int k = 0; k < n_chunk; k++) {
		const int c0 = k * cc, c1 = std::min(C, c0 + cc);
		dist_cells(m, c0, c1, big, small);
		if (big.size() + small.size() > (size_t)INT32_MAX / 2)
			return hibag_fail(HIBAG_HIP_EINVAL, "hlaDistance: %zu cells in classifiers %d..%d", big.size() + small.size(), c0, c1 - 1);
		const size_t cell_bytes = std::max<size_t>(1, big.size() + small.size()) * sizeof(HibagDistCell);
		if (m->dist_cells.reserve(cell_bytes)) return dist_nomem(m, "the cell list", cell_bytes);
		HibagDistCell *d_big = m->dist_cells.as<HibagDistCell>(), *d_small = d_big + big.size();
		if (!big.empty()) HIP_TRY(hipMemcpyAsync(d_big, big.data(), big.size() * sizeof(HibagDistCell), hipMemcpyHostToDevice, st));
		if (!small.empty()) HIP_TRY(hipMemcpyAsync(d_small, small.data(), small.size() * sizeof(HibagDistCell), hipMemcpyHostToDevice, st));
		double *d_tri = m->dist_tri.as<double>();
		HIP_TRY(hipMemsetAsync(d_tri, 0xff, tri_bytes * (c1 - c0), st));      // all-ones: NaN, the value of an empty cell

		HIP_TRY(hipEventRecord(m->dist_ev[0], st));
		const int n_big = (int)big.size(), n_small = (int)small.size();
		const int64_t waves = (int64_t)n_big + (n_small + 63) / 64;
		if (waves > 0) {
			const int wpb = HIBAG_DIST_BLOCK / 64;
			hipLaunchKernelGGL(k_dist_cells, dim3((unsigned)((waves + wpb - 1) / wpb)), dim3(HIBAG_DIST_BLOCK), 0, st,
				T, d_big, n_big, d_small, n_small, c0, n_tri, d_tri);
		}
		hipLaunchKernelGGL(k_dist_fold, dim3((unsigned)((nh + HIBAG_DIST_BLOCK - 1) / HIBAG_DIST_BLOCK), (unsigned)nh), dim3(HIBAG_DIST_BLOCK), 0, st,
			(const double *)d_tri, c1 - c0, nh, n_tri, m->dist_acc.as<double>(), m->dist_num.as<int>(), k == 0 ? 1 : 0,
			k == n_chunk - 1 ? 1 : 0, m->dist_out.as<double>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(m->dist_ev[1], st));
		if (out_each) {
			each.resize((size_t)n_tri * (c1 - c0));
			HIP_TRY(hipMemcpyAsync(each.data(), d_tri, tri_bytes * (c1 - c0), hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipStreamSynchronize(st));      // the cell lists and `each` are reused by the next chunk
		float ms = 0;
		if (hipEventElapsedTime(&ms, m->dist_ev[0], m->dist_ev[1]) == hipSuccess) ms_total += ms;
		if (out_each)
			for (int c = c0; c < c1; c++) {
				const double *t = each.data() + (size_t)(c - c0) * n_tri;
				double *o = out_each + (size_t)c * nh * nh;
				for (int64_t a = 0; a < nh; a++)
					for (int64_t b = a; b < nh; b++) {
						double v = t[hibag_dist_tri(nh, a, b)];
						if (std::isnan(v)) v = NAN;
						o[a * nh + b] = v;
						o[b * nh + a] = v;
					}
			}
	}
	HIP_TRY(hipMemcpyAsync(out, m->dist_out.p, out_bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	m->dist_ms = ms_total;
	return 0;
}

} // namespace hibag_detail

extern "C" {

int hibag_hip_model_distance(hibag_hip_model *m, double *out, double *out_each)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (!out) return hibag_fail(HIBAG_HIP_EINVAL, "out is NULL");
	std::lock_guard<std::mutex> g(m->lock);
	if (m->cls.empty()) return hibag_fail(HIBAG_HIP_EINVAL, "hlaDistance: the model has no classifier");
	HIP_TRY(hipSetDevice(m->device));
	const int rc = model_distance_locked(m, out, out_each);
	if (rc && m->dist_st) (void)hipStreamSynchronize(m->dist_st);
	return rc;
}

int hibag_hip_model_distance_ms(const hibag_hip_model *m, double *ms)
{
	if (!m || !ms) return hibag_fail(HIBAG_HIP_EINVAL, "NULL argument");
	*ms = m->dist_ms;
	return 0;
}

} // extern "C"
