// hibag_cohort.hip -- hibag_hip_cohort: a cohort's genotypes resident on one device (include/hibag_hip.h "resident cohort").
//
// Every other entry takes the raw genotypes again on every call: 4 bytes per genotype up the bus and a decode per model.  A
// cohort keeps them on the device in the 2-bit SNP-major form of a PLINK BED payload (hibag_k_cohort.h: PLINK's codes, rows
// a multiple of 16 bytes apart, the slots behind the last sample missing), which k_bed_codes turns into the byte codes of
// k_pack for any model, row map, flip set and sample window -- so a model's prediction on a cohort is the BED route of
// hibag_predict.hip with the payload already in place, and everything from k_pack on is the code every entry runs.
//   hibag_hip_cohort_new        from an int32 matrix in either memory order: slabs of at most 8 MB go up through pinned
//                               staging and k_cohort_pack turns each into its part of the rows (the int32 matrix is never
//                               resident whole); two slabs in flight, the host fills one while the other travels
//   hibag_hip_cohort_from_bed   from a BED file: the selected rows as they are in the file (an individual-major file is
//                               transposed on the host, two bits at a time)
//   hibag_hip_cohort_snp_counts k_cohort_counts: called genotypes and their sum per row
//   hibag_hip_predict_cohort / hibag_hip_predict_topk_cohort / hibag_hip_predict_draw_cohort
// A cohort is immutable once built: calls on different models may read it from different threads; each takes its model's
// lock like the other host-pointer entries.

#include "hibag_internal.h"
#include <functional>

struct hibag_hip_cohort {
	int device = 0;
	int n_samp = 0, n_snp = 0;
	size_t stride = 0;                 // bytes from one row to the next: ceil(n_samp / 4) rounded up to 16
	DevBuf rows;                       // [n_snp][stride]
	~hibag_hip_cohort()
	{
		(void)hipSetDevice(device);
		rows.release();
	}
};

namespace {

constexpr size_t SLAB_BYTES = (size_t)8 << 20;     // one slab of the int32 matrix (host staging and device, two of each)
constexpr int MAX_SAMP = 1 << 30;                  // k_cohort_counts sums a row in 32 bits

// Staging of hibag_hip_cohort_new, one per process: pinned memory is expensive to make (milliseconds for a few MB), so it is
// kept between calls; a build holds the lock throughout (cohorts are built one at a time).
struct Staging {
	std::mutex lock;
	int device = -1;
	PinBuf pin;
	DevBuf dev;
	hipStream_t st = nullptr;
	hipEvent_t done[2] = {nullptr, nullptr};

	void close()
	{
		if (device < 0) return;
		(void)hipSetDevice(device);
		if (st) (void)hipStreamDestroy(st);
		for (hipEvent_t &e : done) { if (e) (void)hipEventDestroy(e); e = nullptr; }
		st = nullptr;
		pin.release();
		dev.release();
		device = -1;
	}
	int open(int d)
	{
		if (device != d) {
			close();
			HIP_TRY(hipSetDevice(d));
			device = d;
			HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
			for (hipEvent_t &e : done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		}
		HIP_TRY(hipSetDevice(d));
		if (int rc = pin.reserve(2 * SLAB_BYTES)) return rc;
		return dev.reserve(2 * SLAB_BYTES);
	}
};
Staging g_stage;

size_t cohort_stride(int n_samp) { return (((size_t)n_samp + 3) / 4 + 15) / 16 * 16; }

int select_device(int *device)
{
	*device = hibag_selected_device();
	if (hibag_hip_device_count() <= *device) return hibag_fail(HIBAG_HIP_ENODEV, "no HIP device available");
	return 0;
}

int alloc_rows(hibag_hip_cohort *c, int device, int n_samp, int n_rows)
{
	c->device = device;
	c->n_samp = n_samp;
	c->n_snp = n_rows;
	c->stride = cohort_stride(n_samp);
	HIP_TRY(hipSetDevice(device));
	return c->rows.reserve(std::max<size_t>(c->stride * (size_t)n_rows, 16));
}

// the matrix -> the rows, slab by slab (g_stage.lock held)
int pack_matrix(hibag_hip_cohort *c, const int32_t *geno, int snp_major, size_t ld, const int32_t *snp_rows)
{
	Staging &S = g_stage;
	if (int rc = S.open(c->device)) return rc;
	const int n_samp = c->n_samp, R = c->n_snp;
	HIP_TRY(hipMemsetAsync(c->rows.p, 0x55, c->rows.cap, S.st));           // every slot missing until a slab says otherwise
	const size_t slab_ints = SLAB_BYTES / sizeof(int32_t);
	int n_slab = 0;
	// one slab: wait until the slot's previous slab has been packed, fill the slot (`fill` writes the pinned memory), send, pack
	auto slab = [&](const std::function<void(int32_t *)> &fill, size_t ints, int sm, size_t lds, int nk, int ns, int k0, int s0) -> int {
		const int slot = n_slab & 1;
		if (n_slab >= 2) HIP_TRY(hipEventSynchronize(S.done[slot]));
		int32_t *pin = (int32_t *)((char *)S.pin.p + (size_t)slot * SLAB_BYTES);
		int32_t *dev = (int32_t *)(S.dev.as<char>() + (size_t)slot * SLAB_BYTES);
		fill(pin);
		HIP_TRY(hipMemcpyAsync(dev, pin, ints * sizeof(int32_t), hipMemcpyHostToDevice, S.st));
		hibag_launch_cohort_pack(dev, sm, lds, nk, ns, c->rows.as<uint8_t>() + (size_t)k0 * c->stride, c->stride, (size_t)s0 / 4, S.st);
		HIP_TRY(hipEventRecord(S.done[slot], S.st));
		n_slab++;
		return 0;
	};
	if (snp_major) {
		// rows of the caller's matrix, cut along the samples where a row is long: [rows of the slab][samples of the chunk]
		const int chunk = 1 << 18;
		for (int s0 = 0; s0 < n_samp; s0 += chunk) {
			const int ns = std::min(chunk, n_samp - s0);
			const size_t lds = ((size_t)ns + 3) / 4 * 4;
			const int per = (int)std::max<size_t>(1, std::min<size_t>(slab_ints / lds, 32768));
			for (int k0 = 0; k0 < R; k0 += per) {
				const int nk = std::min(per, R - k0);
				auto fill = [&](int32_t *pin) {
					for (int r = 0; r < nk; r++) {
						const size_t src = snp_rows ? (size_t)snp_rows[k0 + r] : (size_t)(k0 + r);
						memcpy(pin + (size_t)r * lds, geno + src * ld + (size_t)s0, (size_t)ns * sizeof(int32_t));
					}
				};
				if (int rc = slab(fill, (size_t)nk * lds, 1, lds, nk, ns, k0, s0)) return rc;
			}
		}
	} else {
		// sample-major (the memory of R's SNP x sample matrix): [samples of the slab][SNPs of the slab], whole tiles of 256 samples
		const int per_k = std::min(std::max(R, 1), 8192);
		const int per_s = (int)std::max<size_t>(256, slab_ints / (size_t)per_k / 256 * 256);
		for (int s0 = 0; s0 < n_samp; s0 += per_s) {
			const int ns = std::min(per_s, n_samp - s0);
			for (int k0 = 0; k0 < R; k0 += per_k) {
				const int nk = std::min(per_k, R - k0);
				auto fill = [&](int32_t *pin) {
					for (int s = 0; s < ns; s++) {
						const int32_t *src = geno + (size_t)(s0 + s) * ld;
						int32_t *dst = pin + (size_t)s * nk;
						if (!snp_rows) memcpy(dst, src + k0, (size_t)nk * sizeof(int32_t));
						else for (int j = 0; j < nk; j++) dst[j] = src[snp_rows[k0 + j]];
					}
				};
				if (int rc = slab(fill, (size_t)ns * nk, 0, (size_t)nk, nk, ns, k0, s0)) return rc;
			}
		}
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(S.st));
	return 0;
}

// the selected rows of a BED image -> host copy of the resident rows (every slot behind n_samp: missing)
void bed_to_rows(const BedImage &img, int n_samp, int n_rows, size_t stride, std::vector<uint8_t> &out)
{
	out.assign(stride * (size_t)n_rows, 0x55);
	if (img.mode != 0) {
		const int tail = n_samp & 3;
		const uint8_t keep = (uint8_t)((1u << (2 * tail)) - 1u);
		for (int j = 0; j < n_rows; j++) {
			uint8_t *dst = out.data() + (size_t)j * stride;
			if (img.stride) memcpy(dst, img.rows.data() + (size_t)img.index[j] * img.stride, img.stride);
			if (tail) dst[img.stride - 1] = (uint8_t)((dst[img.stride - 1] & keep) | (0x55u & ~keep));
		}
	} else {
		// individual-major: row = sample, column = SNP; moved two bits at a time
		for (int s = 0; s < n_samp; s++) {
			const uint8_t *src = img.rows.data() + (size_t)s * img.stride;
			const int sh = 2 * (s & 3);
			const uint8_t clear = (uint8_t)~(3u << sh);
			for (int j = 0; j < n_rows; j++) {
				const int col = img.index[j];
				const uint8_t two = (uint8_t)((src[col >> 2] >> (2 * (col & 3))) & 3u);
				uint8_t &b = out[(size_t)j * stride + (size_t)(s >> 2)];
				b = (uint8_t)((b & clear) | (two << sh));
			}
		}
	}
}

int check_dims(int n_samp, int n_snp)
{
	if (n_samp < 0 || n_snp < 0) return hibag_fail(HIBAG_HIP_EINVAL, "negative dimensions (n_samp=%d, n_snp=%d)", n_samp, n_snp);
	if (n_samp > MAX_SAMP) return hibag_fail(HIBAG_HIP_EINVAL, "n_samp = %d: a cohort holds at most %d samples", n_samp, MAX_SAMP);
	return 0;
}

int check_rows(const int32_t *snp_rows, int n_rows, int n_snp)
{
	if (snp_rows && n_rows < 0) return hibag_fail(HIBAG_HIP_EINVAL, "n_rows < 0");
	for (int j = 0; snp_rows && j < n_rows; j++)
		if (snp_rows[j] < 0 || snp_rows[j] >= n_snp)
			return hibag_fail(HIBAG_HIP_EINVAL, "snp_rows[%d] = %d outside the %d SNPs of the source", j, snp_rows[j], n_snp);
	return 0;
}

int cohort_new(const int32_t *geno, int snp_major, size_t ld, int n_samp, int n_snp, const int32_t *snp_rows, int n_rows,
	hibag_hip_cohort **out)
{
	if (int rc = check_dims(n_samp, n_snp)) return rc;
	if (int rc = check_rows(snp_rows, n_rows, n_snp)) return rc;
	const int R = snp_rows ? n_rows : n_snp;
	if (n_samp > 0 && R > 0 && !geno) return hibag_fail(HIBAG_HIP_EINVAL, "geno is NULL");
	if (ld < (size_t)(snp_major ? n_samp : n_snp))
		return hibag_fail(HIBAG_HIP_EINVAL, "ld = %zu is smaller than the %d %s of a row", ld, snp_major ? n_samp : n_snp, snp_major ? "samples" : "SNPs");
	int device;
	if (int rc = select_device(&device)) return rc;
	hibag_hip_cohort *c = new (std::nothrow) hibag_hip_cohort;
	if (!c) return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
	int rc = alloc_rows(c, device, n_samp, R);
	if (!rc) {
		std::lock_guard<std::mutex> g(g_stage.lock);
		rc = pack_matrix(c, geno, snp_major, ld, snp_rows);
		if (rc && g_stage.st) (void)hipStreamSynchronize(g_stage.st);       // nothing of a failed build stays in flight on the shared slots
	}
	if (rc) { delete c; return rc; }
	*out = c;
	return 0;
}

int cohort_from_bed(const char *bed_fn, int n_samp, int n_snp, const int32_t *snp_rows, int n_rows, hibag_hip_cohort **out)
{
	if (int rc = check_dims(n_samp, n_snp)) return rc;
	if (int rc = check_rows(snp_rows, n_rows, n_snp)) return rc;
	std::vector<int32_t> all;
	std::vector<uint8_t> host;
	BedImage img;
	const int R = snp_rows ? n_rows : n_snp;
	try {
		if (!snp_rows) { all.resize(n_snp); for (int j = 0; j < n_snp; j++) all[j] = j; snp_rows = all.data(); }
		if (int rc = load_bed(bed_fn, n_samp, n_snp, snp_rows, R, img)) return rc;
		bed_to_rows(img, n_samp, R, cohort_stride(n_samp), host);
	} catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
	int device;
	if (int rc = select_device(&device)) return rc;
	hibag_hip_cohort *c = new (std::nothrow) hibag_hip_cohort;
	if (!c) return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
	auto body = [&]() -> int {
		if (int rc = alloc_rows(c, device, n_samp, R)) return rc;
		if (!host.empty()) HIP_TRY(hipMemcpy(c->rows.p, host.data(), host.size(), hipMemcpyHostToDevice));
		return 0;
	};
	if (int rc = body()) { delete c; return rc; }
	*out = c;
	return 0;
}

int predict_cohort_entry(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, const PredictOut &out)
{
	// (an unfinalized model is stated first by the entries that state it as EINVAL: check_predict_args does, before it looks at `c`)
	if (m && !c && (m->finalized || out.list.unfinalized_code() != HIBAG_HIP_EINVAL)) return hibag_fail(HIBAG_HIP_EINVAL, "cohort is NULL");
	if (int rc = check_predict_args(m, c, std::max(count, 0), vote_method, out.H1, out.H2, out.list.unfinalized_code())) return rc;
	if (m->device != c->device)
		return hibag_fail(HIBAG_HIP_EINVAL, "the cohort is on device %d, the model on device %d", c->device, m->device);
	if (first < 0 || count < 0 || (long long)first + count > c->n_samp)
		return hibag_fail(HIBAG_HIP_EINVAL, "samples [%d, %d + %d) lie outside the cohort's %d samples", first, first, count, c->n_samp);
	if (int rc = check_list_args(m, count, out.list)) return rc;
	if (!snp_col && m->n_snp > 0) return hibag_fail(HIBAG_HIP_EINVAL, "snp_col is NULL");
	for (int k = 0; k < m->n_snp; k++)
		if (snp_col[k] >= c->n_snp)
			return hibag_fail(HIBAG_HIP_EINVAL, "snp_col[%d] = %d outside the %d SNPs of the cohort", k, snp_col[k], c->n_snp);
	if (count == 0) return 0;
	std::lock_guard<std::mutex> g(m->lock);
	HIP_TRY(hipSetDevice(m->device));
	GenoSource src;                              // (a payload on the device: the resident rows)
	src.pack.d_bed = c->rows.as<uint8_t>();
	src.pack.mode = 1;
	src.pack.stride = c->stride;
	src.pack.samp0 = first;
	if (int rc = upload_snp_map(m, snp_col, flip, &src.pack.d_row, &src.pack.d_flip)) return rc;
	return predict_staged_locked(m, src, count, vote_method, out);
}

} // namespace

extern "C" {

hibag_hip_cohort *hibag_hip_cohort_new(const int32_t *geno, int snp_major, size_t ld, int n_samp, int n_snp,
	const int32_t *snp_rows, int n_rows)
{
	hibag_hip_cohort *c = nullptr;
	return cohort_new(geno, snp_major, ld, n_samp, n_snp, snp_rows, n_rows, &c) ? nullptr : c;
}

hibag_hip_cohort *hibag_hip_cohort_from_bed(const char *bed_fn, int n_samp, int n_snp, const int32_t *snp_rows, int n_rows)
{
	hibag_hip_cohort *c = nullptr;
	return cohort_from_bed(bed_fn, n_samp, n_snp, snp_rows, n_rows, &c) ? nullptr : c;
}

void hibag_hip_cohort_free(hibag_hip_cohort *c) { delete c; }

int hibag_hip_cohort_device(const hibag_hip_cohort *c) { return c ? c->device : -1; }
int hibag_hip_cohort_n_samp(const hibag_hip_cohort *c) { return c ? c->n_samp : 0; }
int hibag_hip_cohort_n_snp(const hibag_hip_cohort *c) { return c ? c->n_snp : 0; }
int64_t hibag_hip_cohort_bytes(const hibag_hip_cohort *c) { return c ? (int64_t)(c->stride * (size_t)c->n_snp) : 0; }

int hibag_hip_cohort_snp_counts(const hibag_hip_cohort *c, int32_t *n_valid, int64_t *sum)
{
	if (!c) return hibag_fail(HIBAG_HIP_EINVAL, "cohort is NULL");
	if (c->n_snp == 0) return 0;
	if (!n_valid || !sum) return hibag_fail(HIBAG_HIP_EINVAL, "n_valid and sum are both required");
	HIP_TRY(hipSetDevice(c->device));
	DevBuf d_n, d_sum;
	struct Free { DevBuf &a, &b; ~Free() { a.release(); b.release(); } } fr{d_n, d_sum};
	if (int rc = d_n.reserve((size_t)c->n_snp * sizeof(int32_t))) return rc;
	if (int rc = d_sum.reserve((size_t)c->n_snp * sizeof(int64_t))) return rc;
	hibag_launch_cohort_counts(c->rows.as<uint8_t>(), c->stride, c->n_snp, d_n.as<int32_t>(), d_sum.as<int64_t>(), 0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(n_valid, d_n.p, (size_t)c->n_snp * sizeof(int32_t), hipMemcpyDeviceToHost, 0));
	HIP_TRY(hipMemcpyAsync(sum, d_sum.p, (size_t)c->n_snp * sizeof(int64_t), hipMemcpyDeviceToHost, 0));
	HIP_TRY(hipStreamSynchronize(0));
	return 0;
}

int hibag_hip_predict_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage,
	double *postprob)
{
	return predict_cohort_entry(m, c, first, count, snp_col, flip, vote_method, {H1, H2, max_prob, matching, dosage, postprob});
}

int hibag_hip_predict_topk_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int k, int32_t *h1, int32_t *h2, double *prob, double *matching)
{
	return predict_cohort_entry(m, c, first, count, snp_col, flip, vote_method, PredictOut::topk(k, h1, h2, prob, matching));
}

// (`sample0` is the caller's index of sample `first`: the entry does not add `first` itself)
int hibag_hip_predict_draw_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int n_draw, uint64_t seed, int64_t sample0, int32_t *h1, int32_t *h2, double *prob,
	double *matching)
{
	return predict_cohort_entry(m, c, first, count, snp_col, flip, vote_method, PredictOut::draw(n_draw, seed, sample0, h1, h2, prob, matching));
}

int hibag_hip_predict_groups_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, const hibag_hip_groups *plan, int32_t *g1, int32_t *g2, double *prob, double *matching,
	double *dosage)
{
	return predict_cohort_entry(m, c, first, count, snp_col, flip, vote_method, PredictOut::groups(plan, g1, g2, prob, matching, dosage));
}

// (`allow` is indexed like the outputs: by the call's sample, not by the cohort's)
int hibag_hip_predict_given_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, const uint32_t *allow, int32_t *h1, int32_t *h2, double *prob, double *support,
	double *matching, double *dosage)
{
	return predict_cohort_entry(m, c, first, count, snp_col, flip, vote_method,
		PredictOut::given_sets(m, allow, h1, h2, prob, support, matching, dosage));
}

} // extern "C"
