// hibag_haplo.hip -- host side of hlaHaplotypes: the handle behind `hibag_hip_haplo` and the entries of include/hibag_hip.h
// that use it.  Kernels: hibag_k_haplo.h; definitions: DESIGN.md section 29.
//
// hibag_hip_haplo_new checks and compacts the candidates, counts every sample's states in closed form, and builds on the
// device: the states (k_haplo_states), the dictionary and every haplotype's list (one stable radix sort of the entries' keys
// with the entry number as payload, run heads, a scan), and the work lists -- samples by state count, haplotypes by list
// length -- that decide the lane group an S64 sum gets.  hibag_hip_haplo_fit enqueues the iterations in batches; the kernels
// of a batch test the device's `done` flag, so the frequencies are those of the first iteration with delta <= tol whatever
// the batch size.  hibag_hip_haplo_dosage sums the last E step's posteriors per (haplotype, sample) (k_haplo_dosage).  A handle
// has one stream and is used by one host thread at a time.

#include <cstring>   // (rocprim's headers use memcpy without including it)
#include <rocprim/rocprim.hpp>

#include "hibag_internal.h"
#include "hibag_k_haplo.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using hibag_detail::DevBuf;

struct hibag_hip_haplo {
	int device = 0;
	int n_samp = 0, n_used = 0, L = 0;
	long long S = 0;                             // states; 2 S entries
	int H = 0;                                   // haplotypes
	hipStream_t st = nullptr;
	std::vector<int32_t> used;                   // [n_used]: the used samples' numbers
	std::vector<long long> h_start;              // [n_used + 1]
	std::vector<unsigned long long> h_ukeys;     // [H] ascending
	std::vector<double> h_tot;                   // [n_used]: the last E step's totals (hibag_hip_haplo_fit)
	bool fitted = false;
	int n_s16 = 0, n_s64 = 0, n_h8 = 0, n_h16 = 0, n_h64 = 0;
	DevBuf start, wc, keys, hidx, hstart, entries, q, tot, f0, f1, ctl;
	DevBuf s16, s64, h8, h16, h64;               // the work lists, int32
	DevBuf callA, callB, callP;                  // hibag_hip_haplo_calls
	DevBuf dosHap, dosOut;                       // hibag_hip_haplo_dosage: int32 [rows], double [rows][n_used] of one chunk

	~hibag_hip_haplo()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamSynchronize(st);
		for (DevBuf *b : {&start, &wc, &keys, &hidx, &hstart, &entries, &q, &tot, &f0, &f1, &ctl, &s16, &s64, &h8, &h16, &h64, &callA, &callB, &callP, &dosHap, &dosOut})
			b->release();
		if (st) (void)hipStreamDestroy(st);
	}
};

namespace {

struct TempBuf : DevBuf { ~TempBuf() { release(); } };   // a buffer of one function's frame

constexpr int kMaxK = 64;                        // candidates per sample and locus
constexpr int kMaxAllele = 1 << HAPLO_KEY_BITS;
constexpr long long kMaxEntries = 2147483647LL;
constexpr int kBatch = 8;                        // iterations enqueued between two looks at the device's flag
constexpr size_t kDosageChunk = (size_t)1 << 22; // cells of hibag_hip_haplo_dosage's device buffer (32 MB)

// the drain rule of hibag_assoc.hip: what `body` enqueued is waited for before a frame it reads or writes goes away
template <class Body> int enqueued(hipStream_t st, Body body)
{
	const int rc = body();
	if (rc) (void)hipStreamSynchronize(st);
	return rc;
}

unsigned blocks(size_t n, size_t per_block) { return (unsigned)std::max<size_t>((n + per_block - 1) / per_block, 1); }

int upload_list(DevBuf &b, const std::vector<int32_t> &v, hipStream_t st)
{
	if (b.reserve(sizeof(int32_t) * std::max<size_t>(v.size(), 1))) return HIBAG_HIP_ENOMEM;
	if (!v.empty()) HIP_TRY(hipMemcpyAsync(b.p, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice, st));
	return 0;
}

// what hibag_hip_haplo_new does on the device
int build(hibag_hip_haplo *h, int k, const std::vector<int32_t> &nc, const std::vector<int32_t> &c1, const std::vector<int32_t> &c2,
	const std::vector<double> &cp)
{
	const int nu = h->n_used, L = h->L;
	const size_t S = (size_t)h->S, E = 2 * S;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
	TempBuf d_nc, d_c1, d_c2, d_cp, d_iota, d_skeys, d_head, d_rank, d_tmp;
	if (h->start.reserve(sizeof(long long) * (nu + 1)) || h->wc.reserve(sizeof(double) * S) || h->keys.reserve(sizeof(uint64_t) * E) ||
		h->hidx.reserve(sizeof(uint32_t) * E) || h->entries.reserve(sizeof(uint32_t) * E) || h->q.reserve(sizeof(double) * S) ||
		h->tot.reserve(sizeof(double) * nu) || h->ctl.reserve(sizeof(HaploCtl)) ||
		d_nc.reserve(sizeof(int32_t) * nc.size()) || d_c1.reserve(sizeof(int32_t) * c1.size()) || d_c2.reserve(sizeof(int32_t) * c2.size()) ||
		d_cp.reserve(sizeof(double) * cp.size()) || d_iota.reserve(sizeof(uint32_t) * E) || d_skeys.reserve(sizeof(uint64_t) * E) ||
		d_head.reserve(sizeof(int32_t) * E) || d_rank.reserve(sizeof(int32_t) * E))
		return HIBAG_HIP_ENOMEM;
	unsigned long long *keys = h->keys.as<unsigned long long>(), *skeys = d_skeys.as<unsigned long long>();
	uint32_t *iota = d_iota.as<uint32_t>(), *entries = h->entries.as<uint32_t>();
	int32_t *head = d_head.as<int32_t>(), *rank = d_rank.as<int32_t>();
	size_t sort_bytes = 0, scan_bytes = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, skeys, iota, entries, E, 0u, (unsigned)(HAPLO_KEY_BITS * L), h->st));
	HIP_TRY(rocprim::inclusive_scan(nullptr, scan_bytes, head, rank, E, rocprim::plus<int32_t>(), h->st));
	if (d_tmp.reserve(std::max<size_t>(std::max(sort_bytes, scan_bytes), 16))) return HIBAG_HIP_ENOMEM;

	int32_t last_rank = 0;
	if (int rc = enqueued(h->st, [&]() -> int {
		HIP_TRY(hipMemcpyAsync(h->start.p, h->h_start.data(), sizeof(long long) * (nu + 1), hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(d_nc.p, nc.data(), sizeof(int32_t) * nc.size(), hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(d_c1.p, c1.data(), sizeof(int32_t) * c1.size(), hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(d_c2.p, c2.data(), sizeof(int32_t) * c2.size(), hipMemcpyHostToDevice, h->st));
		HIP_TRY(hipMemcpyAsync(d_cp.p, cp.data(), sizeof(double) * cp.size(), hipMemcpyHostToDevice, h->st));
		hipLaunchKernelGGL(k_haplo_states, dim3(nu), dim3(256), 0, h->st, nu, L, k, d_nc.as<int32_t>(), d_c1.as<int32_t>(), d_c2.as<int32_t>(),
			d_cp.as<double>(), h->start.as<long long>(), h->wc.as<double>(), keys);
		hipLaunchKernelGGL(k_haplo_iota, dim3(blocks(E, 256)), dim3(256), 0, h->st, E, iota);
		HIP_TRY(hipGetLastError());
		HIP_TRY(rocprim::radix_sort_pairs(d_tmp.p, sort_bytes, keys, skeys, iota, entries, E, 0u, (unsigned)(HAPLO_KEY_BITS * L), h->st));
		hipLaunchKernelGGL(k_haplo_heads, dim3(blocks(E, 256)), dim3(256), 0, h->st, E, skeys, head);
		HIP_TRY(hipGetLastError());
		HIP_TRY(rocprim::inclusive_scan(d_tmp.p, scan_bytes, head, rank, E, rocprim::plus<int32_t>(), h->st));
		HIP_TRY(hipMemcpyAsync(&last_rank, rank + (E - 1), sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	})) return rc;
	if (last_rank < 1 || (size_t)last_rank > E) return hibag_fail(HIBAG_HIP_ENODEV, "hibag_hip_haplo_new: the dictionary scan returned %d haplotypes for %zu entries", last_rank, E);
	const int H = h->H = last_rank;
	TempBuf d_ukeys;
	if (h->hstart.reserve(sizeof(uint32_t) * ((size_t)H + 1)) || d_ukeys.reserve(sizeof(uint64_t) * H) || h->f0.reserve(sizeof(double) * H) ||
		h->f1.reserve(sizeof(double) * H))
		return HIBAG_HIP_ENOMEM;
	std::vector<uint32_t> hs((size_t)H + 1);
	h->h_ukeys.resize((size_t)H);
	if (int rc = enqueued(h->st, [&]() -> int {
		hipLaunchKernelGGL(k_haplo_dict, dim3(blocks(E, 256)), dim3(256), 0, h->st, E, skeys, entries, head, rank, h->hidx.as<uint32_t>(),
			h->hstart.as<uint32_t>(), d_ukeys.as<unsigned long long>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(hs.data(), h->hstart.p, sizeof(uint32_t) * hs.size(), hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(h->h_ukeys.data(), d_ukeys.p, sizeof(uint64_t) * H, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	})) return rc;

	// the work lists: which lane group sums a sample's states, a haplotype's list
	std::vector<int32_t> s16, s64, h8, h16, h64;
	for (int u = 0; u < nu; u++) (h->h_start[u + 1] - h->h_start[u] <= 16 ? s16 : s64).push_back(u);
	for (int i = 0; i < H; i++) {
		const uint32_t len = hs[i + 1] - hs[i];
		(len <= 8 ? h8 : len <= 16 ? h16 : h64).push_back(i);
	}
	h->n_s16 = (int)s16.size(); h->n_s64 = (int)s64.size();
	h->n_h8 = (int)h8.size(); h->n_h16 = (int)h16.size(); h->n_h64 = (int)h64.size();
	return enqueued(h->st, [&]() -> int {
		if (int rc = upload_list(h->s16, s16, h->st)) return rc;
		if (int rc = upload_list(h->s64, s64, h->st)) return rc;
		if (int rc = upload_list(h->h8, h8, h->st)) return rc;
		if (int rc = upload_list(h->h16, h16, h->st)) return rc;
		if (int rc = upload_list(h->h64, h64, h->st)) return rc;
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	});
}

template <int G> void launch_estep(hibag_hip_haplo *h, int force, int n_list, const DevBuf &list)
{
	if (n_list == 0) return;
	hipLaunchKernelGGL(k_haplo_estep<G>, dim3(blocks((size_t)n_list * G, 256)), dim3(256), 0, h->st, h->ctl.as<HaploCtl>(), force, n_list,
		list.as<int32_t>(), h->start.as<long long>(), h->wc.as<double>(), h->hidx.as<uint32_t>(), h->f0.as<double>(), h->f1.as<double>(),
		h->q.as<double>(), h->tot.as<double>());
}

void enqueue_estep(hibag_hip_haplo *h, int force)
{
	launch_estep<16>(h, force, h->n_s16, h->s16);
	launch_estep<64>(h, force, h->n_s64, h->s64);
}

template <int G> void launch_mstep(hibag_hip_haplo *h, int n_list, const DevBuf &list, double denom)
{
	if (n_list == 0) return;
	hipLaunchKernelGGL(k_haplo_mstep<G>, dim3(blocks((size_t)n_list * G, 256)), dim3(256), 0, h->st, h->ctl.as<HaploCtl>(), n_list,
		list.as<int32_t>(), h->hstart.as<uint32_t>(), h->entries.as<uint32_t>(), h->q.as<double>(), denom, h->f0.as<double>(), h->f1.as<double>());
}

} // namespace

extern "C" {

hibag_hip_haplo *hibag_hip_haplo_new(int n_samp, int n_loci, int k, const int32_t *h1, const int32_t *h2, const double *prob,
	int max_states, int device)
{
	const char *me = "hibag_hip_haplo_new";
	if (!h1 || !h2 || !prob || n_samp <= 0 || k < 1 || k > kMaxK || max_states < 1) {
		hibag_fail(HIBAG_HIP_EINVAL, "%s: need h1, h2, prob, n_samp > 0, 1 <= k <= %d and max_states >= 1 (got %d samples, k = %d, max_states = %d)",
			me, kMaxK, n_samp, k, max_states);
		return nullptr;
	}
	if (n_loci < 2 || n_loci > HAPLO_MAX_LOCI) {
		hibag_fail(HIBAG_HIP_EINVAL, "%s: %d loci; 2 .. %d", me, n_loci, HAPLO_MAX_LOCI);
		return nullptr;
	}
	int n_dev = 0;
	if (device < -1 || (device >= 0 && (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev))) {
		hibag_fail(HIBAG_HIP_EINVAL, "%s: device %d; -1 (the calling thread's) or 0 .. %d", me, device, n_dev - 1);
		return nullptr;
	}
	const int L = n_loci;
	const auto at = [&](int l, int s, int r) { return ((size_t)l * n_samp + s) * k + r; };
	// the used samples: a candidate at every locus.  A rank with an NA allele or probability 0 is no candidate.
	std::vector<int32_t> used;
	for (int s = 0; s < n_samp; s++) {
		bool all = true;
		for (int l = 0; l < L; l++) {
			int n = 0;
			for (int r = 0; r < k; r++) {
				const int32_t a = h1[at(l, s, r)], b = h2[at(l, s, r)];
				const double p = prob[at(l, s, r)];
				if (a == HIBAG_HIP_NA_INTEGER || b == HIBAG_HIP_NA_INTEGER) continue;
				if (a < 0 || b < 0 || a >= kMaxAllele || b >= kMaxAllele) {
					hibag_fail(HIBAG_HIP_EINVAL, "%s: sample %d, locus %d, rank %d has the alleles (%d, %d); indices are 0 .. %d or NA", me, s, l, r, a, b,
						kMaxAllele - 1);
					return nullptr;
				}
				if (!(p >= 0.0) || !std::isfinite(p)) {
					hibag_fail(HIBAG_HIP_EINVAL, "%s: sample %d, locus %d, rank %d has the probability %g; finite and >= 0", me, s, l, r, p);
					return nullptr;
				}
				n += p > 0.0;
			}
			all = all && n > 0;
		}
		if (all) used.push_back(s);
	}
	if (used.empty()) {
		hibag_fail(HIBAG_HIP_EINVAL, "%s: no sample has a candidate at every locus", me);
		return nullptr;
	}
	// compacted candidates [L][n_used][k] and the states per sample: (prod (hom + 2 het) + prod hom) / 2
	const int nu = (int)used.size();
	std::vector<int32_t> nc((size_t)L * nu), c1((size_t)L * nu * k, 0), c2((size_t)L * nu * k, 0);
	std::vector<double> cp((size_t)L * nu * k, 0.0);
	std::vector<long long> start((size_t)nu + 1, 0);
	for (int u = 0; u < nu; u++) {
		const int s = used[u];
		long long all = 1, hom = 1;
		for (int l = 0; l < L; l++) {
			int n = 0, n_hom = 0;
			for (int r = 0; r < k; r++) {
				const int32_t a = h1[at(l, s, r)], b = h2[at(l, s, r)];
				const double p = prob[at(l, s, r)];
				if (a == HIBAG_HIP_NA_INTEGER || b == HIBAG_HIP_NA_INTEGER || !(p > 0.0)) continue;
				const size_t o = ((size_t)l * nu + u) * k + n;
				c1[o] = std::min(a, b); c2[o] = std::max(a, b); cp[o] = p;
				n++;
				n_hom += a == b;
			}
			nc[(size_t)l * nu + u] = n;
			all *= n_hom + 2 * (n - n_hom);
			hom *= n_hom;
		}
		const long long states = (all + hom) / 2;
		if (states > max_states) {
			hibag_fail(HIBAG_HIP_EINVAL, "%s: sample %d has %lld states, more than max_states = %d", me, s, states, max_states);
			return nullptr;
		}
		start[u + 1] = start[u] + states;
		if (2 * start[u + 1] > kMaxEntries) {
			hibag_fail(HIBAG_HIP_EINVAL, "%s: more than 2^31 - 1 entries (two per state) in total", me);
			return nullptr;
		}
	}
	hibag_hip_haplo *h = new (std::nothrow) hibag_hip_haplo;
	if (!h) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	h->device = device >= 0 ? device : hibag_selected_device();
	h->n_samp = n_samp; h->n_used = nu; h->L = L;
	h->S = start[nu];
	h->used = used;
	h->h_start = start;
	if (build(h, k, nc, c1, c2, cp) != 0) { delete h; return nullptr; }
	return h;
}

void hibag_hip_haplo_free(hibag_hip_haplo *h) { delete h; }

int hibag_hip_haplo_dims(const hibag_hip_haplo *h, int32_t *n_hap, int64_t *n_states, int32_t *n_used, int32_t *used, int64_t *states)
{
	if (!h) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_dims: null handle");
	if (n_hap) *n_hap = h->H;
	if (n_states) *n_states = h->S;
	if (n_used) *n_used = h->n_used;
	if (used) std::fill(used, used + h->n_samp, 0);
	if (states) std::fill(states, states + h->n_samp, (int64_t)0);
	for (int u = 0; u < h->n_used; u++) {
		if (used) used[h->used[u]] = 1;
		if (states) states[h->used[u]] = h->h_start[u + 1] - h->h_start[u];
	}
	return 0;
}

int hibag_hip_haplo_fit(hibag_hip_haplo *h, int maxit, double tol, double *freq, uint64_t *keys, int32_t *n_iter, double *delta,
	int32_t *n_zero)
{
	if (!h || !freq || !keys || !n_iter || !delta || !n_zero) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_fit: null argument");
	if (maxit < 1) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_fit: maxit = %d; at least 1", maxit);
	if (!(tol >= 0.0)) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_fit: tol must be >= 0");
	HIP_TRY(hipSetDevice(h->device));
	const size_t H = (size_t)h->H;
	const double denom = 2.0 * (double)h->n_used;
	HaploCtl c;
	h->h_tot.resize((size_t)h->n_used);
	h->fitted = false;
	if (int rc = enqueued(h->st, [&]() -> int {
		HIP_TRY(hipMemsetAsync(h->ctl.p, 0, sizeof(HaploCtl), h->st));
		hipLaunchKernelGGL(k_haplo_fill, dim3(blocks(H, 256)), dim3(256), 0, h->st, H, 1.0 / (double)h->H, h->f0.as<double>());
		HIP_TRY(hipGetLastError());
		for (int made = 0;;) {
			// (the device stops counting at maxit; a batch may run past it, its kernels then return at once)
			for (int b = 0; b < kBatch && made < maxit; b++, made++) {
				enqueue_estep(h, 0);
				launch_mstep<8>(h, h->n_h8, h->h8, denom);
				launch_mstep<16>(h, h->n_h16, h->h16, denom);
				launch_mstep<64>(h, h->n_h64, h->h64, denom);
				hipLaunchKernelGGL(k_haplo_step, dim3(1), dim3(1), 0, h->st, h->ctl.as<HaploCtl>(), maxit, tol);
				HIP_TRY(hipGetLastError());
			}
			HIP_TRY(hipMemcpyAsync(&c, h->ctl.p, sizeof(HaploCtl), hipMemcpyDeviceToHost, h->st));
			HIP_TRY(hipStreamSynchronize(h->st));
			if (c.done) break;
			if (made >= maxit) return hibag_fail(HIBAG_HIP_ESTATE, "hibag_hip_haplo_fit: %d iterations enqueued and the device reports %d", made, c.n_iter);
		}
		// the last E step, under the final frequencies: q for the calls, the totals for the log-likelihood
		enqueue_estep(h, 1);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(freq, c.cur ? h->f1.p : h->f0.p, sizeof(double) * H, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(h->h_tot.data(), h->tot.p, sizeof(double) * h->n_used, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	})) return rc;
	std::copy(h->h_ukeys.begin(), h->h_ukeys.end(), keys);
	*n_iter = c.n_iter;
	*delta = c.delta;
	*n_zero = (int32_t)std::count(h->h_tot.begin(), h->h_tot.end(), 0.0);
	h->fitted = true;
	return 0;
}

int hibag_hip_haplo_calls(hibag_hip_haplo *h, int32_t *hapA, int32_t *hapB, double *prob, double *total)
{
	if (!h || !hapA || !hapB || !prob || !total) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_calls: null argument");
	if (!h->fitted) return hibag_fail(HIBAG_HIP_ESTATE, "hibag_hip_haplo_calls: call hibag_hip_haplo_fit first");
	HIP_TRY(hipSetDevice(h->device));
	const int nu = h->n_used, L = h->L;
	if (h->callA.reserve(sizeof(int32_t) * (size_t)nu * L) || h->callB.reserve(sizeof(int32_t) * (size_t)nu * L) || h->callP.reserve(sizeof(double) * nu))
		return HIBAG_HIP_ENOMEM;
	std::vector<int32_t> a((size_t)nu * L), b((size_t)nu * L);
	std::vector<double> p((size_t)nu);
	if (int rc = enqueued(h->st, [&]() -> int {
		hipLaunchKernelGGL(k_haplo_call, dim3(blocks((size_t)nu * 64, 256)), dim3(256), 0, h->st, nu, L, h->start.as<long long>(), h->q.as<double>(),
			h->keys.as<unsigned long long>(), h->callA.as<int32_t>(), h->callB.as<int32_t>(), h->callP.as<double>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(a.data(), h->callA.p, sizeof(int32_t) * a.size(), hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(b.data(), h->callB.p, sizeof(int32_t) * b.size(), hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipMemcpyAsync(p.data(), h->callP.p, sizeof(double) * nu, hipMemcpyDeviceToHost, h->st));
		HIP_TRY(hipStreamSynchronize(h->st));
		return 0;
	})) return rc;
	// the samples left out: NA and NaN
	std::fill(hapA, hapA + (size_t)h->n_samp * L, HIBAG_HIP_NA_INTEGER);
	std::fill(hapB, hapB + (size_t)h->n_samp * L, HIBAG_HIP_NA_INTEGER);
	std::fill(prob, prob + h->n_samp, std::nan(""));
	std::fill(total, total + h->n_samp, std::nan(""));
	for (int u = 0; u < nu; u++) {
		const int s = h->used[u];
		std::copy(&a[(size_t)u * L], &a[(size_t)u * L] + L, hapA + (size_t)s * L);
		std::copy(&b[(size_t)u * L], &b[(size_t)u * L] + L, hapB + (size_t)s * L);
		prob[s] = p[u];
		total[s] = h->h_tot[u];
	}
	return 0;
}

int hibag_hip_haplo_dosage(hibag_hip_haplo *h, const int32_t *hap, int m, double *out)
{
	if (!h || !hap || !out) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_dosage: null argument");
	if (!h->fitted) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_dosage: call hibag_hip_haplo_fit first");
	if (m < 1) return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_dosage: m = %d; at least 1", m);
	for (int j = 0; j < m; j++)
		if (hap[j] < 0 || hap[j] >= h->H)
			return hibag_fail(HIBAG_HIP_EINVAL, "hibag_hip_haplo_dosage: hap[%d] = %d; haplotype indices are 0 .. %d", j, hap[j], h->H - 1);
	HIP_TRY(hipSetDevice(h->device));
	const int nu = h->n_used;
	const int chunk = (int)std::min<size_t>((size_t)m, std::max<size_t>(kDosageChunk / (size_t)nu, 1));   // rows per launch
	if (h->dosHap.reserve(sizeof(int32_t) * (size_t)chunk) || h->dosOut.reserve(sizeof(double) * (size_t)chunk * nu)) return HIBAG_HIP_ENOMEM;
	std::vector<double> d((size_t)chunk * nu);
	for (int j0 = 0; j0 < m; j0 += chunk) {
		const int rows = std::min(chunk, m - j0);
		if (int rc = enqueued(h->st, [&]() -> int {
			HIP_TRY(hipMemcpyAsync(h->dosHap.p, hap + j0, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, h->st));
			HIP_TRY(hipMemsetAsync(h->dosOut.p, 0, sizeof(double) * (size_t)rows * nu, h->st));
			hipLaunchKernelGGL(k_haplo_dosage, dim3(rows), dim3(256), 0, h->st, nu, h->dosHap.as<int32_t>(), h->start.as<long long>(),
				h->hstart.as<uint32_t>(), h->entries.as<uint32_t>(), h->q.as<double>(), h->dosOut.as<double>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(d.data(), h->dosOut.p, sizeof(double) * (size_t)rows * nu, hipMemcpyDeviceToHost, h->st));
			HIP_TRY(hipStreamSynchronize(h->st));
			return 0;
		})) return rc;
		// the samples left out: NaN
		for (int j = 0; j < rows; j++) {
			double *o = out + (size_t)(j0 + j) * h->n_samp;
			std::fill(o, o + h->n_samp, std::nan(""));
			for (int u = 0; u < nu; u++) o[h->used[u]] = d[(size_t)j * nu + u];
		}
	}
	return 0;
}

} // extern "C"
