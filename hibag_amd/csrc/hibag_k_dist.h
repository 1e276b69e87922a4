// hibag_k_dist.h -- hlaDistance on the device (HIBAG_Distance, src/HIBAG.cpp:1284-1332, and the fold of R/HIBAG.R:1545-1570).
//
// A CELL is (classifier c, allele a <= b).  Because a classifier's haplotypes are grouped by ascending allele, its pairs are
// i in [s_a, e_a), j in [max(i, s_b), e_b), taken i-major: pair k of the cell is row r = k / n_b, column q = k % n_b of the
// rectangle (a < b), or the k-th entry of the upper triangle rows r <= q < n_a (a == b).  Per pair
//     d = popcount(bits[i] ^ bits[j]),  f = freq[i] * freq[j],  freq_sum += f,  dist_sum += f * d
// and the cell's value is dist_sum / freq_sum.  The two sums are chains of dependent adds in that order: nothing here
// reorders them, splits them or fuses f * d into the add (-ffp-contract=off).  What runs in parallel is everything else:
// the loads, popcounts and products of the pairs.
//
// k_dist_cells: one launch for every cell of a chunk of classifiers.  Waves [0, n_big) take one LARGE cell each (more than
// HIBAG_DIST_LANE_MAX pairs), largest first: its 64 lanes compute 64 consecutive pairs' (f, f * d) into the wave's LDS
// row and then add them in order, every lane the same chain (the next 64 pairs' loads are in flight meanwhile).  The waves
// after them take 64 SMALL cells each, one cell per lane, walked serially by that lane (cells sorted by size, so the lanes
// of a wave finish together).
// k_dist_fold: R's fold over the classifiers, in classifier order, one thread per (a <= b).
#ifndef HIBAG_K_DIST_H_
#define HIBAG_K_DIST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HIBAG_DIST_LANE_MAX 64        // cells with at most this many pairs are walked by one lane
#define HIBAG_DIST_BLOCK 256          // 4 waves

struct HibagDistTables {
	const uint64_t *bits;             // [haplotype][2]: the two words of THaplotype::PackedHaplo, bits >= n_snp zero
	const double *freq;               // [haplotype]
	const int *off;                   // [classifier] first haplotype
	const int *start;                 // [classifier][n_hla + 1] allele starts within the classifier
	int n_hla;
};

// (classifier, a, b); `pad` unused
struct HibagDistCell { int c, a, b, pad; };

// packed upper triangle: (a, b), a <= b, row-major
__host__ __device__ inline int64_t hibag_dist_tri(int64_t n, int64_t a, int64_t b) { return a * (2 * n - a + 1) / 2 + (b - a); }

// Pair k of a cell as (row r, column q), both relative to the allele starts.
__device__ inline void hibag_dist_pair(int64_t k, bool diag, int64_t na, int64_t nb, int64_t &r, int64_t &q)
{
	if (!diag) {
		if (k <= 0x7fffffff) { const uint32_t r32 = (uint32_t)k / (uint32_t)nb; r = r32; q = (uint32_t)k - r32 * (uint32_t)nb; }
		else { r = k / nb; q = k - r * nb; }
		return;
	}
	// row r of the triangle starts at P(r) = r (2 na - r + 1) / 2: the largest r with P(r) <= k, from the quadratic and
	// corrected in exact integers (the double estimate is off by at most one for any na this library accepts)
	const double w = (double)(2 * na + 1);
	int64_t t = (int64_t)((w - sqrt(w * w - 8.0 * (double)k)) * 0.5);
	t = t < 0 ? 0 : (t > na - 1 ? na - 1 : t);
	if (t * (2 * na - t + 1) / 2 > k) t--;
	if (t + 1 < na && (t + 1) * (2 * na - t) / 2 <= k) t++;
	r = t;
	q = t + (k - t * (2 * na - t + 1) / 2);
}

__global__ void __launch_bounds__(HIBAG_DIST_BLOCK)
k_dist_cells(HibagDistTables T, const HibagDistCell *__restrict__ big, int n_big, const HibagDistCell *__restrict__ small,
	int n_small, int c0, int64_t n_tri, double *__restrict__ tri)
{
	__shared__ double2 lds[HIBAG_DIST_BLOCK];
	const int lane = threadIdx.x & 63;
	const int w = blockIdx.x * (HIBAG_DIST_BLOCK / 64) + (threadIdx.x >> 6);      // wave-uniform
	const int nh = T.n_hla;

	if (w < n_big) {
		const HibagDistCell cell = big[w];
		const int *st = T.start + (int64_t)cell.c * (nh + 1);
		const int64_t o = T.off[cell.c];
		const int64_t sa = o + st[cell.a], na = st[cell.a + 1] - st[cell.a];
		const int64_t sb = o + st[cell.b], nb = st[cell.b + 1] - st[cell.b];
		const bool diag = cell.a == cell.b;
		const int64_t np = diag ? na * (na + 1) / 2 : na * nb;
		double2 *row = lds + (threadIdx.x & ~63);

		// raw operands of pair `base + lane`; the arithmetic on them waits until after the previous chunk's adds
		uint64_t bi0 = 0, bi1 = 0, bj0 = 0, bj1 = 0;
		double fi = 0, fj = 0;
		auto load = [&](int64_t base) {
			const int64_t k = base + lane;
			if (k < np) {
				int64_t r, q;
				hibag_dist_pair(k, diag, na, nb, r, q);
				const int64_t i = sa + r, j = (diag ? sa : sb) + q;
				bi0 = T.bits[2 * i]; bi1 = T.bits[2 * i + 1]; fi = T.freq[i];
				bj0 = T.bits[2 * j]; bj1 = T.bits[2 * j + 1]; fj = T.freq[j];
			}
		};
		double fs = 0, ds = 0;
		load(0);
		for (int64_t base = 0; base < np; base += 64) {
			const int d = __popcll(bi0 ^ bj0) + __popcll(bi1 ^ bj1);
			const double f = fi * fj;
			row[lane] = make_double2(f, f * (double)d);
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			if (base + 64 < np) load(base + 64);
			const int n = (int)(np - base < 64 ? np - base : 64);
			for (int t = 0; t < n; t++) {                 // the reference order: pair base + t
				const double2 v = row[t];
				fs += v.x;
				ds += v.y;
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
		if (lane == 0) tri[(int64_t)(cell.c - c0) * n_tri + hibag_dist_tri(nh, cell.a, cell.b)] = ds / fs;
		return;
	}

	const int64_t idx = (int64_t)(w - n_big) * 64 + lane;
	if (idx >= n_small) return;
	const HibagDistCell cell = small[idx];
	const int *st = T.start + (int64_t)cell.c * (nh + 1);
	const int o = T.off[cell.c];
	const int sa = o + st[cell.a], na = st[cell.a + 1] - st[cell.a];
	const int sb = o + st[cell.b], nb = st[cell.b + 1] - st[cell.b];
	const bool diag = cell.a == cell.b;
	const int np = diag ? na * (na + 1) / 2 : na * nb;      // <= HIBAG_DIST_LANE_MAX
	const int qn = diag ? na : nb;
	double fs = 0, ds = 0;
	int r = 0, q = 0;
	for (int k = 0; k < np; k++) {
		const int i = sa + r, j = (diag ? sa : sb) + q;
		const int d = __popcll(T.bits[2 * i] ^ T.bits[2 * j]) + __popcll(T.bits[2 * i + 1] ^ T.bits[2 * j + 1]);
		const double f = T.freq[i] * T.freq[j];
		fs += f;
		ds += f * (double)d;
		if (++q == qn) { r++; q = diag ? r : 0; }
	}
	tri[(int64_t)(cell.c - c0) * n_tri + hibag_dist_tri(nh, cell.a, cell.b)] = ds / fs;
}

// R's `num <- num + !is.na(m); m[is.na(m)] <- 0; Reduce("+", lst) / num` over the n_c classifiers of one chunk, for the
// cells (a, b = blockIdx.x * 256 + threadIdx.x >= a): the running sum and count come in from `acc` / `num` unless this is
// the first chunk (the fold then starts at the first classifier's value, as Reduce does), and go out to them unless this
// is the last, which writes both (a, b) and (b, a) of the n_hla x n_hla result.
__global__ void __launch_bounds__(HIBAG_DIST_BLOCK)
k_dist_fold(const double *__restrict__ tri, int n_c, int n_hla, int64_t n_tri, double *__restrict__ acc, int *__restrict__ num,
	int first, int last, double *__restrict__ out)
{
	const int a = blockIdx.y;
	const int b = blockIdx.x * HIBAG_DIST_BLOCK + threadIdx.x;
	if (b < a || b >= n_hla) return;
	const int64_t t = hibag_dist_tri(n_hla, a, b);
	double s = first ? 0.0 : acc[t];
	int k = first ? 0 : num[t];
	for (int c = 0; c < n_c; c++) {
		const double v = tri[(int64_t)c * n_tri + t];
		const bool ok = !isnan(v);
		const double v0 = ok ? v : 0.0;
		s = (first && c == 0) ? v0 : s + v0;
		k += ok ? 1 : 0;
	}
	if (!last) { acc[t] = s; num[t] = k; return; }
	const double r = s / (double)k;
	out[(int64_t)a * n_hla + b] = r;
	out[(int64_t)b * n_hla + a] = r;
}

#endif
