// hibag_k_haplo.h -- kernels of hlaHaplotypes: the multi-locus haplotype EM over imputed calls.  Host side: hibag_haplo.hip;
// the definitions -- candidates, state order, the key, the summation rule S64, the EM -- are DESIGN.md section 29.
//
// A STATE is one phased choice of a sample: a candidate pair per locus and, for every heterozygous locus after the first, a
// phase bit.  State s has the constant wc[s] (the candidates' probabilities multiplied in locus order, times 2 unless every
// locus is homozygous) and two ENTRIES, 2s (haplotype A) and 2s + 1 (haplotype B); an entry's haplotype is a key of 10 bits
// per locus.  The dictionary is the sorted set of keys; hidx[entry] is the entry's haplotype, and entries[hstart[h] ..
// hstart[h + 1]) is haplotype h's list of entries in ascending entry number (one stable radix sort gives all three).
//
// Every sum is S64: 64 lanes stride the list, each adding in order, then p_j += p_{j + h} for h = 32 .. 1.  All terms are
// >= 0, so a lane without a term holds an exact 0, and a list of at most G = 8 or 16 entries summed by a group of G lanes
// with the butterfly from G / 2 down gives the same bits.  No atomics touch a frequency; the largest change of an iteration,
// a maximum of non-negative doubles, is taken on their bit patterns with one integer atomic per wavefront.
//
// The iterations of a batch are enqueued without a host round trip in between: every kernel of an iteration reads HaploCtl
// and returns at once when `done` is set, and k_haplo_step, the last kernel of an iteration, decides that.
#ifndef HIBAG_K_HAPLO_H_
#define HIBAG_K_HAPLO_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HAPLO_MAX_LOCI 6
#define HAPLO_KEY_BITS 10

// The loop's state on the device.  f[cur] is the current frequency vector, f[cur ^ 1] the one the M step writes.
struct HaploCtl {
	int done;                          // set by k_haplo_step: delta <= tol, or maxit iterations made
	int n_iter;                        // iterations made
	int cur;                           // which of the two frequency buffers is current
	int pad;
	unsigned long long delta_bits;     // max |f' - f| of the iteration under way, as the bits of a non-negative double
	double delta;                      // that of the last iteration made
};

// k_haplo_states: the states of every used sample, one workgroup of 256 per sample.  nc [L][n_used]: candidates per locus;
// c1 / c2 / cp [L][n_used][k]: the candidates (c1 <= c2), compacted to the front.  Combinations are numbered with locus
// L - 1 innermost; a lane takes a combination, a block scan of 2^max(het - 1, 0) gives its first state, and the lane writes
// the combination's states in ascending phase mask.  start [n_used + 1]: the samples' first states (the host's closed form);
// a state that would fall outside the sample's range is not written.
__global__ void __launch_bounds__(256) k_haplo_states(int n_used, int L, int k, const int32_t *__restrict__ nc,
	const int32_t *__restrict__ c1, const int32_t *__restrict__ c2, const double *__restrict__ cp,
	const long long *__restrict__ start, double *__restrict__ wc, unsigned long long *__restrict__ keys)
{
	__shared__ int s_scan[256];
	const int u = blockIdx.x, t = threadIdx.x;
	int n_c[HAPLO_MAX_LOCI];
	long long C = 1;
#pragma unroll
	for (int l = 0; l < HAPLO_MAX_LOCI; l++) {
		n_c[l] = l < L ? nc[(size_t)l * n_used + u] : 1;
		C *= n_c[l];
	}
	const long long s_begin = start[u], s_end = start[u + 1];
	long long base = 0;
	for (long long c0 = 0; c0 < C; c0 += 256) {
		const long long c = c0 + t;
		int a1[HAPLO_MAX_LOCI], a2[HAPLO_MAX_LOCI];
		double w = 0.0;
		int n_het = 0, slots = 0;
		if (c < C) {
			long long rest = c;
			int r[HAPLO_MAX_LOCI];
#pragma unroll
			for (int l = HAPLO_MAX_LOCI - 1; l >= 0; l--) {
				r[l] = 0;
				if (l < L) { r[l] = (int)(rest % n_c[l]); rest /= n_c[l]; }
			}
#pragma unroll
			for (int l = 0; l < HAPLO_MAX_LOCI; l++) {
				a1[l] = a2[l] = 0;
				if (l < L) {
					const size_t at = ((size_t)l * n_used + u) * k + r[l];
					a1[l] = c1[at]; a2[l] = c2[at];
					w = l == 0 ? cp[at] : w * cp[at];
					n_het += a1[l] != a2[l];
				}
			}
			slots = 1 << (n_het > 1 ? n_het - 1 : 0);
		}
		s_scan[t] = slots;
		__syncthreads();
		for (int d = 1; d < 256; d <<= 1) {
			const int v = t >= d ? s_scan[t - d] : 0;
			__syncthreads();
			s_scan[t] += v;
			__syncthreads();
		}
		const long long first = s_begin + base + (s_scan[t] - slots);
		base += s_scan[255];
		__syncthreads();
		if (c < C) {
			const double v = w * (n_het ? 2.0 : 1.0);
			for (int m = 0; m < slots; m++) {
				unsigned long long ka = 0, kb = 0;
				int j = -1;                  // heterozygous loci seen: the first is the anchor, the others take bit j of m
#pragma unroll
				for (int l = 0; l < HAPLO_MAX_LOCI; l++) {
					if (l >= L) continue;
					int x = a1[l], y = a2[l];
					if (x != y) {
						if (j >= 0 && ((m >> j) & 1)) { x = a2[l]; y = a1[l]; }
						j++;
					}
					ka |= (unsigned long long)x << (HAPLO_KEY_BITS * l);
					kb |= (unsigned long long)y << (HAPLO_KEY_BITS * l);
				}
				const long long s = first + m;
				if (s < s_end) {
					wc[s] = v;
					keys[2 * s] = ka;
					keys[2 * s + 1] = kb;
				}
			}
		}
	}
}

// payload of the sort: the entry numbers
__global__ void __launch_bounds__(256) k_haplo_iota(size_t n, uint32_t *__restrict__ out)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = (uint32_t)i;
}

// run heads of the sorted keys
__global__ void __launch_bounds__(256) k_haplo_heads(size_t n, const unsigned long long *__restrict__ key, int32_t *__restrict__ head)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) head[i] = i == 0 || key[i] != key[i - 1];
}

// rank: the inclusive scan of the heads.  Entry -> haplotype, and per haplotype its key and the start of its list
// (hstart [H + 1], the last written by the last entry).
__global__ void __launch_bounds__(256) k_haplo_dict(size_t n, const unsigned long long *__restrict__ key, const uint32_t *__restrict__ entries,
	const int32_t *__restrict__ head, const int32_t *__restrict__ rank, uint32_t *__restrict__ hidx, uint32_t *__restrict__ hstart,
	unsigned long long *__restrict__ ukeys)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t h = (uint32_t)rank[i] - 1;
	hidx[entries[i]] = h;
	if (head[i]) { hstart[h] = (uint32_t)i; ukeys[h] = key[i]; }
	if (i == n - 1) hstart[h + 1] = (uint32_t)n;
}

__global__ void __launch_bounds__(256) k_haplo_fill(size_t n, double v, double *__restrict__ out)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = v;
}

// the butterfly of S64 from G / 2 down: lane 0 of every group of G lanes ends with the sum
template <int G> __device__ __forceinline__ double haplo_butterfly(double p)
{
#pragma unroll
	for (int h = G / 2; h >= 1; h >>= 1) p = p + __shfl_down(p, h, G);
	return p;
}

// k_haplo_estep<G>: a group of G lanes per sample of `list` (G = 64: any sample; G = 16: samples of at most 16 states, four
// to a wavefront).  g = (wc f[A]) f[B] per state, tot = S64(g), q = g / tot (0 where tot == 0).  `force`: run although the
// loop is done (the last E step under the final frequencies).
template <int G> __global__ void __launch_bounds__(256) k_haplo_estep(const HaploCtl *__restrict__ ctl, int force, int n_list,
	const int32_t *__restrict__ list, const long long *__restrict__ start, const double *__restrict__ wc,
	const uint32_t *__restrict__ hidx, const double *__restrict__ f0, const double *__restrict__ f1, double *__restrict__ q,
	double *__restrict__ tot)
{
	if (!force && ctl->done) return;
	const double *f = ctl->cur ? f1 : f0;
	const int grp = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) / G), j = threadIdx.x % G;
	const bool live = grp < n_list;              // (a group past the list keeps its lanes in the shuffles, over an empty range)
	const int u = live ? list[grp] : 0;
	const long long s0 = live ? start[u] : 0, s1 = live ? start[u + 1] : 0;
	double p = 0.0;
	for (long long s = s0 + j; s < s1; s += G) {
		const double g = (wc[s] * f[hidx[2 * s]]) * f[hidx[2 * s + 1]];
		q[s] = g;
		p = p + g;
	}
	const double t = __shfl(haplo_butterfly<G>(p), 0, G);
	for (long long s = s0 + j; s < s1; s += G) q[s] = t == 0.0 ? 0.0 : q[s] / t;
	if (live && j == 0) tot[u] = t;
}

// k_haplo_mstep<G>: a group of G lanes per haplotype of `list` (G = 8, 16: lists of at most G entries).
// f'[h] = S64(q over h's list) / denom into the other buffer; the iteration's largest |f' - f| into ctl->delta_bits.
template <int G> __global__ void __launch_bounds__(256) k_haplo_mstep(HaploCtl *__restrict__ ctl, int n_list, const int32_t *__restrict__ list,
	const uint32_t *__restrict__ hstart, const uint32_t *__restrict__ entries, const double *__restrict__ q, double denom,
	double *__restrict__ f0, double *__restrict__ f1)
{
	if (ctl->done) return;
	const double *f = ctl->cur ? f1 : f0;
	double *fn = ctl->cur ? f0 : f1;
	const int grp = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) / G), j = threadIdx.x % G;
	const bool live = grp < n_list;
	const int h = live ? list[grp] : 0;
	const uint32_t a = live ? hstart[h] : 0, b = live ? hstart[h + 1] : 0;
	double p = 0.0;
	for (uint32_t i = a + j; i < b; i += G) p = p + q[entries[i] >> 1];
	p = haplo_butterfly<G>(p);
	double d = 0.0;
	if (live && j == 0) {
		const double v = p / denom;
		fn[h] = v;
		d = fabs(v - f[h]);
	}
#pragma unroll
	for (int w = 32; w >= 1; w >>= 1) d = fmax(d, __shfl_xor(d, w, 64));
	if ((threadIdx.x & 63) == 0 && d > 0.0) atomicMax(&ctl->delta_bits, (unsigned long long)__double_as_longlong(d));
}

// the end of an iteration: one thread
__global__ void k_haplo_step(HaploCtl *ctl, int maxit, double tol)
{
	if (ctl->done) return;
	const double d = __longlong_as_double((long long)ctl->delta_bits);
	ctl->delta = d;
	ctl->delta_bits = 0;
	ctl->n_iter += 1;
	ctl->cur ^= 1;
	if (d <= tol || ctl->n_iter >= maxit) ctl->done = 1;
}

// k_haplo_call: a wavefront per used sample: the state with the largest q, the first of equals; its two haplotypes decoded
// (hapA / hapB [n_used][L]) and its q.
__global__ void __launch_bounds__(256) k_haplo_call(int n_used, int L, const long long *__restrict__ start, const double *__restrict__ q,
	const unsigned long long *__restrict__ keys, int32_t *__restrict__ hapA, int32_t *__restrict__ hapB, double *__restrict__ prob)
{
	const int u = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) / 64), j = threadIdx.x & 63;
	const bool live = u < n_used;
	const long long s0 = live ? start[u] : 0, s1 = live ? start[u + 1] : 0;
	double bq = -1.0;
	long long bs = 0x7fffffffffffffffLL;
	for (long long s = s0 + j; s < s1; s += 64) {
		const double v = q[s];
		if (v > bq) { bq = v; bs = s; }
	}
#pragma unroll
	for (int w = 32; w >= 1; w >>= 1) {
		const double oq = __shfl_xor(bq, w, 64);
		const long long os = __shfl_xor(bs, w, 64);
		if (oq > bq || (oq == bq && os < bs)) { bq = oq; bs = os; }
	}
	if (!live || s1 <= s0) return;
	if (j < L) {
		const int sh = HAPLO_KEY_BITS * j;
		hapA[(size_t)u * L + j] = (int32_t)((keys[2 * bs] >> sh) & 1023);
		hapB[(size_t)u * L + j] = (int32_t)((keys[2 * bs + 1] >> sh) & 1023);
	}
	if (j == 0) prob[u] = bq;
}

// k_haplo_dosage: the posterior dosages of the haplotypes hap[0 .. m): out [m][n_used], zeroed
// by the host beforehand.  A haplotype's list is in ascending entry number and a sample's states are one range, so the list
// falls into one segment per sample that has an entry.  One workgroup per selected haplotype; thread t looks at the positions
// t, t + 256, ... of the list, finds the position's sample by bisection of `start`, and where the position before belongs
// to another sample (a segment head) adds the segment's q in order from 0.0 -- an all-homozygous state has both its entries
// here and adds its q twice -- and stores the sum.  Every cell has one writer.  Grid: m, 256 threads.
__global__ void __launch_bounds__(256) k_haplo_dosage(int n_used, const int32_t *__restrict__ hap, const long long *__restrict__ start,
	const uint32_t *__restrict__ hstart, const uint32_t *__restrict__ entries, const double *__restrict__ q, double *__restrict__ out)
{
	const int h = hap[blockIdx.x];
	const uint32_t a = hstart[h], b = hstart[h + 1];
	double *row = out + (size_t)blockIdx.x * n_used;
	for (uint32_t i = a + threadIdx.x; i < b; i += 256) {
		const long long s = entries[i] >> 1;
		int lo = 0, hi = n_used;                     // start[lo] <= s < start[hi]
		while (hi - lo > 1) {
			const int mid = lo + ((hi - lo) >> 1);
			if (start[mid] <= s) lo = mid; else hi = mid;
		}
		if (i > a && (long long)(entries[i - 1] >> 1) >= start[lo]) continue;   // not the head of its segment
		const long long s_end = start[lo + 1];
		double d = 0.0;
		for (uint32_t k = i; k < b; k++) {
			const long long t = entries[k] >> 1;
			if (t >= s_end) break;
			d = d + q[t];
		}
		row[lo] = d;
	}
}

#endif
