// hibag_k_prefix.h -- the kernels of hibag_prefix.hip (included there): hibag_hip_predict_prefix, the prediction of every
// sub-model "first sizes[i] classifiers" (hlaSubModelObj, R/HIBAG.R:1121-1129) of one model from ONE pass 1.
//
// What a sub-model of the first k classifiers shares with the full model: every classifier's cell sums, their in-order total
// and 1/total (they depend on the classifier and the sample alone).  What differs: snp_weight[s] counts the classifiers OF
// THE SUB-MODEL that use SNP s (_GetSNPWeights, src/LibHLA.cpp:2484-2496), so each classifier's weight for a sample --
// the share of its non-missing SNPs under those counts (:2418-2431) -- is the sub-model's own.  Whether a weight is
// positive is not: every SNP of a classifier c < k counts at least c itself, so the weight is positive exactly where the
// sample has any of c's SNPs, in every sub-model that contains c (pass 1 skips a (group, classifier) by the full model's
// weights; the kernels here skip the same ones).
//
// Conventions as in hibag_k_pass2.h / hibag_k_finish.h: lane = sample, every ordered sum is a serial loop inside one lane,
// no fused multiply-add (-ffp-contract=off).  The order of the arithmetic, per size k = sizes[i] and sample:
//   cw_i[c]  = (double)num / den   num, den: integer sums of the sub-model's SNP counts over c's non-missing / all SNPs  (k_prefix_weights = k_pack)
//   S[p]     = 0, then += (cell[c][p] * inv[c]) * cw_i[c] for c = 0 .. k-1 in order, where cw_i[c] > 0                   (k_prefix_accum = k_accum_cells)
//   sum_w    = 0, then += cw_i[c] in the same order                                                                      (= ensemble_scalars)
//   the call = first strict maximum over p of (sum_w > 0 ? S[p] * (1 / sum_w) : S[p]), from 0                            (= finish_call)
//   matching = (sum of tot[c] * cw_i[c]) / (sum of cw_i[c])                                                              (= ensemble_scalars, finish_call)
// dosage and the posterior matrix are not produced (they would be n_sizes matrices).
#ifndef HIBAG_K_PREFIX_H_
#define HIBAG_K_PREFIX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hibag_device.h"

#define PREFIX_WAVES 4                     // k_prefix_accum: wavefronts per workgroup = consecutive sizes of one (tile, sample group)
#ifndef PREFIX_OCC
#define PREFIX_OCC 4                       // workgroups per CU it is compiled for (LDS: 4 x HIBAG_TILE x 64 x 8 = 30,720 bytes each)
#endif
#define PREFIX_NA_INTEGER (-2147483647 - 1)

// (the model's tables through the constant address space: a kernel that stores would otherwise read wave-uniform
// values with vector loads -- hibag_k_engine.h, as_const)
template <class T> using PrefixConst = const __attribute__((address_space(4))) T *;
template <class T> __device__ __forceinline__ PrefixConst<T> prefix_const(const T *p) { return (PrefixConst<T>)(uintptr_t)p; }

struct HibagPrefixView {
	int n_sizes;
	const int *sizes;          // [n_sizes] strictly ascending, 1 .. n_classifier
	const int *row0;           // [n_sizes] first row of size i in `cw` (sum of the sizes before it)
	const int *snp_weight;     // [n_sizes][n_snp] classifiers among the first sizes[i] that use the SNP
	double *cw;                // [sum of sizes][n_pad] row row0[i] + c: weight of classifier c in sub-model i
	double *pbest;             // [n_sizes][n_tile][n_pad] the tile's first strict maximum of the normalised sums ...
	int *pcell;                // ... and its cell (-1: nothing positive)
	int32_t *h1, *h2;          // outputs [n_sizes][ld], the batch's sample 0 at column 0
	double *prob, *matching;
	size_t ld;
};

// k_prefix_weights (behind k_codes / k_pack of the batch): the classifier weights of every sub-model, formed as k_pack
// forms the full model's -- the same integer sums, the same one division.  grid (n_pad / 64, C), thread = sample: the
// classifier's byte codes are read once (3 = missing) and kept as a bit field, the sub-models' SNP counts are wave-uniform.
__global__ __launch_bounds__(64) void k_prefix_weights(HibagModelView M, HibagBatchView B, HibagPrefixView Q,
	const uint8_t *__restrict__ codes)
{
	const int c = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	const int k = prefix_const(M.n_snp_c)[c];
	const PrefixConst<int> idx = prefix_const(M.snp_index) + prefix_const(M.snp_off)[c];
	uint32_t have[4] = {0u, 0u, 0u, 0u};               // bit j: SNP j of the classifier has a genotype (k <= 128)
#pragma unroll
	for (int w = 0; w < 4; w++) {
		const int j1 = min(k, 32 * w + 32);
		for (int j = 32 * w; j < j1; j++)
			have[w] |= (uint32_t)(codes[(size_t)idx[j] * B.n_pad + s] != 3) << (j - 32 * w);
	}
	const PrefixConst<int> sizes = prefix_const(Q.sizes), row0 = prefix_const(Q.row0);
	for (int i = 0; i < Q.n_sizes; i++) {
		if (sizes[i] <= c) continue;                   // the sub-model does not contain the classifier
		const PrefixConst<int> sw = prefix_const(Q.snp_weight) + (size_t)i * M.n_snp;
		int num = 0, den = 0;
#pragma unroll
		for (int w = 0; w < 4; w++) {
			const int j1 = min(k, 32 * w + 32);
			for (int j = 32 * w; j < j1; j++) {
				const int wt = sw[idx[j]];
				den += wt;
				if ((have[w] >> (j - 32 * w)) & 1u) num += wt;
			}
		}
		Q.cw[(size_t)(row0[i] + c) * B.n_pad + s] = (s < B.n_samp && den > 0) ? ((double)num / den) : 0.0;
	}
}

// k_prefix_accum (the hot path; modelled on k_accum_cells, hibag_k_pass2.h): for one size, one tile of cells and 64 samples,
// S[p] += (cell * (1/total)) * w over the sub-model's classifiers in order, from the cell sums pass 1 stored (store mode 1),
// then the tile's first strict maximum of the normalised sums.  Wavefront = (size, tile, 64 samples), the tile's sums in
// LDS; the four wavefronts of a workgroup take four CONSECUTIVE SIZES of one (tile, sample group): they read the same
// rows of stored sums in the same order at about the same time, so three of the four reads come out of the CU's L1, and
// a group's workgroups all go to XCD group % 8 with the sizes fastest, so the other sizes' reads of a tile meet in one L2.
__global__ __launch_bounds__(PREFIX_WAVES * HIBAG_WAVE, PREFIX_OCC) void k_prefix_accum(HibagModelView M, HibagBatchView B, HibagPrefixView Q)
{
	constexpr int CELLS_V = (HIBAG_TILE + 3) / 4 * 4;
	__shared__ double acc_s[PREFIX_WAVES][HIBAG_TILE][HIBAG_WAVE];
	const int n_group = B.n_pad / HIBAG_WAVE;
	const int n_sq = (Q.n_sizes + PREFIX_WAVES - 1) / PREFIX_WAVES;
	const int per_group = M.n_tile * n_sq;
	const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	const int group = (jb / per_group) * 8 + xcd, item = jb % per_group;
	const int tile = item / n_sq, isz = (item % n_sq) * PREFIX_WAVES + wave;
	if (group >= n_group || isz >= Q.n_sizes) return;
	const int s = group * HIBAG_WAVE + lane;
	const int C = prefix_const(Q.sizes)[isz];          // classifiers of this sub-model
	const int ncell = M.tile_n[tile];
	double (*acc)[HIBAG_WAVE] = acc_s[wave];
#pragma unroll
	for (int q = 0; q < HIBAG_TILE; q++) acc[q][lane] = 0;

	typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
	const PrefixConst<u32x8> ct = prefix_const(reinterpret_cast<const u32x8 *>(M.ctile)) + tile;
	const double *__restrict__ const group_rows = B.cells + (size_t)group * (size_t)prefix_const(M.cell_row)[M.n_classifier] * HIBAG_WAVE + lane;
	const double *__restrict__ const cw = Q.cw + (size_t)prefix_const(Q.row0)[isz] * B.n_pad + s;
	struct Visit { u32x8 rec; double w, inv; };
	// what classifier c contributes to the tile: its record, the lane's sub-model weight and 1/total -- requested two classifiers ahead
	auto visit = [&](int c) {
		Visit x;
		x.rec = ct[(size_t)c * M.n_tile];
		x.w = cw[(size_t)c * B.n_pad];
		x.inv = B.inv[(size_t)c * B.n_pad + s];
		return x;
	};
	// the tile's n non-empty cells of the classifier, four at a time (stale rows where pass 1 skipped the (group, classifier):
	// `add` never looks at them)
	auto fetch = [&](const Visit &x, double (&v)[CELLS_V]) {
		const int n = (int)((x.rec[0] >> 8) & 31u);
		const double *__restrict__ rows = group_rows + (size_t)(x.rec[5] & 0x7FFFFFFu) * HIBAG_WAVE;
#pragma unroll
		for (int g = 0; g < HIBAG_TILE; g += 4) {
			if (g >= n) break;
#pragma unroll
			for (int i = g; i < g + 4; i++) v[i] = rows[(size_t)(i < n ? i : n - 1) * HIBAG_WAVE];
		}
	};
	double sum_w = 0;
	auto add = [&](int c, const Visit &x, const double (&v)[CELLS_V]) {
		const bool active = x.w > 0;
		if (active) sum_w += x.w;                    // _Sum_Weight, classifiers in order (src/LibHLA.cpp:1505)
		if (__ballot(active) == 0) return;           // nobody in the group uses the classifier (src/LibHLA.cpp:2451)
		const bool poison = __ballot(active && !(fabs(x.inv) <= 1.79769313486231570815e+308)) != 0;
		const double inv_e = active ? x.inv : 0.0;   // inactive lanes keep their sums: (cell * 0) * 0 = +0
		const int n = (int)((x.rec[0] >> 8) & 31u);
		uint64_t jp = ((uint64_t)x.rec[7] << 32) | x.rec[6];
#pragma unroll
		for (int i = 0; i < HIBAG_TILE; i++) {
			if (i >= n) break;
			__hip_atomic_fetch_add(&acc[(int)(jp & 15)][lane], (v[i] * inv_e) * x.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (ds_add_f64: a plain IEEE addition, as in k_accum_cells)
			jp >>= 4;
		}
		if (poison) {                                // empty cells: (0 * inv) * w is NaN where inv is not finite
			const uint32_t *__restrict__ meta = M.tile_meta + ((size_t)c * M.n_tile + tile) * HIBAG_TILE_META;
			for (int i = n; i < ncell; i++) {
				const double t = (0.0 * x.inv) * x.w;
				acc[meta[4 + i] >> 24][lane] += active ? t : 0.0;
			}
		}
	};

	// two classifiers per turn: while classifier c is added, the cells of c + 1 and the records of c + 2 are in flight
	double va[CELLS_V], vb[CELLS_V];
	Visit x0 = visit(0), x1 = visit(C > 1 ? 1 : 0);
	fetch(x0, va);
	for (int c = 0; c < C; c += 2) {
		const Visit x2 = visit(c + 2 < C ? c + 2 : C - 1);
		if (c + 1 < C) fetch(x1, vb);
		add(c, x0, va);
		const Visit x3 = visit(c + 3 < C ? c + 3 : C - 1);
		if (c + 2 < C) fetch(x2, va);
		if (c + 1 < C) add(c + 1, x1, vb);
		x0 = x2; x1 = x3;
	}

	// NormalizeSumPostProb on the fly, then the tile's part of BestGuessEnsemble (finish_call: first strict maximum from 0)
	const bool scale = sum_w > 0;
	const double ff = 1.0 / sum_w;
	const int p0 = M.tile_p0[tile];
	double best = 0;
	int cell = -1;
	for (int q = 0; q < ncell; q++) {
		const double v = acc[q][lane];
		const double x = scale ? v * ff : v;
		if (best < x) { best = x; cell = p0 + q; }
	}
	const size_t at = ((size_t)isz * M.n_tile + tile) * B.n_pad + s;
	Q.pbest[at] = best;
	Q.pcell[at] = cell;
}

// k_prefix_finish: per (size, sample) the tiles' maxima merged in cell order with the same strict comparison (which
// reproduces the sequential scan, as finish_call's segments do), the called pair's probability, and the matching
// proportion from the ensemble scalars formed as ensemble_scalars forms them, over the sub-model's classifiers.
// grid (n_pad / 64, n_sizes), thread = sample.
__global__ __launch_bounds__(64) void k_prefix_finish(HibagModelView M, HibagBatchView B, HibagPrefixView Q)
{
	const int i = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
	if (s >= B.n_samp) return;
	const int C = prefix_const(Q.sizes)[i];
	const double *__restrict__ cw = Q.cw + (size_t)prefix_const(Q.row0)[i] * B.n_pad + s;
	double sum_m = 0, num_m = 0;
	for (int c0 = 0; c0 < C; c0 += 16) {             // sixteen classifiers' loads in flight, then the sums in classifier order
		double wv[16], tv[16];
#pragma unroll
		for (int j = 0; j < 16; j++) {
			const bool in = c0 + j < C;
			const int c = in ? c0 + j : c0;
			wv[j] = in ? cw[(size_t)c * B.n_pad] : 0.0;
			tv[j] = B.tot[(size_t)c * B.n_pad + s];
		}
#pragma unroll
		for (int j = 0; j < 16; j++) {
			const double w = wv[j];
			if (!(w > 0)) continue;
			sum_m += tv[j] * w;                      // src/LibHLA.cpp:2458
			num_m += w;                              // :2459
		}
	}
	double best = 0;
	int cell = -1;
	for (int t = 0; t < M.n_tile; t++) {
		const size_t at = ((size_t)i * M.n_tile + t) * B.n_pad + s;
		const double b = Q.pbest[at];
		if (best < b) { best = b; cell = Q.pcell[at]; }
	}
	int b1 = PREFIX_NA_INTEGER, b2 = PREFIX_NA_INTEGER;
	if (cell >= 0) {
		// invert p = h2 + h1*(2n-h1-1)/2 (src/LibHLA.cpp:1523)
		int h1 = 0, row = M.n_hla, rem = cell;
		while (rem >= row) { rem -= row; row--; h1++; }
		b1 = h1; b2 = h1 + rem;
	}
	const size_t o = (size_t)i * Q.ld + s;
	Q.h1[o] = b1; Q.h2[o] = b2;
	Q.prob[o] = cell >= 0 ? best : 0.0;
	Q.matching[o] = sum_m / num_m;
}

#endif
