// hibag_k_merge.h -- the kernels of hibag_merge.hip (included there): hlaPredMerge (R/HIBAG.R:825-1023 around HIBAG_SumList,
// HIBAG_UpdateAddProbW and HIBAG_NormalizeProb, src/HIBAG.cpp:1455-1547) as a device operation over the posteriors of k
// models of one locus.
//
// Conventions as in hibag_k_finish.h: lane = sample, so every ordered sum is a serial loop inside one lane and nothing is
// reduced across lanes; no fused multiply-add (-ffp-contract=off); a scan for a maximum may be cut into segments that are
// merged in order, a floating-point sum may not.  All matrices the kernels write are row-major [row][n_pad] with the sample
// fastest: loads and stores of a wavefront are 512 contiguous bytes.
//
// The order of the arithmetic (what makes the result bit-equal to hlaPredMerge on the k posterior matrices):
//   matching[s] = 0.0, then += w[i] * matching_i[s] for model i ascending                           (k_merge_rows)
//   w2_i[s]     = w[i] * matching_i[s] if use_matching, else w[i]
//   acc[r][s]   = 0.0, then += p_i[j][s] * w2_i[s] over the gather list of merged row r -- (model, source cell) in model
//                 order, then ascending cell; product rounded, then the sum                            (k_merge_rows)
//   total[s]    = 0.0, then += acc[r][s] for r ascending                                              (k_merge_total)
//   prob[r][s]  = acc[r][s] / total[s], an IEEE division; the call = the first maximum in row order, NaN read as -inf
//                 (a column of NaN: row 0 and a NaN probability)                                      (k_merge_call)
//   dosage[a][s] = (sum of prob over the rows whose first name is a, ascending) + (the same for the second name)
//                                                                                                      (k_merge_dosage)
// Row r = (i, j), i <= j, of the n merged alleles is named a[j]/a[i] and sits at j + i (2n - i - 1) / 2: its first name is
// j (h2 / allele2), its second i (h1 / allele1).  The rows whose first name is a are (0, a), (1, a), ..., (a, a); those whose
// second name is a are the contiguous run (a, a) ... (a, n - 1): the diagonal row is in both lists.
#ifndef HIBAG_K_MERGE_H_
#define HIBAG_K_MERGE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HIBAG_MERGE_MAX_MODELS 16          // the sources travel as kernel arguments
#define MRG_ROW_WAVES 4                    // k_merge_rows: wavefronts per workgroup ...
#define MRG_ROWS 64                        // ... which share this many merged rows
#define MRG_SEG 16                         // k_merge_call / k_merge_dosage: segments (alleles) per workgroup

// Where the k posteriors come from.
//   part != 0: src[i] is model i's un-normalised ensemble sums [n_cell_i + 3][n_pad] (HibagBatchView::part); the posterior
//              and the matching proportion are formed on the fly exactly as k_finish_prob / finish_call form them.
//   part == 0: src[i] is the sample-major posterior matrix [n_samp][n_cell_i] hibag_hip_predict_device wrote, mt[i] its
//              matching vector [n_samp] (lane = sample reads it with a stride of n_cell_i doubles).
struct HibagMergeSrc {
	const double *src[HIBAG_MERGE_MAX_MODELS];
	const double *mt[HIBAG_MERGE_MAX_MODELS];
	double w[HIBAG_MERGE_MAX_MODELS];      // normalised weights
	int n_cell[HIBAG_MERGE_MAX_MODELS];
	int n_models;
	int use_matching;
};

struct HibagMergePlanView {
	const int *row_off;                    // [n_row + 1] gather lists of the merged rows (CSR) ...
	const uint32_t *ent;                   // ... entries: model << 24 | source cell
	int n_hla, n_row;                      // merged alleles n, rows n (n + 1) / 2
};

// k_merge_rows: steps 2-4.  Workgroup = 64 samples x MRG_ROWS merged rows, wavefront w takes rows w, w + 4, ...; the
// per-model, per-sample factors are formed once per workgroup and kept in LDS.  The gather entries are wave-uniform (scalar
// loads); with part != 0 each term is one coalesced load.
template <bool PART>
__global__ __launch_bounds__(64 * MRG_ROW_WAVES) void k_merge_rows(HibagMergePlanView Q, HibagMergeSrc S, int n_samp, int n_pad,
	double *__restrict__ acc, double *__restrict__ matching_out)
{
	__shared__ double w2_s[HIBAG_MERGE_MAX_MODELS][64];
	__shared__ double ff_s[PART ? HIBAG_MERGE_MAX_MODELS : 1][64];
	__shared__ double sw_s[PART ? HIBAG_MERGE_MAX_MODELS : 1][64];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const int s = blockIdx.x * 64 + lane;
	const int sc = min(s, n_samp - 1);           // (sample-major sources end at n_samp: the padding lanes read the last sample)
	const size_t np = (size_t)n_pad;
	if (wave == 0) {
		double m = 0.0;
		for (int i = 0; i < S.n_models; i++) {
			double mt;
			if (PART) {
				const double *__restrict__ part = S.src[i];
				const size_t P = (size_t)S.n_cell[i];
				const double sum_w = part[P * np + s];
				sw_s[i][lane] = sum_w;
				ff_s[i][lane] = 1.0 / sum_w;
				mt = part[(P + 1) * np + s] / part[(P + 2) * np + s];
			} else {
				mt = S.mt[i][sc];
			}
			const double wm = S.w[i] * mt;
			m += wm;
			w2_s[i][lane] = S.use_matching ? wm : S.w[i];
		}
		if (blockIdx.y == 0 && matching_out && s < n_samp) matching_out[s] = m;
	}
	__syncthreads();
	const int r1 = min(Q.n_row, ((int)blockIdx.y + 1) * MRG_ROWS);
	for (int r = blockIdx.y * MRG_ROWS + wave; r < r1; r += MRG_ROW_WAVES) {
		const int e1 = Q.row_off[r + 1];
		double a = 0.0;
		for (int e = Q.row_off[r]; e < e1; e++) {
			const uint32_t u = Q.ent[e];
			const int i = (int)(u >> 24);
			const size_t j = u & 0xffffffu;
			double p;
			if (PART) {
				const double v = S.src[i][j * np + s];
				const double sum_w = sw_s[i][lane];
				p = sum_w != sum_w ? sum_w : (sum_w > 0 ? v * ff_s[i][lane] : v);      // (k_finish_prob's posterior)
			} else {
				p = S.src[i][(size_t)sc * (size_t)S.n_cell[i] + j];
			}
			a += p * w2_s[i][lane];
		}
		acc[(size_t)r * np + s] = a;
	}
}

// k_merge_total: step 5's column sums, one wavefront per 64 samples, sixteen rows in flight, added in row order.
__global__ __launch_bounds__(64) void k_merge_total(int n_row, int n_pad, const double *__restrict__ acc, double *__restrict__ total)
{
	const int s = blockIdx.x * 64 + threadIdx.x;
	const size_t np = (size_t)n_pad;
	double t = 0.0;
	int r = 0;
	for (; r + 16 <= n_row; r += 16) {
		double v[16];
#pragma unroll
		for (int j = 0; j < 16; j++) v[j] = acc[(size_t)(r + j) * np + s];
#pragma unroll
		for (int j = 0; j < 16; j++) t += v[j];
	}
	for (; r < n_row; r++) t += acc[(size_t)r * np + s];
	total[s] = t;
}

// k_merge_call: the division of step 5, in place, and step 6.  Workgroup = 64 samples x MRG_SEG segments of the row range;
// every thread divides and scans its segment in row order, then the segments are merged in order with the same strict
// comparison, which reproduces the sequential scan (finish_call's scheme).
__global__ __launch_bounds__(64 * MRG_SEG) void k_merge_call(int n_hla, int n_row, int n_samp, int n_pad,
	double *__restrict__ prob, const double *__restrict__ total, int32_t *__restrict__ H1, int32_t *__restrict__ H2,
	double *__restrict__ max_prob)
{
	__shared__ double key_s[MRG_SEG][64], val_s[MRG_SEG][64];
	__shared__ int row_s[MRG_SEG][64];
	const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
	const int s = blockIdx.x * 64 + lane;
	const size_t np = (size_t)n_pad;
	const double t = total[s];
	const int per = (n_row + MRG_SEG - 1) / MRG_SEG;
	const int lo = seg * per, hi = min(n_row, lo + per);
	const double ninf = -__builtin_huge_val();
	double key = ninf, val = 0.0;
	int row = -1;                                  // (an empty segment takes no part in the merge)
	for (int r = lo; r < hi; r++) {
		const double v = prob[(size_t)r * np + s] / t;
		prob[(size_t)r * np + s] = v;
		const double x = v != v ? ninf : v;
		if (row < 0 || key < x) { key = x; val = v; row = r; }
	}
	key_s[seg][lane] = key;
	val_s[seg][lane] = val;
	row_s[seg][lane] = row;
	__syncthreads();
	if (seg != 0 || s >= n_samp) return;
	for (int g = 1; g < MRG_SEG; g++)
		if (row_s[g][lane] >= 0 && key < key_s[g][lane]) { key = key_s[g][lane]; val = val_s[g][lane]; row = row_s[g][lane]; }
	if (H1) {
		int i = 0, len = n_hla, rem = row;
		while (rem >= len) { rem -= len; len--; i++; }
		H1[s] = i;                                 // the row's second name
		H2[s] = i + rem;                           // its first name
	}
	if (max_prob) max_prob[s] = val;
}

// k_merge_dosage: step 7, thread = (sample, merged allele); dosage is [n_hla][ld], allele-major like hlaPredMerge's matrix.
__global__ __launch_bounds__(64 * MRG_SEG) void k_merge_dosage(int n_hla, int n_samp, int n_pad,
	const double *__restrict__ prob, double *__restrict__ dosage, size_t ld)
{
	const int s = blockIdx.x * 64 + (threadIdx.x & 63);
	const int a = blockIdx.y * MRG_SEG + (threadIdx.x >> 6);
	if (s >= n_samp || a >= n_hla) return;
	const size_t np = (size_t)n_pad;
	const size_t n = (size_t)n_hla;
	double first = 0.0, second = 0.0;
#pragma unroll 8
	for (size_t i = 0; i <= (size_t)a; i++) first += prob[((size_t)a + i * (2 * n - i - 1) / 2) * np + s];
	const size_t diag = (size_t)a + (size_t)a * (2 * n - (size_t)a - 1) / 2;
#pragma unroll 8
	for (size_t j = 0; j < n - (size_t)a; j++) second += prob[(diag + j) * np + s];
	dosage[(size_t)a * ld + s] = first + second;
}

#endif
