// hibag_k_cox.h -- kernels of hlaAssocSurv: one Cox regression Surv(time, event) ~ h + covariates per test of an association
// handle, the Efron / Breslow partial likelihood with the order of summation swapped.  Host side:
// hibag_assoc.hip.
//
// The samples of the handle are in time order, latest first.  A BLOCK is a maximal run of equal times; the risk set of block
// k is every sample of the blocks 0 .. k, so the sums over risk sets are prefix sums along the samples.  Per evaluation at
// beta a fit needs, with r_j = exp(x_j beta): the prefix sums S_k of r x at the block ends, the sums D_k of r x over a
// block's events, per block the scalars a_k, b_k and the vectors v_kl, the suffix sums A_k of a, the weights
// w_j = r_j (A_b(j) - e_j b_b(j)), and two 16 x 16 Grams: sum_j w_j x_j x_j' and sum_kl v_kl v_kl', each one
// v_mfma_f64_16x16x4_f64 per four samples (or four l).
//
// Slots of a row, fixed: 0 h (het for `genotype`), 1 hom (`genotype` only), 2 .. 1 + q the covariates, 15 the constant: 1 in
// the row of a real sample, 0 in a padding row (i >= n), so that S[15] is S0 and column 15 of the first Gram is sum w x.  A
// slot that a fit does not use holds 0 in every row and stays out of the factorisation (its outputs are NaN).
//
// Order of every sum of a fit (section 31 item 8).  Wave w of the fit's workgroup owns the CONTIGUOUS samples
// [w kp / COX_WAVES, (w + 1) kp / COX_WAVES), its segment.  Prefix sums: the segment's samples one by one from 0, the
// segments' totals one by one in wave order, then S at a sample = (total of the earlier segments) + the segment's samples one
// by one.  A block that crosses a seam is finished by the segment in which it ends; D of such a block is summed one by one
// from the block's first sample.  Over l: in chunks of four, a chunk as (t0 + t1) + (t2 + t3), the chunks one by one.  The
// suffix sums A mirror the prefix sums from the end.  Tiles, log terms and event sums: per wave in walk order, then in wave
// order.  So a fit's numbers depend on n, the blocks and COX_WAVES alone.  No floating-point atomics.
#ifndef HIBAG_K_COX_H_
#define HIBAG_K_COX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define COX_WAVES 8                 // waves of a fit's workgroup
#define COX_SLOTS 16
#define COX_COV0 2                  // slot of the first covariate
#define COX_ONE 15                  // slot of the constant
#define COX_STEP 4                  // samples of one MFMA step
#define COX_ETA_MAX 200.0           // eta is clamped to [-200, 200]

#define COX_FLAG_MAXIT 1            // not converged within maxit
#define COX_FLAG_RANK 2             // a failing pivot, a column that cannot be fitted, no event: the values are NaN
#define COX_FLAG_CLAMP 4            // an eta outside [-200, 200] was clamped in some evaluation
#define COX_FLAG_DECREASE 8         // the log-likelihood decreased in an iteration that did not converge

#define COX_TIES_EFRON 0
#define COX_TIES_BRESLOW 1

typedef double cox_d4 __attribute__((ext_vector_type(4)));

// What a fit reads beside the shared image: the feature rows behind slots 0 and 1 (-1: the slot is unused); row_a == -2
// marks a fit that is not run at all (flags = COX_FLAG_RANK, NaN everywhere).
struct CoxFit {
	int row_a, row_b;
};

// The block table of a call, from the times: blk [kp] the block of a sample (0 for padding), first [kp + 1] the first sample
// of a block (first[n_block] = n), dk [kp] the events of a block.
struct CoxTable {
	const int32_t *blk, *first, *dk;
};

// k_cox_image: the operand image float64 [kp][16] (workgroups 0 .. gridDim.x - 2, one thread per element) and the block
// table (the last workgroup).  covar [q][n], already centred; time [n] not increasing; y [kp] the event indicator.
// The table's sums are integer scans: thread t takes the samples [t c, (t + 1) c), c = ceil(n / 256); the threads' counts
// are added by thread 0.  `scan` [2 kp] is scratch: the events up to and including a sample, then per block up to its end.
__global__ void __launch_bounds__(256) k_cox_image(const double *__restrict__ covar, const double *__restrict__ time,
	const int8_t *__restrict__ y, int n, int q, int kp, double *__restrict__ img, int32_t *__restrict__ blk, int32_t *__restrict__ first,
	int32_t *__restrict__ dk, int32_t *__restrict__ scan)
{
	if (blockIdx.x + 1 < gridDim.x) {
		const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
		if (i >= (size_t)kp * COX_SLOTS) return;
		const int s = (int)(i >> 4), c = (int)(i & 15);
		double v = 0.0;
		if (s < n) {
			if (c == COX_ONE) v = 1.0;
			else if (c >= COX_COV0 && c < COX_COV0 + q) v = covar[(size_t)(c - COX_COV0) * n + s];
		}
		img[i] = v;
		return;
	}
	__shared__ int s_new[256], s_ev[256];
	const int t = threadIdx.x, chunk = (n + 255) / 256;
	const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
	int32_t *ev_at = scan, *ev_end = scan + kp;
	int c_new = 0, c_ev = 0;
	for (int s = lo; s < hi; s++) {
		c_new += s == 0 || time[s] != time[s - 1];
		c_ev += y[s] != 0;
	}
	s_new[t] = c_new; s_ev[t] = c_ev;
	__syncthreads();
	if (t == 0) {
		int a = 0, b = 0;
		for (int i = 0; i < 256; i++) {
			const int ca = s_new[i], cb = s_ev[i];
			s_new[i] = a; s_ev[i] = b;
			a += ca; b += cb;
		}
		first[a] = n;                                         // a = the number of blocks
	}
	__syncthreads();
	c_new = s_new[t]; c_ev = s_ev[t];
	for (int s = lo; s < hi; s++) {
		if (s == 0 || time[s] != time[s - 1]) first[c_new++] = s;
		c_ev += y[s] != 0;
		blk[s] = c_new - 1;
		ev_at[s] = c_ev;
		if (s == n - 1 || time[s + 1] != time[s]) ev_end[c_new - 1] = c_ev;
	}
	for (int s = n + t; s < kp; s += 256) blk[s] = 0;
	__syncthreads();
	for (int s = lo; s < hi; s++)
		if (s == n - 1 || time[s + 1] != time[s]) {
			const int k = blk[s];
			dk[k] = ev_at[s] - (k > 0 ? ev_end[k - 1] : 0);
		}
}

// The sum of v over the 16 lanes of a sample, the same bits in all of them.
__device__ __forceinline__ double cox_row_sum(double v)
{
	v += __shfl_xor(v, 1);
	v += __shfl_xor(v, 2);
	v += __shfl_xor(v, 4);
	v += __shfl_xor(v, 8);
	return v;
}

// (t0 + t1) + (t2 + t3) over the four sample groups of a wave, the same bits in all of them.
__device__ __forceinline__ double cox_group_sum(double v)
{
	v += __shfl_xor(v, 16);
	v += __shfl_xor(v, 32);
	return v;
}

// One block's terms (a wave, all lanes): S, D hold slot `lane & 15` of the prefix sum at the block's end and of the sum over
// its d > 0 events.  Lane group g takes l = l0 + g of every chunk of four.  Adds the v v' of the chunk to `acc` and the
// log phi to `ll_phi`; returns a_k and b_k.
__device__ __forceinline__ void cox_block(double S, double D, int d, int ties, int lane, cox_d4 &acc, double &ll_phi, double &a_k, double &b_k)
{
	const int g = lane >> 4;
	const double S0 = __shfl(S, (lane & 48) | COX_ONE), D0 = __shfl(D, (lane & 48) | COX_ONE);
	double a = 0.0, b = 0.0;
	for (int l0 = 0; l0 < d; l0 += COX_STEP) {
		const int l = l0 + g;
		const bool live = l < d;
		const double f = ties == COX_TIES_EFRON ? (double)l / (double)d : 0.0;
		const double phi = S0 - f * D0;
		const double v = live ? (S - f * D) / phi : 0.0;
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
		a += cox_group_sum(live ? 1.0 / phi : 0.0);
		b += cox_group_sum(live ? f / phi : 0.0);
		ll_phi += cox_group_sum(live ? log(phi) : 0.0);
	}
	a_k = a; b_k = b;
}

// k_cox_fit: one workgroup per fit, COX_WAVES waves.  Lane l of a wave holds slot l & 15 of sample 4 step + (l >> 4).
//
// An evaluation at beta (section 31 item 4) is four walks of a wave over its segment, with workgroup barriers between them:
// 1. eta, r (kept in `scr`), the segment's totals of r x, of the events' eta and of the events' x; then the exclusive
//    prefix over the segments from LDS;
// 2. sample by sample the running S and D; at the end of a block with events, cox_block: a_k, b_k to `scr`, the log terms,
//    the correction Gram;
// 3. the exclusive suffix over the segments' totals of a_k;
// 4. backwards, sample by sample the running A; per step one MFMA with a = w x, b = x.
// Then the waves' tiles are added in wave order and thread 0 tests convergence, factorises I = G - V over the used slots
// (column order, pivot rule 1e-11 G_jj) and takes the Newton step.  The factor of the LAST solve stays in LDS; the standard
// errors come from it after the loop.  After the first factorisation thread 0 also forms the score statistic of the h slots.
//
// start [16] by slot: where the fit starts.  scr: 3 kp doubles per fit of the launch (r by sample; a, b by block).
// Outputs per fit: coef / se [16] in slot order (unused slots NaN), loglik, score, iterations, flags.
__global__ void __launch_bounds__(COX_WAVES * 64) k_cox_fit(const double *__restrict__ img, const int8_t *__restrict__ y,
	const int8_t *__restrict__ feat, const CoxFit *__restrict__ fits, CoxTable tab, const double *__restrict__ start, int n, int kp, int q,
	int ties, int maxit, double epsilon, double *scr, double *__restrict__ coef, double *__restrict__ se,
	double *__restrict__ loglik, double *__restrict__ score, int32_t *__restrict__ iterations, int32_t *__restrict__ flags)
{
	__shared__ double s_G[COX_WAVES][256];      // the waves' tiles of sum w x x'
	__shared__ double s_V[COX_WAVES][256];      // the waves' tiles of sum v v'
	__shared__ double s_I[256];                 // G - V: rows / columns = slots
	__shared__ double s_Gd[COX_SLOTS];          // the diagonal of G: the scale a pivot of G - V is judged against
	__shared__ double s_T[COX_WAVES][COX_SLOTS]; // the segments' totals of r x
	__shared__ double s_ex[COX_WAVES][COX_SLOTS]; // the segments' sums of the events' x
	__shared__ double s_eta[COX_WAVES], s_phi[COX_WAVES], s_a[COX_WAVES];
	__shared__ int s_clamp[COX_WAVES];
	__shared__ double s_L[COX_SLOTS * COX_SLOTS]; // the factor of the last solve, compact (index = position among the used slots)
	__shared__ double s_beta[COX_SLOTS];        // by slot; 0 in unused slots
	__shared__ double s_U[COX_SLOTS];           // by slot
	__shared__ int s_act[COX_SLOTS];            // the used slots in column order
	__shared__ int s_state[4];                  // [0] 0 go on, 1 done; [1] flags; [2] iterations; [3] used slots
	__shared__ double s_x[COX_SLOTS][COX_SLOTS + 1]; // the columns of L^-1, one row per solving lane
	__shared__ double s_u[COX_SLOTS];
	__shared__ double s_out[3];                 // [0] the previous log-likelihood, [1] the one reported, [2] the score statistic

	const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
	const CoxFit fit = fits[f];
	const double nan = __builtin_nan("");
	if (fit.row_a == -2) {
		if (tid < COX_SLOTS) { coef[(size_t)f * COX_SLOTS + tid] = nan; se[(size_t)f * COX_SLOTS + tid] = nan; }
		if (tid == 0) { loglik[f] = nan; score[f] = nan; iterations[f] = 0; flags[f] = COX_FLAG_RANK; }
		return;
	}
	if (tid == 0) {
		int p = 0;
		if (fit.row_a >= 0) s_act[p++] = 0;
		if (fit.row_b >= 0) s_act[p++] = 1;
		for (int j = 0; j < q; j++) s_act[p++] = COX_COV0 + j;
		s_state[0] = 0; s_state[1] = 0; s_state[2] = 0; s_state[3] = p;
		s_out[2] = nan;
	}
	if (tid < COX_SLOTS) s_beta[tid] = (tid >= COX_COV0 && tid < COX_COV0 + q) ? start[tid] : 0.0;
	__syncthreads();

	const int8_t *fa = fit.row_a >= 0 ? feat + (size_t)fit.row_a * kp : nullptr;
	const int8_t *fb = fit.row_b >= 0 ? feat + (size_t)fit.row_b * kp : nullptr;
	const int seg_steps = (kp / COX_STEP) / COX_WAVES;      // kp is a multiple of 128
	const int step0 = wave * seg_steps, step1 = step0 + seg_steps;
	double *r_of = scr + (size_t)blockIdx.x * 3 * kp, *a_of = r_of + kp, *b_of = a_of + kp;

	// the row of the lane's sample at `step`
#define COX_ROW(step, s, x)                                              \
	const int s = COX_STEP * (step) + g;                                 \
	double x = img[(size_t)(step) * 64 + lane];                          \
	if (c == 0 && fa) x = (double)fa[s];                                 \
	if (c == 1 && fb) x = (double)fb[s];

	for (int k = 0;; k++) {
		const double beta_c = s_beta[c];

		// walk 1: eta, r, the segment's totals
		{
			double T = 0.0, ev_eta = 0.0, ev_x = 0.0;
			bool clamp = false;
			for (int step = step0; step < step1; step++) {
				COX_ROW(step, s, x)
				double eta = cox_row_sum(x * beta_c);
				if (eta < -COX_ETA_MAX) { eta = -COX_ETA_MAX; clamp = clamp || s < n; }
				if (eta > COX_ETA_MAX) { eta = COX_ETA_MAX; clamp = clamp || s < n; }
				const double r = exp(eta);
				if (c == 0) r_of[s] = r;
				const bool ev = y[s] != 0;
				ev_eta += ev ? eta : 0.0;
				ev_x += ev ? x : 0.0;
				const double u = r * x;
#pragma unroll
				for (int gg = 0; gg < COX_STEP; gg++) T += __shfl(u, 16 * gg + c);
			}
			ev_eta = cox_group_sum(ev_eta);
			ev_x = cox_group_sum(ev_x);
			const bool any_clamp = __any(clamp);
			if (g == 0) { s_T[wave][c] = T; s_ex[wave][c] = ev_x; }
			if (lane == 0) { s_eta[wave] = ev_eta; s_clamp[wave] = any_clamp; }
		}
		__syncthreads();

		// walk 2: the blocks that end in the segment
		{
			double R = 0.0, D = 0.0, ll_phi = 0.0, a_tot = 0.0;
			cox_d4 acc = {0.0, 0.0, 0.0, 0.0};
			for (int w = 0; w < wave; w++) R += s_T[w][c];
			const int s_first = COX_STEP * step0;
			if (s_first > 0 && s_first < n) {
				// a block that began before the seam and ends in this segment: its events so far, from its first sample
				const int kb = tab.blk[s_first];
				const int b0 = tab.first[kb], b1 = tab.first[kb + 1];
				if (b0 < s_first && b1 <= COX_STEP * step1 && tab.dk[kb] > 0) {
					for (int step = b0 / COX_STEP; step < step0; step++) {
						COX_ROW(step, s, x)
						const double u = r_of[s] * x;
						const int ev = s >= b0 && y[s] != 0;
#pragma unroll
						for (int gg = 0; gg < COX_STEP; gg++) {
							const double ug = __shfl(u, 16 * gg + c);
							if (__builtin_amdgcn_readlane(ev, 16 * gg)) D += ug;
						}
					}
				}
			}
			for (int step = step0; step < step1; step++) {
				COX_ROW(step, s, x)
				const double u = r_of[s] * x;
				const int ev = y[s] != 0;
				const int kb = tab.blk[s];
				const int is_end = s < n && tab.first[kb + 1] == s + 1;
				const int d = is_end ? tab.dk[kb] : 0;
				const unsigned long long ends = __ballot(is_end);
#pragma unroll
				for (int gg = 0; gg < COX_STEP; gg++) {
					const double ug = __shfl(u, 16 * gg + c);
					R += ug;
					if (__builtin_amdgcn_readlane(ev, 16 * gg)) D += ug;
					if ((ends >> (16 * gg)) & 1) {
						const int dd = __builtin_amdgcn_readlane(d, 16 * gg), kk = __builtin_amdgcn_readlane(kb, 16 * gg);
						double a_k = 0.0, b_k = 0.0;
						if (dd > 0) cox_block(R, D, dd, ties, lane, acc, ll_phi, a_k, b_k);
						if (lane == 0) { a_of[kk] = a_k; b_of[kk] = b_k; }
						a_tot += a_k;
						D = 0.0;
					}
				}
			}
#pragma unroll
			for (int r = 0; r < 4; r++) s_V[wave][(g + 4 * r) * 16 + c] = acc[r];
			if (lane == 0) { s_phi[wave] = ll_phi; s_a[wave] = a_tot; }
		}
		__syncthreads();

		// walks 3 and 4: the suffix sums of a, the weights, the Gram
		{
			double A = 0.0, my_A = 0.0;
			cox_d4 acc = {0.0, 0.0, 0.0, 0.0};
			for (int w = COX_WAVES - 1; w > wave; w--) A += s_a[w];
			for (int step = step1 - 1; step >= step0; step--) {
				COX_ROW(step, s, x)
				const int kb = tab.blk[s];
				const int is_end = s < n && tab.first[kb + 1] == s + 1;
				const double a_k = a_of[kb], b_k = b_of[kb];
				const unsigned long long ends = __ballot(is_end);
#pragma unroll
				for (int gg = COX_STEP - 1; gg >= 0; gg--) {
					const double ag = __shfl(a_k, 16 * gg);
					if ((ends >> (16 * gg)) & 1) A += ag;
					if (g == gg) my_A = A;
				}
				const double w = r_of[s] * (y[s] != 0 ? my_A - b_k : my_A);
				acc = __builtin_amdgcn_mfma_f64_16x16x4f64(w * x, x, acc, 0, 0, 0);
			}
			// C/D map of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
			for (int r = 0; r < 4; r++) s_G[wave][(g + 4 * r) * 16 + c] = acc[r];
		}
		__syncthreads();
		if (tid < 256) {
			double G = s_G[0][tid], V = s_V[0][tid];
			for (int w = 1; w < COX_WAVES; w++) { G += s_G[w][tid]; V += s_V[w][tid]; }
			s_I[tid] = G - V;
			if ((tid >> 4) == (tid & 15)) s_Gd[tid >> 4] = G;
			if ((tid & 15) == COX_ONE) {
				const int i = tid >> 4;
				double ex = s_ex[0][i];
				for (int w = 1; w < COX_WAVES; w++) ex += s_ex[w][i];
				s_U[i] = ex - G;
			}
		}
		__syncthreads();
		if (tid == 0) {
			double e = s_eta[0], ph = s_phi[0];
			int cl = s_clamp[0];
			for (int w = 1; w < COX_WAVES; w++) { e += s_eta[w]; ph += s_phi[w]; cl |= s_clamp[w]; }
			const double ll = e - ph;
			const int p = s_state[3];
			int done = 0;
			if (cl) s_state[1] |= COX_FLAG_CLAMP;
			if (k > 0) {
				s_state[2] = k;
				if (fabs(1.0 - s_out[0] / ll) <= epsilon) done = 1;
				else {
					if (ll < s_out[0]) s_state[1] |= COX_FLAG_DECREASE;      // (a decrease within epsilon is convergence)
					if (k == maxit) { done = 1; s_state[1] |= COX_FLAG_MAXIT; }
				}
			} else if (p == 0) {
				done = 1;
			}
			s_out[0] = ll;
			s_out[1] = ll;
			if (!done) {
				// solve k + 1: L L' = I over the used slots, column by column
				bool ok = true;
				for (int j = 0; j < p && ok; j++) {
					const int sj = s_act[j];
					double dj = s_I[sj * 16 + sj];
					for (int m = 0; m < j; m++) dj -= s_L[j * 16 + m] * s_L[j * 16 + m];
					// against G_jj, what the subtraction cancelled: an information that is rounding noise fails in every precision
					if (!(dj > 1e-11 * s_Gd[sj])) { ok = false; break; }
					const double ljj = sqrt(dj);
					s_L[j * 16 + j] = ljj;
					for (int i = j + 1; i < p; i++) {
						double v = s_I[s_act[i] * 16 + sj];
						for (int m = 0; m < j; m++) v -= s_L[i * 16 + m] * s_L[j * 16 + m];
						s_L[i * 16 + j] = v / ljj;
					}
				}
				if (!ok) {
					done = 1;
					s_state[1] = COX_FLAG_RANK;
					s_state[2] = k + 1;
				} else {
					double *u = s_u;
					for (int i = 0; i < p; i++) {           // L u = U
						double v = s_U[s_act[i]];
						for (int m = 0; m < i; m++) v -= s_L[i * 16 + m] * u[m];
						u[i] = v / s_L[i * 16 + i];
					}
					for (int i = p - 1; i >= 0; i--) {      // L' delta = u
						double v = u[i];
						for (int m = i + 1; m < p; m++) v -= s_L[m * 16 + i] * u[m];
						u[i] = v / s_L[i * 16 + i];
					}
					for (int i = 0; i < p; i++) s_beta[s_act[i]] += u[i];
					if (k == 0) {
						// the score statistic U_h' (I^-1)_hh U_h: (I^-1)_ij = the dot product of columns i and j of L^-1
						const int d = (fit.row_a >= 0) + (fit.row_b >= 0);
						for (int j = 0; j < d; j++)
							for (int i = j; i < p; i++) {
								double v = i == j ? 1.0 : 0.0;
								for (int m = j; m < i; m++) v -= s_L[i * 16 + m] * s_x[j][m];
								s_x[j][i] = v / s_L[i * 16 + i];
							}
						double st = 0.0;
						for (int i = 0; i < d; i++)
							for (int j = 0; j < d; j++) {
								double m_ij = 0.0;
								for (int m = (i > j ? i : j); m < p; m++) m_ij += s_x[i][m] * s_x[j][m];
								st += s_U[s_act[i]] * m_ij * s_U[s_act[j]];
							}
						if (d > 0) s_out[2] = st;
					}
				}
			}
			s_state[0] = done;
		}
		__syncthreads();
		if (s_state[0]) break;
	}
#undef COX_ROW

	// results: the lane of a used slot solves L x = e_j for its column j; (I^-1)_jj is the squared norm of x
	const int p = s_state[3], fl = s_state[1];
	if (tid < COX_SLOTS) {
		double cf = nan, sd = nan;
		int j = -1;
		for (int i = 0; i < p; i++) if (s_act[i] == tid) j = i;
		if (!(fl & COX_FLAG_RANK) && j >= 0) {
			double ss = 0.0;
			for (int i = j; i < p; i++) {
				double v = i == j ? 1.0 : 0.0;
				for (int m = j; m < i; m++) v -= s_L[i * 16 + m] * s_x[tid][m];
				v /= s_L[i * 16 + i];
				s_x[tid][i] = v;
				ss += v * v;
			}
			cf = s_beta[tid];
			sd = sqrt(ss);
		}
		coef[(size_t)f * COX_SLOTS + tid] = cf;
		se[(size_t)f * COX_SLOTS + tid] = sd;
	}
	if (tid == 0) {
		loglik[f] = (fl & COX_FLAG_RANK) ? nan : s_out[1];
		score[f] = (fl & COX_FLAG_RANK) ? nan : s_out[2];
		iterations[f] = s_state[2];
		flags[f] = fl;
	}
}

#endif
