// hibag_k_glmw.h -- kernels of hlaAssocOmnibus: one logistic regression y ~ r_1 + ... + r_d + covariates per SET of feature
// rows of an association handle (all residues of an amino-acid position, all two-digit types, ...), the fit of
// hibag_k_glm.h over a 32-slot design (the definitions of the fit itself are section 23).  Host
// side: hibag_hip_assoc_glm_sets in hibag_assoc.hip.
//
// Slots of a row, fixed per CALL (H = the largest set of the call): 0 the intercept, 1 .. H the h slots (a set's rows in
// the order given; slots past the set's size hold 0), 1 + H .. H + q the covariates, 31 z; 1 + H + q <= 31.  The normal
// matrix X'W[X|z] is 32 x 32: four 16 x 16 blocks, of which (0,0), (1,0) and (1,1) are one v_mfma_f64_16x16x4_f64 each per
// four samples and (0,1) is the transpose of (1,0).
//
// Operand image (k_glm_image_wide, once per call): float64 [kp][32], 256 bytes per sample, with 0 in the h slots and in
// slot 31; rows of padding samples are all zero and their weight is 0, as in hibag_k_glm.h.
//
// Aliased columns: the factorisation goes in the order intercept, covariates, h slots, and a column whose pivot is
// <= 1e-11 A_jj is DROPPED -- it leaves the active set for this and all later solves, its coefficient counts as 0 in
// eta and is reported NaN, flag bit 3 is set -- where k_glm_fit stops.  Only the intercept failing the rule stops a fit.
//
// Order of every sum of a fit: as in hibag_k_glm.h (steps wave, wave + GLM_WAVES, ...; waves added in wave order), so a
// fit's numbers depend on n, its own rows, the covariates, H and compile-time constants -- not on the other fits.  They
// depend on H through eta alone: the 16-lane butterfly pairs other slots when the covariates move (section 26).
#ifndef HIBAG_K_GLMW_H_
#define HIBAG_K_GLMW_H_

#include "hibag_k_glm.h"

#define GLMW_SLOTS 32
#define GLMW_Z 31                   // slot of z
#define GLMW_MAX_ROWS 30            // rows of a set at most (with no covariate)

#define GLM_FLAG_ALIASED 8          // a column was dropped (its values are NaN); the fit went on without it
#define GLM_FLAG_TOO_WIDE 16        // the set does not fit beside the covariates: not fitted

// What a fit reads beside the shared image: the feature rows behind slots 1 .. n_rows (-1: left out, the slot stays 0).
// n_rows == -1 marks a set that is not fitted at all: flags = flags0, NaN everywhere.  flags0 is what the host decided
// (GLM_FLAG_ALIASED for a row it left out).
struct GlmWideFit {
	int n_rows, flags0;
	int rows[GLMW_MAX_ROWS];
};

// k_glm_image_wide: one thread per image element; grid ceil(32 kp / 256), 256 threads.  covar [q][n], weight [n] or NULL.
__global__ void __launch_bounds__(256) k_glm_image_wide(const double *__restrict__ covar, const double *__restrict__ weight, int n, int q,
	int H, int kp, double *__restrict__ img, double *__restrict__ wt)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)kp * GLMW_SLOTS) return;
	const int s = (int)(i >> 5), c = (int)(i & 31);
	double v = 0.0;
	if (s < n) {
		if (c == 0) v = 1.0;
		else if (c >= 1 + H && c < 1 + H + q) v = covar[(size_t)(c - 1 - H) * n + s];
	}
	img[i] = v;
	if (c == 0) wt[s] = s < n ? (weight ? weight[s] : 1.0) : 0.0;
}

// k_glm_fit_wide: one workgroup per fit, GLM_WAVES waves.  Lane l of a wave holds slots l & 15 and 16 + (l & 15) of sample
// 4 step + (l >> 4).  The passes are k_glm_fit's: pass 0 from the start value, pass k >= 1 from eta = X beta_k, each also
// accumulating the tile of the next solve; between passes the three blocks go through one tile buffer per wave, one after
// the other, into s_A, and thread 0 tests convergence, factorises (dropping aliased columns) and solves.
//
// Outputs per fit: coef / se [32] by slot (slot 31, unused and dropped slots NaN), deviance, iterations, flags, df_h (the h
// slots active in the last solve).
__global__ void __launch_bounds__(GLM_WAVES * 64) k_glm_fit_wide(const double *__restrict__ img, const double *__restrict__ wt,
	const int8_t *__restrict__ y, const int8_t *__restrict__ feat, const GlmWideFit *__restrict__ fits, int n, int kp, int q, int H,
	int maxit, double epsilon, double *__restrict__ coef, double *__restrict__ se, double *__restrict__ deviance,
	int32_t *__restrict__ iterations, int32_t *__restrict__ flags, int32_t *__restrict__ df_h)
{
	__shared__ double s_tile[GLM_WAVES][256];   // one block of one wave's tile at a time
	__shared__ double s_A[GLMW_SLOTS * GLMW_SLOTS]; // the waves' tiles added: rows / columns = slots
	__shared__ double s_L[GLMW_SLOTS * GLMW_SLOTS]; // the factor of the last solve, compact (index = position among the active slots)
	__shared__ double s_x[GLMW_SLOTS][GLMW_SLOTS + 1]; // the columns of L^-1, one row per solving lane
	__shared__ double s_beta[GLMW_SLOTS];       // by slot; 0 in unused and dropped slots and in slot 31
	__shared__ double s_u[GLMW_SLOTS];
	__shared__ double s_dev[GLM_WAVES];
	__shared__ double s_out[2];                 // [0] devold, [1] the deviance reported
	__shared__ int s_bnd[GLM_WAVES];
	__shared__ int s_act[GLMW_SLOTS];           // the active slots in factorisation order
	__shared__ int s_state[5];                  // [0] 0 go on, 1 done; [1] flags of the last pass; [2] iterations; [3] active slots; [4] sticky flags

	const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15;
	const GlmWideFit *fit = fits + f;
	const int n_rows = fit->n_rows;
	const double nan = __builtin_nan("");
	if (n_rows < 0) {
		if (tid < GLMW_SLOTS) { coef[(size_t)f * GLMW_SLOTS + tid] = nan; se[(size_t)f * GLMW_SLOTS + tid] = nan; }
		if (tid == 0) { deviance[f] = nan; iterations[f] = 0; flags[f] = fit->flags0; df_h[f] = 0; }
		return;
	}
	if (tid == 0) {
		int p = 0;
		s_act[p++] = 0;
		for (int j = 0; j < q; j++) s_act[p++] = 1 + H + j;
		for (int j = 0; j < n_rows; j++) if (fit->rows[j] >= 0) s_act[p++] = 1 + j;
		s_state[0] = 0; s_state[1] = 0; s_state[2] = 0; s_state[3] = p; s_state[4] = fit->flags0;
	}
	if (tid < GLMW_SLOTS) s_beta[tid] = 0.0;
	__syncthreads();

	// the feature rows behind this lane's two slots (slot c is h slot c - 1, slot 16 + c is h slot 15 + c)
	const int8_t *f_lo = nullptr, *f_hi = nullptr;
	if (c >= 1 && c - 1 < n_rows && fit->rows[c - 1] >= 0) f_lo = feat + (size_t)fit->rows[c - 1] * kp;
	if (c + 15 < n_rows && fit->rows[c + 15] >= 0) f_hi = feat + (size_t)fit->rows[c + 15] * kp;
	const int n_steps = kp >> 2;

	for (int k = 0;; k++) {
		const bool first = k == 0;
		const double beta_lo = s_beta[c], beta_hi = s_beta[16 + c];
		glm_d4 acc[3];
#pragma unroll
		for (int b = 0; b < 3; b++) acc[b] = glm_d4{0.0, 0.0, 0.0, 0.0};
		double dev = 0.0;
		bool bnd = false;
		for (int step = wave; step < n_steps; step += GLM_WAVES) {
			const int s = 4 * step + (lane >> 4);
			const double *row = img + (size_t)s * GLMW_SLOTS;
			double g_lo = row[c], g_hi = row[16 + c];
			if (f_lo) g_lo = (double)f_lo[s];
			if (f_hi) g_hi = (double)f_hi[s];
			const double w0 = wt[s];
			const bool is_case = y[s] != 0;
			const double yy = is_case ? 1.0 : 0.0;
			double eta, mu_dev = 0.0;
			if (first) {
				mu_dev = (w0 * yy + 0.5) / (w0 + 1.0);
				eta = log(mu_dev / (1.0 - mu_dev));
			} else {
				eta = glm_row_sum(g_lo * beta_lo + g_hi * beta_hi);
			}
			double t = exp(eta);
			if (eta < -30.0) t = GLM_EPS;
			if (eta > 30.0) t = 1.0 / GLM_EPS;
			const double mu = t / (1.0 + t);
			if (!first) {
				mu_dev = mu;
				bnd = bnd || (s < n && (mu < 10.0 * GLM_EPS || mu > 1.0 - 10.0 * GLM_EPS));
			}
			dev += (2.0 * w0) * log(1.0 / (is_case ? mu_dev : 1.0 - mu_dev));
			double gp = t / ((1.0 + t) * (1.0 + t));
			if (fabs(eta) > 30.0) gp = GLM_EPS;
			const double v = mu * (1.0 - mu);
			const double z = eta + (yy - mu) / gp;
			const double W = w0 * (gp * gp) / v;
			if (c == 15) g_hi = z;
			const double a_lo = W * g_lo, a_hi = W * g_hi;
			// D[i][j] = sum_k A[i][k] B[k][j]: the a operand names the block's rows, the b operand its columns
			acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_lo, g_lo, acc[0], 0, 0, 0);
			acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_hi, g_lo, acc[1], 0, 0, 0);
			acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_hi, g_hi, acc[2], 0, 0, 0);
		}
		dev += __shfl_xor(dev, 16);
		dev += __shfl_xor(dev, 32);
		const bool any_bnd = __any(bnd);
		if (lane == 0) { s_dev[wave] = dev; s_bnd[wave] = any_bnd; }
		// the blocks (0,0), (1,0), (1,1) one after the other; C/D map of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
		for (int b = 0; b < 3; b++) {
#pragma unroll
			for (int r = 0; r < 4; r++) s_tile[wave][((lane >> 4) + 4 * r) * 16 + c] = acc[b][r];
			__syncthreads();
			if (tid < 256) {
				double a = s_tile[0][tid];
				for (int w = 1; w < GLM_WAVES; w++) a += s_tile[w][tid];
				const int r = tid >> 4, cc = tid & 15;
				if (b == 0) s_A[r * GLMW_SLOTS + cc] = a;
				else if (b == 1) { s_A[(16 + r) * GLMW_SLOTS + cc] = a; s_A[cc * GLMW_SLOTS + 16 + r] = a; }
				else s_A[(16 + r) * GLMW_SLOTS + 16 + cc] = a;
			}
			__syncthreads();
		}
		if (tid == 0) {
			double d = s_dev[0];
			for (int w = 1; w < GLM_WAVES; w++) d += s_dev[w];
			int done = 0;
			if (!first) {
				int b = 0;
				for (int w = 0; w < GLM_WAVES; w++) b |= s_bnd[w];
				const double crit = fabs(d - s_out[0]) / (fabs(d) + 0.1);
				s_out[1] = d;
				s_state[2] = k;
				s_state[1] = b ? GLM_FLAG_BOUNDARY : 0;
				if (crit < epsilon) done = 1;
				else if (k == maxit) { done = 1; s_state[1] |= GLM_FLAG_MAXIT; }
			}
			s_out[0] = d;
			if (!done) {
				// solve k + 1: L L' = A over the active slots, column by column.  Row i of s_L is candidate i of s_act until the
				// candidate is kept, which moves it to the compact row np (np <= i: that row's owner was moved or dropped before).
				const int p = s_state[3];
				int np = 0;
				bool ok = true;
				for (int j = 0; j < p; j++) {
					const int sj = s_act[j];
					const double ajj = s_A[sj * GLMW_SLOTS + sj];
					double dj = ajj;
					for (int m = 0; m < np; m++) dj -= s_L[j * GLMW_SLOTS + m] * s_L[j * GLMW_SLOTS + m];
					if (!(dj > 1e-11 * ajj)) {
						if (sj == 0) { ok = false; break; }
						s_state[4] |= GLM_FLAG_ALIASED;     // dropped: the candidates after it never see this column
						continue;
					}
					const double ljj = sqrt(dj);
					if (np != j)
						for (int m = 0; m < np; m++) s_L[np * GLMW_SLOTS + m] = s_L[j * GLMW_SLOTS + m];
					s_L[np * GLMW_SLOTS + np] = ljj;
					for (int i = j + 1; i < p; i++) {
						double v = s_A[s_act[i] * GLMW_SLOTS + sj];
						for (int m = 0; m < np; m++) v -= s_L[i * GLMW_SLOTS + m] * s_L[np * GLMW_SLOTS + m];
						s_L[i * GLMW_SLOTS + np] = v / ljj;
					}
					s_act[np++] = sj;
				}
				if (!ok) {
					done = 1;
					s_state[1] = GLM_FLAG_RANK;
					s_state[2] = k + 1;
				} else {
					s_state[3] = np;
					double *u = s_u;
					for (int i = 0; i < np; i++) {          // L u = b
						double v = s_A[s_act[i] * GLMW_SLOTS + GLMW_Z];
						for (int m = 0; m < i; m++) v -= s_L[i * GLMW_SLOTS + m] * u[m];
						u[i] = v / s_L[i * GLMW_SLOTS + i];
					}
					for (int i = np - 1; i >= 0; i--) {     // L' beta = u
						double v = u[i];
						for (int m = i + 1; m < np; m++) v -= s_L[m * GLMW_SLOTS + i] * u[m];
						u[i] = v / s_L[i * GLMW_SLOTS + i];
					}
					for (int i = 0; i < GLMW_SLOTS; i++) s_beta[i] = 0.0;
					for (int i = 0; i < np; i++) s_beta[s_act[i]] = u[i];
				}
			}
			s_state[0] = done;
		}
		__syncthreads();
		if (s_state[0]) break;
	}

	// results: the lane of an active slot solves L x = e_j for its column j; (A^-1)_jj is the squared norm of x
	const int p = s_state[3], fl = s_state[1] | s_state[4];
	if (tid < GLMW_SLOTS) {
		double cf = nan, sd = nan;
		int j = -1;
		for (int i = 0; i < p; i++) if (s_act[i] == tid) j = i;
		if (!(fl & GLM_FLAG_RANK) && j >= 0) {
			double ss = 0.0;
			for (int i = j; i < p; i++) {
				double v = i == j ? 1.0 : 0.0;
				for (int m = j; m < i; m++) v -= s_L[i * GLMW_SLOTS + m] * s_x[tid][m];
				v /= s_L[i * GLMW_SLOTS + i];
				s_x[tid][i] = v;
				ss += v * v;
			}
			cf = s_beta[tid];
			sd = sqrt(ss);
		}
		coef[(size_t)f * GLMW_SLOTS + tid] = cf;
		se[(size_t)f * GLMW_SLOTS + tid] = sd;
	}
	if (tid == 0) {
		int dfh = 0;
		for (int i = 0; i < p; i++) dfh += s_act[i] >= 1 && s_act[i] <= H;
		deviance[f] = (fl & GLM_FLAG_RANK) ? nan : s_out[1];
		iterations[f] = s_state[2];
		flags[f] = fl;
		df_h[f] = (fl & GLM_FLAG_RANK) ? 0 : dfh;
	}
}

#endif
