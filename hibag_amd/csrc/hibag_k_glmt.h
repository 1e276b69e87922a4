// hibag_k_glmt.h -- kernels of hlaAssocInteract: one logistic regression per FIT RECORD of up to three terms beside the
// covariates, a term being a feature row of an association handle or the PRODUCT of two rows, formed while the samples are
// walked (the definitions of the fit itself are section 23, the drop rule section 26 item 2).  Host
// side: hibag_hip_assoc_glm_terms in hibag_assoc.hip.
//
// Slots of a row, fixed: 0 the intercept, 1 .. 3 the terms, 4 .. 3 + q the covariates (q <= 11), 15 z.  A slot that a fit
// does not use holds 0 in every row.  The layout does not move with the call, so a fit's bits depend on n, its own terms,
// the covariates and the arguments -- there is no H as in hibag_k_glmw.h.
//
// Operand image (k_glm_image_terms, once per call): float64 [kp][16], 128 bytes per sample, with 0 in slots 1 .. 3 and 15;
// rows of padding samples are all zero and their weight is 0, as in hibag_k_glm.h.
//
// Terms: the lane of slot 1 + j keeps the one or two row pointers of term j.  (a, -1) is the row itself, (a, b) the product
// feat[a][s] * feat[b][s] as an integer (the rows hold 0 / 1 / 2), converted to double: exact.  No product row is ever
// written to memory.
//
// Aliased columns: the factorisation goes in the order intercept, covariates, terms in slot order (a product comes after
// its factors), and a column whose pivot is <= 1e-11 A_jj is DROPPED as in hibag_k_glmw.h.  Only the intercept failing the
// rule stops a fit.
//
// Order of every sum of a fit: as in hibag_k_glm.h (steps wave, wave + GLM_WAVES, ...; waves added in wave order).
#ifndef HIBAG_K_GLMT_H_
#define HIBAG_K_GLMT_H_

#include "hibag_k_glmw.h"

#define GLMT_TERMS 3                // term slots 1 .. 3
#define GLMT_COV0 4                 // slot of the first covariate
#define GLMT_MAX_COVAR 11
#define GLMT_Z 15                   // slot of z

// What a fit reads beside the shared image: term j stands behind slot 1 + j; (-1, -1) unused, (a, -1) row a, (a, b) the
// product of rows a and b.  fitted == 0 marks a record that is not fitted at all: flags = flags0, NaN everywhere.  flags0 is
// what the host decided (GLM_FLAG_ALIASED for a term it left out).
struct GlmTermsFit {
	int term[GLMT_TERMS][2];
	int fitted, flags0;
};

// k_glm_image_terms: one thread per image element; grid ceil(16 kp / 256), 256 threads.  covar [q][n], weight [n] or NULL.
__global__ void __launch_bounds__(256) k_glm_image_terms(const double *__restrict__ covar, const double *__restrict__ weight, int n,
	int q, int kp, double *__restrict__ img, double *__restrict__ wt)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)kp * GLM_SLOTS) return;
	const int s = (int)(i >> 4), c = (int)(i & 15);
	double v = 0.0;
	if (s < n) {
		if (c == 0) v = 1.0;
		else if (c >= GLMT_COV0 && c < GLMT_COV0 + q) v = covar[(size_t)(c - GLMT_COV0) * n + s];
	}
	img[i] = v;
	if (c == 0) wt[s] = s < n ? (weight ? weight[s] : 1.0) : 0.0;
}

// k_glm_fit_terms: one workgroup per fit, GLM_WAVES waves.  Lane l of a wave holds slot l & 15 of sample 4 step + (l >> 4).
// The passes are k_glm_fit's: pass 0 from the start value, pass k >= 1 from eta = X beta_k, each also accumulating the tile
// of the next solve with ONE v_mfma_f64_16x16x4_f64 per step (a = W g, b = g, z in slot 15); between passes the waves' tiles
// are added in wave order, and thread 0 tests convergence, factorises (dropping aliased columns) and solves.
//
// Outputs per fit: coef / se [16] by slot (slot 15, unused and dropped slots NaN), deviance, iterations, flags, df_h (the
// terms active in the last solve).
__global__ void __launch_bounds__(GLM_WAVES * 64) k_glm_fit_terms(const double *__restrict__ img, const double *__restrict__ wt,
	const int8_t *__restrict__ y, const int8_t *__restrict__ feat, const GlmTermsFit *__restrict__ fits, int n, int kp, int q,
	int maxit, double epsilon, double *__restrict__ coef, double *__restrict__ se, double *__restrict__ deviance,
	int32_t *__restrict__ iterations, int32_t *__restrict__ flags, int32_t *__restrict__ df_h)
{
	__shared__ double s_tile[GLM_WAVES][256];
	__shared__ double s_A[256];                 // the waves' tiles added: rows / columns = slots
	__shared__ double s_L[GLM_SLOTS * GLM_SLOTS]; // the factor of the last solve, compact (index = position among the active slots)
	__shared__ double s_x[GLM_SLOTS][GLM_SLOTS + 1]; // the columns of L^-1, one row per solving lane
	__shared__ double s_beta[GLM_SLOTS];        // by slot; 0 in unused and dropped slots and in slot 15
	__shared__ double s_u[GLM_SLOTS];
	__shared__ double s_dev[GLM_WAVES];
	__shared__ double s_out[2];                 // [0] devold, [1] the deviance reported
	__shared__ int s_bnd[GLM_WAVES];
	__shared__ int s_act[GLM_SLOTS];            // the active slots in factorisation order
	__shared__ int s_state[5];                  // [0] 0 go on, 1 done; [1] flags of the last pass; [2] iterations; [3] active slots; [4] sticky flags

	const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15;
	const GlmTermsFit *fit = fits + f;
	const double nan = __builtin_nan("");
	if (!fit->fitted) {
		if (tid < GLM_SLOTS) { coef[(size_t)f * GLM_SLOTS + tid] = nan; se[(size_t)f * GLM_SLOTS + tid] = nan; }
		if (tid == 0) { deviance[f] = nan; iterations[f] = 0; flags[f] = fit->flags0; df_h[f] = 0; }
		return;
	}
	if (tid == 0) {
		int p = 0;
		s_act[p++] = 0;
		for (int j = 0; j < q; j++) s_act[p++] = GLMT_COV0 + j;
		for (int j = 0; j < GLMT_TERMS; j++) if (fit->term[j][0] >= 0) s_act[p++] = 1 + j;
		s_state[0] = 0; s_state[1] = 0; s_state[2] = 0; s_state[3] = p; s_state[4] = fit->flags0;
	}
	if (tid < GLM_SLOTS) s_beta[tid] = 0.0;
	__syncthreads();

	// the one or two feature rows behind this lane's slot (slot c is term c - 1)
	const int8_t *fa = nullptr, *fb = nullptr;
	if (c >= 1 && c <= GLMT_TERMS) {
		const int ra = fit->term[c - 1][0], rb = fit->term[c - 1][1];
		if (ra >= 0) fa = feat + (size_t)ra * kp;
		if (ra >= 0 && rb >= 0) fb = feat + (size_t)rb * kp;
	}
	const int n_steps = kp >> 2;

	for (int k = 0;; k++) {
		const bool first = k == 0;
		const double beta_c = s_beta[c];
		glm_d4 acc = {0.0, 0.0, 0.0, 0.0};
		double dev = 0.0;
		bool bnd = false;
		for (int step = wave; step < n_steps; step += GLM_WAVES) {
			const int s = 4 * step + (lane >> 4);
			double g = img[(size_t)step * 64 + lane];
			if (fa) {
				int v = fa[s];
				if (fb) v *= (int)fb[s];
				g = (double)v;
			}
			const double w0 = wt[s];
			const bool is_case = y[s] != 0;
			const double yy = is_case ? 1.0 : 0.0;
			double eta, mu_dev = 0.0;
			if (first) {
				mu_dev = (w0 * yy + 0.5) / (w0 + 1.0);
				eta = log(mu_dev / (1.0 - mu_dev));
			} else {
				eta = glm_row_sum(g * beta_c);
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
			if (c == GLMT_Z) g = z;
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(W * g, g, acc, 0, 0, 0);
		}
		// the wave's deviance part: every lane of a sample holds the same sum; add the four sample groups
		dev += __shfl_xor(dev, 16);
		dev += __shfl_xor(dev, 32);
		const bool any_bnd = __any(bnd);
		if (lane == 0) { s_dev[wave] = dev; s_bnd[wave] = any_bnd; }
		// C/D map of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
		for (int r = 0; r < 4; r++) s_tile[wave][((lane >> 4) + 4 * r) * 16 + c] = acc[r];
		__syncthreads();
		if (tid < 256) {
			double a = s_tile[0][tid];
			for (int w = 1; w < GLM_WAVES; w++) a += s_tile[w][tid];
			s_A[tid] = a;
		}
		__syncthreads();
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
					const double ajj = s_A[sj * GLM_SLOTS + sj];
					double dj = ajj;
					for (int m = 0; m < np; m++) dj -= s_L[j * GLM_SLOTS + m] * s_L[j * GLM_SLOTS + m];
					if (!(dj > 1e-11 * ajj)) {
						if (sj == 0) { ok = false; break; }
						s_state[4] |= GLM_FLAG_ALIASED;     // dropped: the candidates after it never see this column
						continue;
					}
					const double ljj = sqrt(dj);
					if (np != j)
						for (int m = 0; m < np; m++) s_L[np * GLM_SLOTS + m] = s_L[j * GLM_SLOTS + m];
					s_L[np * GLM_SLOTS + np] = ljj;
					for (int i = j + 1; i < p; i++) {
						double v = s_A[s_act[i] * GLM_SLOTS + sj];
						for (int m = 0; m < np; m++) v -= s_L[i * GLM_SLOTS + m] * s_L[np * GLM_SLOTS + m];
						s_L[i * GLM_SLOTS + np] = v / ljj;
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
						double v = s_A[s_act[i] * GLM_SLOTS + GLMT_Z];
						for (int m = 0; m < i; m++) v -= s_L[i * GLM_SLOTS + m] * u[m];
						u[i] = v / s_L[i * GLM_SLOTS + i];
					}
					for (int i = np - 1; i >= 0; i--) {     // L' beta = u
						double v = u[i];
						for (int m = i + 1; m < np; m++) v -= s_L[m * GLM_SLOTS + i] * u[m];
						u[i] = v / s_L[i * GLM_SLOTS + i];
					}
					for (int i = 0; i < GLM_SLOTS; i++) s_beta[i] = 0.0;
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
	if (tid < GLM_SLOTS) {
		double cf = nan, sd = nan;
		int j = -1;
		for (int i = 0; i < p; i++) if (s_act[i] == tid) j = i;
		if (!(fl & GLM_FLAG_RANK) && j >= 0) {
			double ss = 0.0;
			for (int i = j; i < p; i++) {
				double v = i == j ? 1.0 : 0.0;
				for (int m = j; m < i; m++) v -= s_L[i * GLM_SLOTS + m] * s_x[tid][m];
				v /= s_L[i * GLM_SLOTS + i];
				s_x[tid][i] = v;
				ss += v * v;
			}
			cf = s_beta[tid];
			sd = sqrt(ss);
		}
		coef[(size_t)f * GLM_SLOTS + tid] = cf;
		se[(size_t)f * GLM_SLOTS + tid] = sd;
	}
	if (tid == 0) {
		int dfh = 0;
		for (int i = 0; i < p; i++) dfh += s_act[i] >= 1 && s_act[i] <= GLMT_TERMS;
		deviance[f] = (fl & GLM_FLAG_RANK) ? nan : s_out[1];
		iterations[f] = s_state[2];
		flags[f] = fl;
		df_h[f] = (fl & GLM_FLAG_RANK) ? 0 : dfh;
	}
}

#endif
