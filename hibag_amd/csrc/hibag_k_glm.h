// hibag_k_glm.h -- kernels of hlaAssocGlm (R/Association.R:315-436): one logistic regression y ~ h + covariates per test of
// an association handle, R's glm.fit for family = binomial restated.  Host side: hibag_assoc.hip.
//
// All fits of a call share the covariates and differ in the one or two int8 feature rows of their test.  A fit is an
// iteratively reweighted least squares (IRLS) loop; per iteration it needs A = X'WX and b = X'Wz over all samples with
// p <= 15 columns.  With z as a sixteenth column both are ONE 16 x 16 FP64 tile: per four samples a wave issues one
// v_mfma_f64_16x16x4_f64 with a = W g and b = g, g the sample's row (1, h, h2, covariates ..., z).
//
// Slots of a row, fixed: 0 the intercept, 1 h (het for `genotype`), 2 hom (`genotype` only), 3 .. 2 + q the covariates,
// 15 z.  A slot that a fit does not use holds 0 in every row; it stays out of the factorisation (its outputs are NaN).
//
// Operand image (k_glm_image, once per call): float64 [kp][16], 128 bytes per sample, the slots above with 0 in slots 1, 2
// and 15; rows of padding samples (i >= n) are all zero, and their prior weight in wt [kp] is 0, so W = 0 there while every
// other quantity stays finite.
//
// Order of every sum of a fit: a wave walks the steps (four samples each) wave, wave + GLM_WAVES, ...; the waves' tiles and
// deviance parts are added in wave order.  So a fit's numbers depend on n and on GLM_WAVES alone -- not on the other fits
// of the call.  No floating-point atomics.
#ifndef HIBAG_K_GLM_H_
#define HIBAG_K_GLM_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define GLM_WAVES 8                 // waves of a fit's workgroup
#define GLM_SLOTS 16
#define GLM_COV0 3                  // slot of the first covariate
#define GLM_EPS 0x1p-52             // R's .Machine$double.eps

#define GLM_FLAG_MAXIT 1            // not converged within maxit
#define GLM_FLAG_RANK 2             // rank-deficient (or a column that cannot be fitted): the values are NaN
#define GLM_FLAG_BOUNDARY 4         // a fitted probability numerically 0 or 1

typedef double glm_d4 __attribute__((ext_vector_type(4)));

// What a fit reads beside the shared image: the feature rows behind slots 1 and 2 (-1: the slot is unused); row_a == -2
// marks a test that is not fitted at all (flags = GLM_FLAG_RANK, NaN everywhere).
struct GlmFit {
	int row_a, row_b;
};

// k_glm_image: the operand image and the padded prior weights.  covar [q][n] (one row per covariate), weight [n] or NULL
// for 1.  One thread per image element; grid ceil(16 kp / 256), 256 threads.
__global__ void __launch_bounds__(256) k_glm_image(const double *__restrict__ covar, const double *__restrict__ weight, int n, int q,
	int kp, double *__restrict__ img, double *__restrict__ wt)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)kp * GLM_SLOTS) return;
	const int s = (int)(i >> 4), c = (int)(i & 15);
	double v = 0.0;
	if (s < n) {
		if (c == 0) v = 1.0;
		else if (c >= GLM_COV0 && c < GLM_COV0 + q) v = covar[(size_t)(c - GLM_COV0) * n + s];
	}
	img[i] = v;
	if (c == 0) wt[s] = s < n ? (weight ? weight[s] : 1.0) : 0.0;
}

// The sum of v over the 16 lanes of a sample, the same bits in all of them (every step adds the two halves of a butterfly,
// and addition commutes).
__device__ __forceinline__ double glm_row_sum(double v)
{
	v += __shfl_xor(v, 1);
	v += __shfl_xor(v, 2);
	v += __shfl_xor(v, 4);
	v += __shfl_xor(v, 8);
	return v;
}

// k_glm_fit: one workgroup per fit, GLM_WAVES waves.  Lane l of a wave holds slot l & 15 of sample 4 step + (l >> 4).
//
// Pass 0 takes eta from the start value mu = (wt y + 0.5) / (wt + 1) and sums the deviance there (devold); pass k >= 1
// takes eta = X beta_k and sums the deviance of beta_k.  Either pass also accumulates the tile of the NEXT solve from the
// same eta (both use the new beta, so one walk over the image serves both).  Between passes thread 0 tests convergence,
// and if the fit goes on, factorises the tile (Cholesky in column order over the used slots, pivot rule 1e-11 A_jj) and
// solves for the next beta.  The factor of the LAST solve stays in LDS; the standard errors come from it after the loop.
//
// Outputs per fit: coef / se [16] in slot order (slot 15 and unused slots NaN), deviance, iterations, flags.
__global__ void __launch_bounds__(GLM_WAVES * 64) k_glm_fit(const double *__restrict__ img, const double *__restrict__ wt,
	const int8_t *__restrict__ y, const int8_t *__restrict__ feat, const GlmFit *__restrict__ fits, int n, int kp, int q, int maxit,
	double epsilon, double *__restrict__ coef, double *__restrict__ se, double *__restrict__ deviance, int32_t *__restrict__ iterations,
	int32_t *__restrict__ flags)
{
	__shared__ double s_tile[GLM_WAVES][256];
	__shared__ double s_A[256];                 // the waves' tiles added: rows / columns = slots
	__shared__ double s_L[GLM_SLOTS * GLM_SLOTS]; // the factor of the last solve, compact (index = position among the used slots)
	__shared__ double s_beta[GLM_SLOTS];        // by slot; 0 in unused slots and in slot 15
	__shared__ double s_dev[GLM_WAVES];
	__shared__ int s_bnd[GLM_WAVES];
	__shared__ int s_act[GLM_SLOTS];            // the used slots in column order
	__shared__ int s_state[4];                  // [0] 0 go on, 1 done; [1] flags; [2] iterations; [3] used slots
	__shared__ double s_x[GLM_SLOTS][GLM_SLOTS + 1]; // the columns of L^-1, one row per solving lane
	__shared__ double s_u[GLM_SLOTS];
	__shared__ double s_out[2];                 // [0] devold, [1] the deviance reported

	const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15;
	const GlmFit fit = fits[f];
	const double nan = __builtin_nan("");
	if (fit.row_a == -2) {
		if (tid < GLM_SLOTS) { coef[(size_t)f * GLM_SLOTS + tid] = nan; se[(size_t)f * GLM_SLOTS + tid] = nan; }
		if (tid == 0) { deviance[f] = nan; iterations[f] = 0; flags[f] = GLM_FLAG_RANK; }
		return;
	}
	if (tid == 0) {
		int p = 0;
		s_act[p++] = 0;
		if (fit.row_a >= 0) s_act[p++] = 1;
		if (fit.row_b >= 0) s_act[p++] = 2;
		for (int j = 0; j < q; j++) s_act[p++] = GLM_COV0 + j;
		s_state[0] = 0; s_state[1] = 0; s_state[2] = 0; s_state[3] = p;
	}
	if (tid < GLM_SLOTS) s_beta[tid] = 0.0;
	__syncthreads();

	const int8_t *fa = fit.row_a >= 0 ? feat + (size_t)fit.row_a * kp : nullptr;
	const int8_t *fb = fit.row_b >= 0 ? feat + (size_t)fit.row_b * kp : nullptr;
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
			if (c == 1 && fa) g = (double)fa[s];
			if (c == 2 && fb) g = (double)fb[s];
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
			if (c == 15) g = z;
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
				// solve k + 1: L L' = A over the used slots, column by column
				const int p = s_state[3];
				bool ok = true;
				for (int j = 0; j < p && ok; j++) {
					const int sj = s_act[j];
					const double ajj = s_A[sj * 16 + sj];
					double dj = ajj;
					for (int m = 0; m < j; m++) dj -= s_L[j * 16 + m] * s_L[j * 16 + m];
					if (!(dj > 1e-11 * ajj)) { ok = false; break; }
					const double ljj = sqrt(dj);
					s_L[j * 16 + j] = ljj;
					for (int i = j + 1; i < p; i++) {
						double v = s_A[s_act[i] * 16 + sj];
						for (int m = 0; m < j; m++) v -= s_L[i * 16 + m] * s_L[j * 16 + m];
						s_L[i * 16 + j] = v / ljj;
					}
				}
				if (!ok) {
					done = 1;
					s_state[1] = GLM_FLAG_RANK;
					s_state[2] = k + 1;
				} else {
					double *u = s_u;
					for (int i = 0; i < p; i++) {           // L u = b
						double v = s_A[s_act[i] * 16 + 15];
						for (int m = 0; m < i; m++) v -= s_L[i * 16 + m] * u[m];
						u[i] = v / s_L[i * 16 + i];
					}
					for (int i = p - 1; i >= 0; i--) {      // L' beta = u
						double v = u[i];
						for (int m = i + 1; m < p; m++) v -= s_L[m * 16 + i] * u[m];
						u[i] = v / s_L[i * 16 + i];
					}
					for (int i = 0; i < p; i++) s_beta[s_act[i]] = u[i];
				}
			}
			s_state[0] = done;
		}
		__syncthreads();
		if (s_state[0]) break;
	}

	// results: the lane of a used slot solves L x = e_j for its column j; (A^-1)_jj is the squared norm of x
	const int p = s_state[3], fl = s_state[1];
	if (tid < GLM_SLOTS) {
		double cf = nan, sd = nan;
		int j = -1;
		for (int i = 0; i < p; i++) if (s_act[i] == tid) j = i;
		if (!(fl & GLM_FLAG_RANK) && j >= 0) {
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
		coef[(size_t)f * GLM_SLOTS + tid] = cf;
		se[(size_t)f * GLM_SLOTS + tid] = sd;
	}
	if (tid == 0) {
		deviance[f] = (fl & GLM_FLAG_RANK) ? nan : s_out[1];
		iterations[f] = s_state[2];
		flags[f] = fl;
	}
}

#endif
