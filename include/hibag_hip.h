/*
 * hibag_hip.h -- C ABI of libhibag_hip.so, the MI355X (gfx950) implementation
 * of HIBAG's attribute-bagging prediction hot path.
 *
 * Plain C: pointers, sizes, int/double only.  No exception crosses this
 * boundary: every entry returns 0 on success or a negative HIBAG_HIP_E* code,
 * and hibag_hip_last_error() returns the message of the calling thread's last
 * failure (the reference throws ErrHLA and turns it into Rf_error,
 * src/HIBAG.cpp:41-60; a binding re-raises from the code + message).
 *
 * Each entry names the reference interface it replaces.  Paths are relative to
 * the HIBAG source tree (zhengxwen/HIBAG, package 1.47.3, kernel 1.5).
 */
#ifndef HIBAG_HIP_H_
#define HIBAG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIBAG_HIP_ABI_VERSION 7   /* 2: + PLINK BED entries, training driver; 3: + hibag_hip_predict_mapped[_device]; 4: + hibag_hip_model_stored_cells;
                                     5: + hibag_hip_model_status / _clear_status, hibag_hip_predict_multi, hibag_hip_model_replicate, hibag_hip_model_engine;
                                     7: + hibag_hip_predict_snp_major[_device], hibag_hip_trainer_set_shared, hibag_hip_train_set_thread_budget;
                                        later, additive (no bump): + hibag_hip_predict_oob; + the LD entries (hibag_hip_ld_*);
                                        + hibag_hip_model_distance[_ms]; + the merge entries (hibag_hip_merge_*, hibag_hip_predict_merge[_bed]);
                                        + hibag_hip_predict_prefix[_ms];
                                       + the top-k entries (hibag_hip_predict_topk[_device, _mapped, _snp_major, _bed]): added within version 7;
                                       + the resident cohort (hibag_hip_cohort_*, hibag_hip_predict_cohort, hibag_hip_predict_topk_cohort): likewise;
                                       + hibag_hip_predict_masked: likewise;
                                       + the draw entries (hibag_hip_predict_draw[_device, _mapped, _snp_major, _bed, _cohort]): likewise;
                                       + hibag_hip_test_build_eval_batch (a test entry): likewise;
                                       + hibag_hip_test_em_fit, hibag_hip_test_em_layout (test entries), hibag_hip_trainer_em_counts: likewise;
                                       + the association entries (hibag_hip_assoc_*): likewise;
                                       + the out-of-bag knock-out (hibag_hip_oob_knock, hibag_hip_oob_knock_variants): likewise;
                                       + hibag_hip_test_layout_plan, _count, _get, _free (test entries): likewise;
                                       + the regression entries (hibag_hip_assoc_glm, _n_kept, _feature_rows): likewise;
                                       + the quantitative-trait entries (hibag_hip_assoc_quant_*): likewise;
                                       + the set regression (hibag_hip_assoc_glm_sets, hibag_hip_assoc_row_sums): likewise;
                                       + the term regression (hibag_hip_assoc_glm_terms, hibag_hip_assoc_row_gram): likewise;
                                       + the score tests (hibag_hip_assoc_score_*): likewise;
                                       + the Cox regression (hibag_hip_assoc_cox, hibag_hip_assoc_cox_segment): likewise */

/* error codes */
#define HIBAG_HIP_OK          0
#define HIBAG_HIP_EINVAL     (-1)  /* bad argument (message says which)            */
#define HIBAG_HIP_ENODEV     (-2)  /* no usable HIP device / HIP runtime error     */
#define HIBAG_HIP_ENOMEM     (-3)  /* host or device allocation failed             */
#define HIBAG_HIP_ESTATE     (-4)  /* call order violated (e.g. predict before finalize) */
#define HIBAG_HIP_EHANDOVER  (-5)  /* a launch could not vouch for its sums (see "launch status" below); outputs were poisoned */

/* R's NA_integer_: what H1/H2 hold when no allele pair has positive
 * probability (src/LibHLA.cpp:1552), and the usual missing-genotype code. */
#define HIBAG_HIP_NA_INTEGER (-2147483647 - 1)

/* limits fixed by the reference's packed types */
#define HIBAG_HIP_MAX_SNP_IN_CLASSIFIER 128   /* inst/include/LibHLA_ext.h:223 */

typedef struct hibag_hip_model hibag_hip_model;  /* opaque handle */

/* ---- library / device ---------------------------------------------------- */

int hibag_hip_abi_version(void);

/* Message of this thread's most recent failing call ("" if none). */
const char *hibag_hip_last_error(void);

/* Number of HIP devices visible to the process (0 if none / no driver). */
int hibag_hip_device_count(void);

/* Device used by models created afterwards on this thread (default 0). */
int hibag_hip_set_device(int device);
/* The calling thread's selection (what a host passes on to the worker threads it starts: the selection is per thread). */
int hibag_hip_get_device(void);

/* Kernel-target selection -- the extension of hlaSetKernelTarget()
 * (R/HIBAG.R:1668-1674 -> HIBAG_Kernel_SetTarget, src/HIBAG.cpp:1430-1435 ->
 * CAlg_Prediction::Init_Target_IFunc, src/LibHLA.cpp:1266-1475).  The
 * reference accepts CPU names only; this library accepts exactly "hip" and
 * fails (EINVAL) for anything else, and fails (ENODEV) when no gfx950 device is
 * present -- there is no CPU fallback in this library.  On success writes a
 * description such as "HIP, gfx950, AMD Instinct MI355X, 256 CUs" to `info`. */
int hibag_hip_set_kernel_target(const char *target, char *info, size_t info_len);

/* ---- model construction: replaces HIBAG_New + HIBAG_NewClassifierHaplo --- */

/* HIBAG_New(n.samp, n.snp, n.hla) (src/HIBAG.cpp:486-503).  n_samp is only
 * book-keeping in the reference (bootstrap counts) and is not needed here. */
hibag_hip_model *hibag_hip_model_new(int n_hla, int n_snp);

/* HIBAG_NewClassifierHaplo(model, snpidx-1, samp.num, freq, hla-1, haplo, acc)
 * (src/HIBAG.cpp:817-841 -> CAttrBag_Classifier::Assign, src/LibHLA.cpp:2142-2165).
 *   snpidx[n_snp_c]  0-based indices into the model's SNP list
 *   freq[n_haplo], hla[n_haplo] (0-based, ascending -- haplotypes are grouped
 *   by allele, src/HIBAG.cpp:915-924), haplo[n_haplo] strings of '0'/'1' of
 *   length n_snp_c (char s <-> SNP snpidx[s]).
 * Errors like the reference: more than 128 SNPs, characters other than 0/1. */
int hibag_hip_model_add_classifier(hibag_hip_model *m, int n_snp_c,
	const int32_t *snpidx, int n_haplo, const double *freq,
	const int32_t *hla, const char *const *haplo);

/* Same, from packed haplotypes: bits[2*i], bits[2*i+1] are the two 64-bit words
 * of THaplotype::PackedHaplo (inst/include/LibHLA_ext.h:261-299); bits at
 * positions >= n_snp_c are ignored. */
int hibag_hip_model_add_classifier_packed(hibag_hip_model *m, int n_snp_c,
	const int32_t *snpidx, int n_haplo, const double *freq,
	const int32_t *hla, const uint64_t *bits);

/* Build the device tables (haplotype SoA, cell schedule, mutation table) and
 * upload them.  Must be called once after the last add_classifier. */
int hibag_hip_model_finalize(hibag_hip_model *m);

void hibag_hip_model_free(hibag_hip_model *m);

/* queries */
int hibag_hip_model_device(const hibag_hip_model *m);      /* the HIP device the model lives on (-1 for NULL) */
int hibag_hip_model_n_hla(const hibag_hip_model *m);
int hibag_hip_model_n_snp(const hibag_hip_model *m);
int hibag_hip_model_n_classifier(const hibag_hip_model *m);
/* sum over classifiers of H_c(H_c+1)/2: haplotype-pair evaluations per sample */
int64_t hibag_hip_model_pair_evals(const hibag_hip_model *m);
/* How a finalized model runs its second pass: pass 1 stores `stored_cells` cell sums per sample
 * (8 bytes each: a classifier's sum over the haplotype pairs of one allele pair) that pass 2 reads back, and pass 2
 * evaluates `second_pass_pairs` haplotype pairs per sample again.  All cells / no pairs for models with many pairs per
 * cell; otherwise the cells with many pairs are stored and the pairs of the others evaluated. */
int64_t hibag_hip_model_stored_cells(const hibag_hip_model *m);
int64_t hibag_hip_model_second_pass_pairs(const hibag_hip_model *m);
/* the 257-entry mutation/error table the device uses, exp(d*log(1e-5))
 * (src/LibHLA.cpp:166-183); out[257] */
int hibag_hip_model_mutation_table(const hibag_hip_model *m, double *out);

/* ---- prediction: replaces CAttrBag_Model::PredictHLA -------------------- */

/* CAttrBag_Model::PredictHLA (src/LibHLA.cpp:2317-2412) as reached from
 * HIBAG_Predict_Resp / _Dosage / _Resp_Prob (src/HIBAG.cpp:649-803).
 *   geno        int32 [n_samp][n_snp], sample-major (the memory of the R SNP x
 *               sample matrix); values outside 0..2 (incl. NA_integer_) = missing
 *   vote_method 1 = average posteriors, 2 = majority vote; else EINVAL with the
 *               reference's message "Invalid 'vote_method'."
 * Outputs (any may be NULL; H1 and H2 only together):
 *   H1,H2[n_samp]        0-based allele indices or NA_integer_
 *   max_prob[n_samp]     posterior of the called pair (0 if NA)
 *   matching[n_samp]     weighted mean of the pre-normalisation totals
 *   dosage[n_samp][n_hla]
 *   postprob[n_samp][n_hla(n_hla+1)/2]   pair order h1<=h2, h2 fastest
 * Host-pointer form: copies geno to the device, runs, copies results back. */
int hibag_hip_predict(hibag_hip_model *m, const int32_t *geno, int n_samp,
	int vote_method, int32_t *H1, int32_t *H2, double *max_prob,
	double *matching, double *dosage, double *postprob);

/* hlaOutOfBag's per-classifier predictions (R/HIBAG.R:1320-1334): classifier c of the model, taken as a
 * one-classifier model of its own, predicts every sample s with samp_num[c][s] == 0 -- bit-identical to
 * hlaPredict(vote = "prob") of that one-classifier model (src/LibHLA.cpp:2317-2482): SNP weights all 1, the
 * call the first strict maximum of (0 + p * w) * (1 / w) in pair order, that value the probability.
 *   geno      int32 [n_samp][n_snp], the model's training samples in model$sample.id order
 *   samp_num  int32 [n_classifier][n_samp], the bootstrap counts of each classifier
 * Outputs [n_classifier][n_samp]: H1, H2 (0-based, NA_integer_ where not predicted), prob (0 there).
 * All pointers are host memory and required when n_samp > 0; one batched launch sequence, no second pass. */
int hibag_hip_predict_oob(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num,
	int32_t *H1, int32_t *H2, double *prob);

/* A per-sample classifier mask (hlaOutOfBagEnsemble: every training sample typed by the classifiers that did not see it).
 * Sample s gets exactly what hibag_hip_predict returns for it from the model made of the classifiers c with
 * use[c][s] != 0, in model order (hlaSubModelObj-style; the SNP weights are that sub-model's own,
 * src/LibHLA.cpp:2484-2496) -- every output bit-identical, both vote methods.  A sample no classifier is used for gets
 * what a sample with every SNP missing gets: call NA, max_prob 0, matching NaN.
 *   geno      int32 [n_samp][n_snp], sample-major in model order, as for hibag_hip_predict
 *   use       uint8 [n_classifier][n_samp], row = classifier; nonzero = the classifier takes part for the sample
 * Outputs as for hibag_hip_predict (any may be NULL; H1 and H2 only together).  All pointers are host memory; genotypes
 * and mask go up once, the outputs come down once.  The weights are formed per sample on the device; cell sums, totals
 * and both passes are the model's own kernels. */
int hibag_hip_predict_masked(hibag_hip_model *m, const int32_t *geno, int n_samp, const uint8_t *use, int vote_method,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);

/* Out-of-bag SNP knock-out (hlaSNPImportance; additive, no reference counterpart: DESIGN.md section 21).  A VARIANT is a
 * (classifier c, position j of its SNP list) pair, numbered v = snp_off[c] + j in the order the classifiers and their SNPs
 * were added; hibag_hip_oob_knock_variants returns their number.  Variant (c, j) is classifier c, taken as a one-classifier
 * model of its own as in hibag_hip_predict_oob, predicting its out-of-bag samples with SNP snpidx[c][j] set to missing --
 * bit-identical to hlaPredict(vote = "prob") of that model on those genotypes.  Beside the variants stands one BASE row per
 * classifier with nothing knocked out: row c of hibag_hip_predict_oob.
 *   geno, samp_num  as for hibag_hip_predict_oob
 *   truth           int32 [n_samp][2]: the samples' true alleles as 0-based indices of the model's alleles; a sample with an
 *                   NA_integer_ in its pair (unknown, or an allele the model does not have) is not counted
 *   call_threshold  finite: only calls with prob >= call_threshold count as calls; not finite: every call does
 *   tally           int64 [n_variant + n_classifier][5], the variants' rows first, then the base rows; over the samples
 *                   that are out of bag for the row's classifier and have a truth, counted as hlaCompareAllele does
 *                   (R/DataUtilities.R:1376-1420):
 *                     [0] n_ind      those samples
 *                     [1] n_call     ... with a call (not NA) that passes the threshold
 *                     [2] crt_ind    called samples with both alleles right, in either order
 *                     [3] crt_haplo  right alleles of the called samples (0, 1 or 2 each)
 *                     [4] n_changed  of n_ind, the samples whose (H1, H2) differs from the base row's call (0 in base rows)
 *   H1, H2, prob    optional (NULL: not returned; H1 and H2 only together) [n_variant + n_classifier][n_samp], rows as in
 *                   `tally`: the predictions themselves, NA_integer_ / 0 where the sample is in the bag of the classifier
 * All pointers are host memory.  Rejected before any launch: a NULL or unfinalized model, a model without SNP indices,
 * n_samp < 0, a NULL input or tally.  One call: the cohort goes up once, 40 bytes per row come down. */
int hibag_hip_oob_knock_variants(const hibag_hip_model *m, int *n_variant);
int hibag_hip_oob_knock(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *samp_num, const int32_t *truth,
	double call_threshold, int64_t *tally, int32_t *H1, int32_t *H2, double *prob);

/* ---- allele distances: hlaDistance ------------------------------------------
 * hlaDistance(model) (R/HIBAG.R:1545-1570) in one call: for each classifier HIBAG_Distance (src/HIBAG.cpp:1284-1332),
 * m_c[a][b] = m_c[b][a] = the sum over its haplotype pairs i <= j with alleles (a, b) of f * d divided by the sum of f,
 * f = freq[i] * freq[j], d = the number of SNPs where the two differ, both sums taken in the reference's order (NaN where
 * the cell has no pair); then R's fold: out[a][b] = (m_1 + m_2 + ... with NaN read as 0) / (the number of classifiers
 * whose m_c[a][b] is not NaN), NaN where that number is 0.  Bit-identical to the reference (DESIGN.md "hlaDistance").
 *   out       float64 [n_hla][n_hla], host memory
 *   out_each  NULL, or float64 [n_classifier][n_hla][n_hla]: each classifier's m_c, NaN kept (R's `lst` before NaN -> 0)
 * Works on finalized models and on models that were never finalized (the prediction layout is not needed).  Runs on the
 * model's device after any work outstanding on the model and returns when the results are on the host.  EINVAL for a
 * NULL model or one without classifiers; ENOMEM, with the size, when n_hla is too large for the device. */
int hibag_hip_model_distance(hibag_hip_model *m, double *out, double *out_each);
/* Event time in milliseconds of the kernels of the model's last hibag_hip_model_distance call (for measurements). */
int hibag_hip_model_distance_ms(const hibag_hip_model *m, double *ms);

/* ---- every ensemble size at once: hlaPredictCurve ------------------------
 * For every sizes[i]: what hibag_hip_predict(vote_method = 1) returns for the model made of the first sizes[i] classifiers
 * of `m` (hlaSubModelObj, R/HIBAG.R:1121-1129 -- the SNP weights are that sub-model's own, src/LibHLA.cpp:2484-2496) --
 * the best-guess pair, its posterior probability and the matching proportion -- from ONE pack and ONE pass 1 over all
 * classifiers plus a read-back fold per size.  Every output is bit-identical to the sub-model's own prediction, NA calls
 * and NaN included.
 *   geno      int32 [n_samp][n_snp], host memory, the model's SNPs in model order (as hibag_hip_predict)
 *   sizes     int32 [n_sizes], strictly ascending, 1 <= sizes[i] <= n_classifier; EINVAL otherwise
 *   H1, H2    int32 [n_sizes][n_samp], 0-based alleles or NA_integer_
 *   prob, matching   float64 [n_sizes][n_samp]
 * All four outputs are required.  The dosage and the posterior matrix are not produced (they would be n_sizes matrices),
 * and there is no majority-vote variant.  The entry needs every cell sum kept by pass 1: on a model whose own layout keeps
 * fewer it builds, at its first call, a second layout of the same classifiers that does, owned by the handle (device
 * memory: a second copy of the model's tables and a second workspace); the model's other entries never see it.  Samples go
 * in batches of at most hibag_hip_model_batch_limit(), fewer where the sub-models' weights (8 bytes per sample for every
 * classifier of every size) would exceed 8 GB; HIBAG_PREFIX_BATCH (diagnostic) lowers the batch further.  A failed
 * hand-over is repaired by one run without hand-overs; HIBAG_HIP_EHANDOVER if that fails too.  EINVAL for a classifier
 * shard (hibag_hip_model_shard: its SNP weights are another model's). */
int hibag_hip_predict_prefix(hibag_hip_model *m, const int32_t *geno, int n_samp, const int32_t *sizes, int n_sizes,
	int32_t *H1, int32_t *H2, double *prob, double *matching);
/* Event time in milliseconds of k_prefix_accum (all batches) in the model's last hibag_hip_predict_prefix call. */
int hibag_hip_predict_prefix_ms(const hibag_hip_model *m, double *accum_ms);

/* ---- linkage disequilibrium: hlaGenoLD / hlaLDMatrix ----------------------
 * r^2 = num^2 / (dx dy) from exact integer sums over the samples used (n, Sx, Sxx, Sy, Syy, Sxy; num = n Sxy - Sx Sy,
 * dx = n Sxx - Sx^2, dy = n Syy - Sy^2, all int64, then one double rounding per operation); NaN where dx or dy is 0.
 * The sums are int8 Gram matrices on the matrix cores (DESIGN.md "LD"). */
typedef struct hibag_hip_ld_geno hibag_hip_ld_geno;      /* genotypes resident on the calling thread's device */

/* Copies genotypes to the device selected by the calling thread and packs them there.
 *   geno  int32 [n_snp][n_samp] (snp_major != 0) or [n_samp][n_snp] (snp_major == 0); 0/1/2, anything else is missing
 * n_samp is at most 2^24 (EINVAL beyond: the formula above is exact in double up to there).  NULL on failure
 * (hibag_hip_last_error says why).  Replaces the host matrix that R/HIBAG.R:1431-1443 and :1507 hand to cor(). */
hibag_hip_ld_geno *hibag_hip_ld_geno_new(const int32_t *geno, int n_snp, int n_samp, int snp_major);
void hibag_hip_ld_geno_free(hibag_hip_ld_geno *g);

/* Per SNP the number of called genotypes and their sum: hlaLDMatrix's MAF filter (R/HIBAG.R:1468-1472, rowMeans). */
int hibag_hip_ld_snp_counts(hibag_hip_ld_geno *g, int32_t *n_valid, int64_t *sum);

/* hlaLDMatrix's cor(t(genotype), use = "na.or.complete")^2 (R/HIBAG.R:1507) over the SNPs snp_idx[0 .. n_idx):
 * the samples used are those called at every one of them (*n_complete of them).  r2 is float64 [n_idx][n_idx],
 * host memory; its diagonal is 1, and every entry is NaN when fewer than two samples are complete.  The result is
 * made in row panels (HIBAG_LD_PANEL_ROWS rows if that is set, else about 64 MB each) copied through pinned buffers
 * while the next panel is computed, so device memory does not grow with n_idx^2. */
int hibag_hip_ld_matrix(hibag_hip_ld_geno *g, const int32_t *snp_idx, int n_idx, double *r2, int *n_complete);

/* Event time in milliseconds of the Gram kernels of the handle's last hibag_hip_ld_matrix call (for measurements). */
int hibag_hip_ld_gram_ms(hibag_hip_ld_geno *g, double *ms);

/* hlaGenoLD (R/HIBAG.R:1425-1445): for every SNP j, ld[j] = the mean of the non-NaN r^2(j, a) over the alleles, summed in
 * allele order (NaN if there is none), each r^2 over the samples with a genotype at j and both alleles known.
 *   allele1 / allele2  int32 [n_samp]: 0-based indices into the caller's sorted allele list, HIBAG_HIP_NA_INTEGER = NA
 *   r2_or_null         float64 [n_snp][n_allele], the single r^2 values (may be NULL) */
int hibag_hip_ld_hla(hibag_hip_ld_geno *g, const int32_t *allele1, const int32_t *allele2, int n_allele,
	double *ld, double *r2_or_null);

/* ---- association tests: hlaAssocTest with max-T permutation p-values --------
 * Chi-square tests of every allele, and of every level of every partition of the alleles, against a case / control label
 * (R/Association.R:164-260), under the observed labelling and under permutations of it.  Every statistic is a function of
 * the margins and of the number of case carriers, a dot product over samples; all tests under all permutations of a panel
 * are one int8 Gram matrix on the matrix cores with exact int32 sums.  The definitions -- the statistics' operation order,
 * the permutation generator, the counts -- are DESIGN.md section 20; results do not depend on the panel size or on how a
 * run of permutations is split over calls. */
typedef struct hibag_hip_assoc hibag_hip_assoc;          /* the tests of one cohort, resident on the calling thread's device */

#define HIBAG_HIP_ASSOC_DOMINANT  0   /* unit = sample, feature = carries the allele                        */
#define HIBAG_HIP_ASSOC_ADDITIVE  1   /* unit = chromosome (N = 2 n, cases = 2 n_case), feature = dosage    */
#define HIBAG_HIP_ASSOC_RECESSIVE 2   /* unit = sample, feature = homozygous                                */
#define HIBAG_HIP_ASSOC_GENOTYPE  3   /* 3 x 2 table none / het / hom, no continuity correction             */

/* Builds the tests on the device selected by the calling thread and computes the observed statistics.
 *   allele1 / allele2  int32 [n_samp]: 0-based indices into the caller's allele list, HIBAG_HIP_NA_INTEGER = NA; a sample
 *                      with an NA allele is dropped, the others are the KEPT samples, in order
 *   y                  int32 [n_samp]: 0 = control, 1 = case
 *   group_of           int32 [n_part][n_allele]: the group of every allele in every partition, ids from 0; may be NULL
 *                      with n_part = 0
 *   model              HIBAG_HIP_ASSOC_*
 * The tests, in order: one per allele, then for every partition one per level 0 .. the partition's largest id ("an allele
 * of the sample is in the level" in place of "is the allele").  1 <= n_samp <= 2^24, n_allele >= 1, at most 32,767 tests;
 * EINVAL otherwise, and for an allele index outside [0, n_allele), a label other than 0 / 1 and an unknown model.
 * NULL on failure (hibag_hip_last_error says why). */
hibag_hip_assoc *hibag_hip_assoc_new(const int32_t *allele1, const int32_t *allele2, const int32_t *y, int n_samp, int n_allele,
	const int32_t *group_of, int n_part, int model);
void hibag_hip_assoc_free(hibag_hip_assoc *h);
int hibag_hip_assoc_n_tests(const hibag_hip_assoc *h);

/* The observed labelling: stat float64 [n_tests] (NaN with an empty margin) and table int64 [n_tests][6], the cell counts
 * in units, row-major rows x (control, case): rows (without, with) for the 2 x 2 models -- cells 4 and 5 are 0 --, rows
 * (none, het, hom) for HIBAG_HIP_ASSOC_GENOTYPE. */
int hibag_hip_assoc_observed(hibag_hip_assoc *h, double *stat, int64_t *table);

/* Permutations perm0 .. perm0 + n_perm - 1 of the labels over the kept samples (perm0 >= 1: permutation 0 is the observed
 * labelling; permutation p depends on (seed, p) and the kept samples' number and case count alone):
 *   max_stat     float64 [n_perm]: the largest non-NaN statistic over the tests under each permutation, NaN if none
 *   count_point  int64 [n_tests]: the permutations of THIS call with stat[t] >= the observed stat[t] (0 where that is NaN)
 * A run may be split over calls, handles and devices: max_stat concatenates and the counts add.  The work goes in panels
 * of permutations (HIBAG_ASSOC_PANEL_PERMS per panel if that is set, read per call; else about 64 MB per buffer), so
 * device memory does not grow with n_perm beyond 8 bytes each. */
int hibag_hip_assoc_permute(hibag_hip_assoc *h, uint64_t seed, uint64_t perm0, int64_t n_perm, double *max_stat,
	int64_t *count_point);

/* The label rows of permutations perm0 .. perm0 + n - 1 themselves: out int8 [n][kept samples], 0 / 1 (for tests of the
 * generator). */
int hibag_hip_assoc_labels(hibag_hip_assoc *h, uint64_t seed, uint64_t perm0, int n, int8_t *out);

/* The samples the handle kept (two known alleles), and its feature rows themselves: out int8 [n_rows][n_kept], rows
 * row0 .. row0 + n_rows - 1 without their padding.  Row t is test t's 0 / 1 / 2 column; HIBAG_HIP_ASSOC_GENOTYPE has the rows
 * 2 t (het) and 2 t + 1 (hom).  EINVAL for rows outside the handle's. */
int hibag_hip_assoc_n_kept(const hibag_hip_assoc *h);
int hibag_hip_assoc_feature_rows(hibag_hip_assoc *h, int row0, int n_rows, int8_t *out);

/* ---- covariate-adjusted logistic regression per test: hlaAssocGlm ------------
 * glm(y ~ h + covariates, family = binomial) for every test of the handle (R/Association.R:315-436) and for the base model
 * y ~ covariates: R's glm.fit restated -- iteratively reweighted least squares from R's start value, convergence on the
 * relative change of the deviance, no step halving -- with the standard errors of summary.glm (dispersion 1).  The unit is
 * a sample for every model; `additive` regresses on the dosage 0 / 1 / 2.  The definitions are DESIGN.md section 23.  A
 * fit's numbers depend on the kept samples, its own columns and the arguments below, not on the other tests of the handle.
 *   covar       float64 [n_covar][n_kept], one row per covariate (NULL with n_covar = 0); 0 <= n_covar <= HIBAG_HIP_GLM_MAX_COVAR
 *   weight      float64 [n_kept] prior weights, finite and >= 0, or NULL for 1
 *   maxit       >= 1 iterations at most (R: 25); epsilon > 0 (R: 1e-8)
 * Outputs for n_tests + 1 fits, fit n_tests the base model:
 *   coef, se    float64 [n_tests + 1][16] by slot: 0 the intercept, 1 h (het for GENOTYPE), 2 hom (GENOTYPE only),
 *               3 .. 2 + n_covar the covariates; every other slot NaN
 *   deviance    float64, iterations int32, flags int32 (HIBAG_HIP_GLM_*) [n_tests + 1]
 * A test whose column is constant over the kept samples is not fitted (RANK, NaN).  GENOTYPE: a dummy that nobody carries
 * is left out of its fit (its slot NaN); both empty, or nobody without the allele: RANK.
 * EINVAL for a null handle or output, n_covar outside its range, maxit < 1, epsilon not > 0, a non-finite covariate, a
 * non-finite or negative weight. */
#define HIBAG_HIP_GLM_MAX_COVAR 12
#define HIBAG_HIP_GLM_MAXIT     1   /* not converged within maxit: the last iteration's values are reported */
#define HIBAG_HIP_GLM_RANK      2   /* rank-deficient (a pivot <= 1e-11 A_jj) or not fitted: the values are NaN */
#define HIBAG_HIP_GLM_BOUNDARY  4   /* a fitted probability below 10 eps or above 1 - 10 eps (R's warning)  */
int hibag_hip_assoc_glm(hibag_hip_assoc *h, const double *covar, int n_covar, const double *weight, int maxit, double epsilon,
	double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags);

/* ---- multi-column logistic regression per set of feature rows: hlaAssocOmnibus ------------
 * glm(y ~ r_1 + ... + r_d + covariates, family = binomial) for every SET of feature rows of the handle -- the residues of an
 * amino-acid position, the two-digit types, any partition's levels -- and for the base model y ~ covariates: the fit of
 * hibag_hip_assoc_glm over a design of 32 slots, with R's treatment of aliased columns:
 * a column whose pivot is <= 1e-11 A_jj is dropped (coefficient and standard error NaN, HIBAG_HIP_GLM_ALIASED) and the fit
 * goes on without it.  The factorisation takes the columns in the order intercept, covariates, set rows, so that of two
 * aliased columns the set's is the one dropped.  The definitions are DESIGN.md section 26.
 *   set_start   int32 [n_sets + 1], set_start[0] = 0, not decreasing; set t is set_rows[set_start[t] .. set_start[t + 1])
 *   set_rows    int32 row indices of the handle, as hibag_hip_assoc_feature_rows numbers them; no row twice in a set
 *   covar       float64 [n_covar][n_kept] (NULL with n_covar = 0); 0 <= n_covar <= 29
 *   weight, maxit, epsilon: as hibag_hip_assoc_glm
 * Outputs for n_sets + 1 fits, fit n_sets the base model.  With H the largest size among the sets that are fitted:
 *   coef, se    float64 [n_sets + 1][32] by slot: 0 the intercept, 1 + j row j of the set, 1 + H .. H + n_covar the
 *               covariates; every other slot, and every dropped column, NaN
 *   deviance    float64, iterations int32, flags int32 (HIBAG_HIP_GLM_*) [n_sets + 1]
 *   df_h        int32 [n_sets + 1]: the set's columns still in the fit at its last solve (0 where not fitted)
 * An empty set and a set whose rows all have row sum 0 are not fitted (RANK, NaN); a row with row sum 0 beside others is
 * left out before the fit and counts as ALIASED; a set of more than 30 - n_covar rows is not fitted (TOO_WIDE | RANK).
 * A set's numbers depend on the kept samples, its own rows, the arguments and H -- not on the other sets otherwise.
 * EINVAL as hibag_hip_assoc_glm, and for n_sets < 0, a null set_start or one that does not start at 0 or decreases, a null
 * set_rows with rows to read, a row index outside the handle's rows, the same row twice in a set. */
#define HIBAG_HIP_GLM_WIDE_SLOTS 32
#define HIBAG_HIP_GLM_ALIASED    8   /* a column was dropped as aliased (or left out with row sum 0): its values are NaN */
#define HIBAG_HIP_GLM_TOO_WIDE   16  /* the set has more than 30 - n_covar rows: not fitted (with RANK)                */
int hibag_hip_assoc_glm_sets(hibag_hip_assoc *h, const int32_t *set_start, const int32_t *set_rows, int n_sets, const double *covar,
	int n_covar, const double *weight, int maxit, double epsilon, double *coef, double *se, double *deviance, int32_t *iterations,
	int32_t *flags, int32_t *df_h);

/* The sums of the handle's feature rows over the kept samples: out int32 [rows], rows as hibag_hip_assoc_feature_rows. */
int hibag_hip_assoc_row_sums(hibag_hip_assoc *h, int32_t *out);

/* ---- Cox regression per test for time-to-event traits: hlaAssocSurv ------------
 * coxph(Surv(time, event) ~ h + covariates) for every test of the handle and for the base model Surv ~ covariates: Newton's
 * method on the Efron or Breslow partial likelihood, no step halving.  The handle's kept samples must come in time order,
 * LATEST FIRST, and its y is the event indicator.  The definitions are DESIGN.md section 31.  A fit's numbers depend on the
 * kept samples, its own columns and the arguments below, not on the other tests of the handle.
 *   time        float64 [n_kept], finite, >= 0, not increasing
 *   covar       float64 [n_covar][n_kept], one row per covariate, centred by the caller (NULL with n_covar = 0);
 *               0 <= n_covar <= HIBAG_HIP_COX_MAX_COVAR
 *   ties        HIBAG_HIP_COX_EFRON or HIBAG_HIP_COX_BRESLOW
 *   maxit       >= 1 iterations at most; epsilon > 0: converged when |1 - loglik_old / loglik_new| <= epsilon
 *   start       float64 [n_covar] where the base model's coefficients start, or NULL for 0
 * Outputs for 1 + n_tests fits, fit 0 the base model, fit 1 + t test t; a test starts from 0 for h and the base model's
 * coefficients:
 *   coef, se    float64 [1 + n_tests][16] by slot: 0 h (het for GENOTYPE), 1 hom (GENOTYPE only), 2 .. 1 + n_covar the
 *               covariates; every other slot NaN
 *   loglik      float64: the partial log-likelihood of the reported coefficients
 *   score       float64: the score statistic of the h slots at the start (NaN for the base model)
 *   iterations int32, flags int32 (HIBAG_HIP_COX_*)
 * A test whose column is constant over the kept samples is not fitted (RANK, NaN), GENOTYPE as hibag_hip_assoc_glm; with
 * no event among the kept samples, or a base model with RANK, no fit is.
 * EINVAL for a null handle, time or output, n_covar outside its range, bad ties, maxit < 1, epsilon not > 0, a non-finite
 * covariate or start value, a time that is not finite, negative or larger than its predecessor. */
#define HIBAG_HIP_COX_MAX_COVAR 12
#define HIBAG_HIP_COX_EFRON     0
#define HIBAG_HIP_COX_BRESLOW   1
#define HIBAG_HIP_COX_MAXIT     1   /* not converged within maxit: the last values are reported */
#define HIBAG_HIP_COX_RANK      2   /* a pivot of I = G - V <= 1e-11 G_jj, a column that cannot be fitted, no event: the values are NaN */
#define HIBAG_HIP_COX_CLAMP     4   /* a linear predictor outside [-200, 200] was clamped in some evaluation */
#define HIBAG_HIP_COX_DECREASE  8   /* the log-likelihood decreased in an iteration that did not converge (no step halving) */
int hibag_hip_assoc_cox(hibag_hip_assoc *h, const double *time, const double *covar, int n_covar, int ties, int maxit, double epsilon,
	const double *start, double *coef, double *se, double *loglik, double *score, int32_t *iterations, int32_t *flags);

/* The constants of the fit kernel's walk at n_kept samples: *step the samples of one matrix-core step, *segment the
 * contiguous samples one wave owns (the tests place ties across the seams with them). */
int hibag_hip_assoc_cox_segment(int n_kept, int *step, int *segment);

/* ---- pairwise interaction fits: hlaAssocInteract ------------
 * The co-carriage sums of feature rows: out int32 [n_rows][n_rows], out[i][j] = the sum over the kept samples of
 * feat[row0 + i][s] * feat[row0 + j][s], rows as hibag_hip_assoc_feature_rows numbers them.  Integer sums on the int8 Gram
 * kernel, exact; the diagonal of a 0 / 1 row is its row sum.  EINVAL for a null pointer, rows outside the handle's, or
 * n_rows > 8192. */
int hibag_hip_assoc_row_gram(hibag_hip_assoc *h, int row0, int n_rows, int32_t *out);

/* glm(y ~ t_1 + t_2 + t_3 + covariates, family = binomial) for every fit RECORD of up to three terms, and for the base model
 * y ~ covariates: the fit of hibag_hip_assoc_glm with the aliased-column rule of
 * hibag_hip_assoc_glm_sets, where a term is a feature row of the handle or the PRODUCT of two rows -- for two alleles of one
 * locus the heterozygote a/b.  The product is formed per sample as an integer while the fit walks the samples; no product row
 * exists in memory.  The definitions are DESIGN.md section 27.
 *   terms       int32 [n_fits][3][2]: term j of a fit is (row_a, row_b): (-1, -1) unused, (a, -1) row a, (a, b) the product
 *               of rows a and b; 0 <= n_fits <= 2^20
 *   covar       float64 [n_covar][n_kept] (NULL with n_covar = 0); 0 <= n_covar <= HIBAG_HIP_GLM_TERMS_MAX_COVAR
 *   weight, maxit, epsilon: as hibag_hip_assoc_glm
 * Outputs for n_fits + 1 fits, fit n_fits the base model:
 *   coef, se    float64 [n_fits + 1][16] by slot: 0 the intercept, 1 + j term j, 4 .. 3 + n_covar the covariates; every other
 *               slot, every term left out and every dropped column NaN
 *   deviance    float64, iterations int32, flags int32 (HIBAG_HIP_GLM_*) [n_fits + 1]
 *   df_h        int32 [n_fits + 1]: the terms still in the fit at its last solve (0 where not fitted)
 * The factorisation takes the columns in the order intercept, covariates, terms in slot order; a column whose pivot is
 * <= 1e-11 A_jj is dropped (NaN, ALIASED).  Decided from integer sums before any fit: a term whose column sum is 0 is left out
 * (its slot NaN, ALIASED); a fit with no term left, or with three unused terms, is not fitted (RANK, NaN, df_h 0).  The slot
 * layout is fixed, so a fit's numbers depend on the kept samples, its own terms and the arguments -- not on the other fits.
 * EINVAL as hibag_hip_assoc_glm, and for n_covar > 11, n_fits outside its range, null terms with fits to read, a row index
 * outside the handle's rows, row_a = -1 with row_b >= 0, the same term twice in a fit (a product taken unordered). */
#define HIBAG_HIP_GLM_TERMS_MAX_COVAR 11
int hibag_hip_assoc_glm_terms(hibag_hip_assoc *h, const int32_t *terms, int n_fits, const double *covar, int n_covar,
	const double *weight, int maxit, double epsilon, double *coef, double *se, double *deviance, int32_t *iterations,
	int32_t *flags, int32_t *df_h);

/* ---- a quantitative trait on the tests of a handle: hlaAssocQuant ------------
 * lm(y ~ h + covariates) for every test of the handle (R/Association.R:262-313, 368-376 with a continuous y), with max-T
 * permutation p-values by Freedman-Lane permutations of the residual trait, and the class sums behind the t-test and ANOVA
 * columns.  The unit is a sample for every model.  With the constant and the covariates orthonormalised (q_0 .. q_q), a
 * permuted statistic is a function of g = F r, a real-valued Gram matrix int8 feature rows x FP64 residual rows on the FP64
 * matrix cores, and of rr = sum r^2.  The definitions -- basis, permutation generator, orders of the sums, statistic -- are
 * DESIGN.md section 25; results do not depend on the panel size, on the other tests of the handle or on how a run of
 * permutations is split over calls.  The labels the association handle was built with play no part. */
typedef struct hibag_hip_quant hibag_hip_quant;          /* a trait and its basis on a hibag_hip_assoc, which it borrows */

#define HIBAG_HIP_QUANT_RANK 2   /* the test is not fitted (a constant column, sxx <= 1e-11 xx, det <= 1e-11 a11 a22): NaN */

/* Orthonormalises (1, covariates) on the host by modified Gram-Schmidt applied twice, takes the residual trait, and runs the
 * class sums, the projections of the feature rows and the observed trait (permutation 0) on the device of `h`.
 *   y       float64 [n_kept], finite
 *   covar   float64 [n_covar][n_kept], one row per covariate (NULL with n_covar = 0), finite; 0 <= n_covar <= HIBAG_HIP_GLM_MAX_COVAR
 * The handle is owned separately (hibag_hip_assoc_quant_free) and must be freed before `h`; it uses the stream of `h`, so
 * the two are used by one host thread at a time.  NULL on failure: EINVAL for a null pointer, n_covar outside its range, a
 * non-finite value, fewer than 1 residual degree of freedom (n_kept - 1 - n_covar - d, d = 2 for HIBAG_HIP_ASSOC_GENOTYPE,
 * else 1), and for a covariate in the span of the constant and the earlier ones (the message says "collinear"). */
hibag_hip_quant *hibag_hip_assoc_quant_new(hibag_hip_assoc *h, const double *y, const double *covar, int n_covar);
void hibag_hip_assoc_quant_free(hibag_hip_quant *q);

/* Per test and class d = 0, 1, 2 of its samples (the row value; het = 1, hom = 2 for GENOTYPE): cnt int64, S1 = sum y_c and
 * S2 = sum y_c^2 float64, each [n_tests][3], with y_c = y - *ybar. */
int hibag_hip_assoc_quant_classes(hibag_hip_quant *q, int64_t *cnt, double *S1, double *S2, double *ybar);

/* The observed trait: proj float64 [rows][1 + n_covar] (feature row x basis column; rows = n_tests, 2 n_tests for GENOTYPE),
 * g float64 [rows], *rr, stat float64 [n_tests] (NaN where not fitted or rr - m <= 0), flags int32 [n_tests]
 * (HIBAG_HIP_QUANT_RANK). */
int hibag_hip_assoc_quant_observed(hibag_hip_quant *q, double *proj, double *g, double *rr, double *stat, int32_t *flags);

/* Permutations perm0 .. perm0 + n_perm - 1 of the residual trait (perm0 >= 1: permutation 0 is the identity; permutation p
 * depends on (seed, p) and the number of kept samples alone); max_stat [n_perm] and count_point [n_tests] as
 * hibag_hip_assoc_permute's.  The work goes in panels of permutations, in whole tiles of 16 (HIBAG_QUANT_PANEL_PERMS per panel
 * if that is set, read per call; else about 256 MB of residuals). */
int hibag_hip_assoc_quant_permute(hibag_hip_quant *q, uint64_t seed, uint64_t perm0, int64_t n_perm, double *max_stat,
	int64_t *count_point);

/* The permutations themselves: out int32 [n][n_kept], row j = permutation perm0 + j (for tests of the generator). */
int hibag_hip_assoc_quant_perm_rows(hibag_hip_quant *q, uint64_t seed, uint64_t perm0, int n, int32_t *out);

/* Event time of the Gram kernels of the last hibag_hip_assoc_quant_permute call, in ms (for measurements). */
int hibag_hip_assoc_quant_gram_ms(const hibag_hip_quant *q, double *ms);

/* ---- covariate-adjusted score tests with multiplier resampling: hlaAssocScore ------------
 * Under the base model glm(y ~ covariates, family = binomial), fitted once, the score test of a SET of feature rows of the
 * handle -- a single test's row, the two dummies of GENOTYPE, the residues of a position -- is T = U' V^-1 U with
 * U = X~'(y - mu), X~ the rows projected off the covariates under the model's weights, chi-square with one degree of freedom
 * per kept row.  Lin's multiplier resampling (Bioinformatics 21:781, 2005) replaces every sample's residual e_i by e_i s_i with
 * independent signs; replicate 0 has all signs +1 and is the observed run.  All rows under all replicates of a panel are one
 * real-valued Gram matrix, int8 feature rows x FP64 resampled residuals, on the FP64 matrix cores; no fit is repeated.  The
 * definitions -- base fit, weighted basis, sign generator, orders of the sums, statistic -- are DESIGN.md section 28; results
 * do not depend on the panel size, on the other sets or on how a run of replicates is split over calls. */
typedef struct hibag_hip_score hibag_hip_score;          /* a base model and its sets on a hibag_hip_assoc, which it borrows */

#define HIBAG_HIP_SCORE_MAX_ROWS 30   /* feature rows of a set */

/* Fits the base model (the fit of hibag_hip_assoc_glm without an h column; covar, weight, maxit, epsilon as there), takes
 * mu, the weights w = weight mu (1 - mu) and the residuals e = weight (y - mu) on the host, orthonormalises (1, covariates)
 * under sum_i w_i a_i b_i by modified Gram-Schmidt applied twice, and projects every feature row of `h` on that basis on the
 * device of `h`.  A base fit that did not converge (HIBAG_HIP_GLM_MAXIT in hibag_hip_assoc_score_base's flags) leaves a
 * handle whose sets all carry that flag and NaN.  The handle is owned separately (hibag_hip_assoc_score_free) and must be
 * freed before `h`; it uses the stream of `h`, so the two are used by one host thread at a time.  NULL on failure: EINVAL as
 * hibag_hip_assoc_glm, and for a rank-deficient base fit or a column in the weighted span of the earlier ones (the message
 * says "collinear"). */
hibag_hip_score *hibag_hip_assoc_score_new(hibag_hip_assoc *h, const double *covar, int n_covar, const double *weight, int maxit,
	double epsilon);
void hibag_hip_assoc_score_free(hibag_hip_score *s);

/* The base model's fit as hibag_hip_assoc_glm reports fit n_tests: coef, se float64 [16] by slot (0 the intercept,
 * 3 .. 2 + n_covar the covariates, NaN elsewhere), *deviance, *iterations, *flags. */
int hibag_hip_assoc_score_base(hibag_hip_score *s, double *coef, double *se, double *deviance, int32_t *iterations, int32_t *flags);

/* Installs the sets (set_start, set_rows as hibag_hip_assoc_glm_sets takes them; a set has at most HIBAG_HIP_SCORE_MAX_ROWS
 * rows) and runs the observed residuals through them.  Per set the device sums S[a][b] = sum_i w_i F[a][i] F[b][i]; the host
 * forms V = S - P P' (P the set's rows of proj) and factorises it in column order.  A row with row sum 0, and a column whose
 * pivot is <= 1e-11 S_jj, is dropped: its bit in `kept` is clear, the set has HIBAG_HIP_GLM_ALIASED and one degree of freedom
 * less; a set left without columns (an empty one included) has HIBAG_HIP_GLM_RANK alone and NaN.
 *   proj   float64 [rows][1 + n_covar]: feature row x basis column, every row of the handle
 *   S      float64, set t's [m][m] (m its rows, symmetric) at the sum of the earlier sets' m^2
 *   kept   int32 [n_sets]: bit j set = row j of the set is in its factor
 * Installing sets again replaces the earlier ones.  EINVAL as hibag_hip_assoc_glm_sets, and for a set of more than 30 rows. */
int hibag_hip_assoc_score_sets(hibag_hip_score *s, const int32_t *set_start, const int32_t *set_rows, int n_sets, double *proj, double *S,
	int32_t *kept);

/* The same on REAL-VALUED feature rows (hlaAssocHaplo: expected haplotype dosages): `rows` is host
 * float64 [m][n_kept] in the handle's kept-sample order, and set_rows names rows 0 .. m - 1 of it.  proj[row][k] =
 * sum_i X[row][i] (w_i q_k[i]), S[a][b] = sum_i (w_i X[a][i]) X[b][i], g[row][p] = sum_i X[row][i] r_i: the definitions above
 * with X in place of the int8 rows, every sum in the int8 kernels' order.  A row with S_jj == 0 is dropped (in place of
 * "row sum 0"); the pivot rule, flags, df and kept masks are unchanged.  proj is float64 [m][1 + n_covar]; S and kept as
 * above.  After this call hibag_hip_assoc_score_observed (g float64 [m]) and _resample run over these rows; after a later
 * hibag_hip_assoc_score_sets call they run over the handle's int8 rows again.  EINVAL as hibag_hip_assoc_score_sets, and
 * for m < 1, a null `rows`, a value that is NaN or infinite. */
int hibag_hip_assoc_rscore_sets(hibag_hip_score *s, const double *rows, int m, const int32_t *set_start, const int32_t *set_rows,
	int n_sets, double *proj, double *S, int32_t *kept);

/* The observed run: g float64 [rows] (every feature row's score), stat float64 [n_sets] (NaN where not fitted), df int32
 * [n_sets] (the kept rows; 0 where not fitted), flags int32 [n_sets] (HIBAG_HIP_GLM_MAXIT: the base fit did not converge;
 * _RANK; _ALIASED).  hibag_hip_assoc_score_n_df: the number of distinct values > 0 in df. */
int hibag_hip_assoc_score_observed(hibag_hip_score *s, double *g, double *stat, int32_t *df, int32_t *flags);
int hibag_hip_assoc_score_n_df(const hibag_hip_score *s);

/* Replicates p0 .. p0 + n_perm - 1 (p0 >= 1; replicate p's signs depend on (seed, p) and the sample's index alone):
 *   max_stat     float64 [n_perm][n_df]: per replicate and distinct df value (ascending) the largest non-NaN statistic over
 *                the sets with that df, NaN if none
 *   count_point  int64 [n_sets]: the replicates of THIS call with T >= the observed T (0 where that is NaN)
 * A run may be split over calls: max_stat concatenates and the counts add.  The work goes in panels of replicates, in whole
 * tiles of 16 (HIBAG_SCORE_PANEL_PERMS per panel if that is set, read per call; else about 256 MB of residuals). */
int hibag_hip_assoc_score_resample(hibag_hip_score *s, uint64_t seed, uint64_t p0, int64_t n_perm, double *max_stat, int64_t *count_point);

/* The signs themselves: out int8 [n][n_kept], row j = replicate p0 + j, +1 or -1 (for tests of the generator). */
int hibag_hip_assoc_score_signs(hibag_hip_score *s, uint64_t seed, uint64_t p0, int n, int8_t *out);

/* Event times of the last hibag_hip_assoc_score_resample call, in ms: ms[0] the residual panels (signs, projection, panel
 * write), ms[1] the Gram, ms[2] the statistics (for measurements). */
int hibag_hip_assoc_score_ms(const hibag_hip_score *s, double *ms);

/* ---- multi-locus haplotypes: hlaHaplotypes, an EM over imputed calls ---------
 * Which alleles of 2 .. 6 loci sit together on a chromosome, and how often: an EM over the haplotype pairs that each
 * sample's candidate allele pairs (hibag_hip_predict_topk's lists, or certain typing) allow.  The definitions -- candidate
 * and state order, the haplotype key, the one summation rule, the iteration -- are DESIGN.md section 29; every number is
 * made of IEEE FP64 adds, multiplies and divides in a fixed order and does not depend on launch shapes. */
typedef struct hibag_hip_haplo hibag_hip_haplo;          /* the states and the dictionary of one cohort, resident on a device */

#define HIBAG_HIP_HAPLO_MAX_LOCI   6
#define HIBAG_HIP_HAPLO_MAX_ALLELE 1024   /* alleles of a locus: 10 bits of the key each */
#define HIBAG_HIP_HAPLO_MAX_K      64     /* candidates per sample and locus */

/* Builds the states, the haplotype dictionary and every haplotype's list on `device` (-1: the calling thread's).
 *   h1 / h2 / prob  int32, int32, float64 [n_loci][n_samp][k]: per locus and sample the candidate pairs in rank order
 *                   (0-based allele indices, the smaller first when stored) with their weights.  A rank with
 *                   HIBAG_HIP_NA_INTEGER or weight 0 is no candidate; a sample without a candidate at some locus is left out.
 *   max_states      the most states one sample may have (the caller trims its candidates beforehand)
 * EINVAL: n_loci outside 2 .. 6, k outside 1 .. HIBAG_HIP_HAPLO_MAX_K, an allele index outside [0, 1024) and not NA, a
 * weight that is negative or not finite, a sample with more than max_states states, more than 2^31 - 1 entries (two per
 * state) in total, no sample used.  NULL on failure (hibag_hip_last_error says why). */
hibag_hip_haplo *hibag_hip_haplo_new(int n_samp, int n_loci, int k, const int32_t *h1, const int32_t *h2, const double *prob,
	int max_states, int device);
void hibag_hip_haplo_free(hibag_hip_haplo *h);

/* *n_hap: distinct haplotypes H; *n_states: states of all used samples; *n_used; used int32 [n_samp]: 1 = used; states
 * int64 [n_samp]: states per sample (0 for one left out).  Every output may be NULL. */
int hibag_hip_haplo_dims(const hibag_hip_haplo *h, int32_t *n_hap, int64_t *n_states, int32_t *n_used, int32_t *used, int64_t *states);

/* The EM from f = 1 / H: at most maxit >= 1 iterations, stopping after the first with delta = max |f' - f| <= tol (tol >= 0).
 *   freq float64 [H], keys uint64 [H]: the frequencies after the last iteration made and the haplotypes' keys (allele index
 *   of locus l in bits 10 l .. 10 l + 9), ascending; *n_iter, *delta: iterations made and the last one's delta;
 *   *n_zero: used samples whose states all have weight 0 under freq (their total is 0, their posteriors are 0, not NaN).
 * A fit starts afresh: two fits on one handle give the same arrays. */
int hibag_hip_haplo_fit(hibag_hip_haplo *h, int maxit, double tol, double *freq, uint64_t *keys, int32_t *n_iter, double *delta,
	int32_t *n_zero);

/* After a fit, under its frequencies: per sample the state with the largest posterior, the first of equals in state order:
 * hapA / hapB int32 [n_samp][n_loci] (allele indices), prob float64 [n_samp] (that posterior), total float64 [n_samp] (the
 * sample's likelihood, the sum of its states' weights).  A sample left out has HIBAG_HIP_NA_INTEGER and NaN.  ESTATE before
 * a fit. */
int hibag_hip_haplo_calls(hibag_hip_haplo *h, int32_t *hapA, int32_t *hapB, double *prob, double *total);

/* After a fit, under its frequencies and the posteriors q of the same last E step as hibag_hip_haplo_calls: the expected
 * number of copies of haplotype hap[j] (an index into the fit's ascending-key order, 0 .. H - 1) that sample i carries,
 *   out  float64 [m][n_samp]: the sum of q over those entries of the haplotype's list that belong to sample i, from 0.0 in
 *        ascending entry number with one rounding per addition (an all-homozygous state lists its haplotype twice and adds
 *        its q twice); 0.0 where the list has no entry of the sample; NaN for a sample left out.
 * EINVAL before a fit, for m < 1, an index outside 0 .. H - 1, a null pointer. */
int hibag_hip_haplo_dosage(hibag_hip_haplo *h, const int32_t *hap, int m, double *out);

/* ---- several models of one locus, merged: hlaPredMerge on the device ----------
 * hlaPredMerge(hlaPredict(m1, type = "response+prob"), hlaPredict(m2, ...), ...) (R/HIBAG.R:825-1023 around HIBAG_SumList,
 * HIBAG_UpdateAddProbW, HIBAG_NormalizeProb, src/HIBAG.cpp:1455-1547) without the k posterior matrices leaving the device,
 * bit-identical to the merge of the k host results.  The NAMES (allele replacement, the merged allele list, which merged
 * pair a model's pair becomes) are the host's business; the plan takes their outcome:
 *   n_src_cell[i]      allele pairs of model i, n_hla_i (n_hla_i + 1) / 2, in hibag_hip_predict's postprob order
 *   row_of_cell[i][j]  merged row of model i's pair j; merged rows are the pairs of the n_merged_hla merged alleles in the
 *                      same order (row (a, b), a <= b, at b + a (2 n - a - 1) / 2 is named allele[b] "/" allele[a]); a map
 *                      may send several pairs to one row, and a row may have none
 * With weights w (given normalised, sum 1) and per sample s:
 *   matching[s] = 0 + w[0] matching_0[s] + w[1] matching_1[s] + ...          (in model order)
 *   acc[r][s]   = 0 + the terms p_i[j][s] * w2_i[s] of row r, in model order, then ascending j;
 *                 w2_i[s] = w[i] * matching_i[s] if use_matching, else w[i]; product rounded, then the sum
 *   postprob[r][s] = acc[r][s] / (0 + acc[0][s] + acc[1][s] + ...)           (rows ascending; an IEEE division)
 *   the call    = the first maximum of postprob[.][s] in row order, NaN read as -infinity: H2 = b (the row's first name),
 *                 H1 = a, max_prob = that row's value (NaN where the whole column is)
 *   dosage[a][s] = (the sum of postprob over the rows whose first name is a, ascending) + (the same for the second name)
 * Output MATRICES are row-major with the sample fastest -- dosage [n_merged_hla][ld], postprob [rows][ld] -- the memory of
 * hlaPredMerge's own matrices, not the sample-major form of hibag_hip_predict.  At most 16 models.
 * Device memory: the merged matrix is made for one chunk of samples at a time, chunks sized so that it stays within
 * HIBAG_HIP_MERGE_BUDGET_BYTES (and a chunk is one batch of every model); the k posterior matrices are never materialised
 * by hibag_hip_predict_merge, which reads each model's un-normalised ensemble sums.  The environment variable
 * HIBAG_MERGE_CHUNK (samples) asks for smaller chunks; results do not depend on the chunking. */
#define HIBAG_HIP_MERGE_BUDGET_BYTES ((size_t)1 << 30)
typedef struct hibag_hip_merge_plan hibag_hip_merge_plan;
/* NULL on failure (hibag_hip_last_error says why).  The plan lives on `device`, where its models must be. */
hibag_hip_merge_plan *hibag_hip_merge_plan_new(int n_models, const int32_t *n_src_cell, const int32_t *const *row_of_cell,
	int n_merged_hla, int device);
void hibag_hip_merge_plan_free(hibag_hip_merge_plan *plan);
/* The merge alone, on device buffers: d_postprob[i] [n_samp][n_src_cell[i]] and d_matching[i] [n_samp] as
 * hibag_hip_predict_device wrote them.  Enqueued on `stream`, no synchronisation; any output may be NULL (H1 and H2 only
 * together); ld_out >= n_samp is the row stride of d_dosage and d_postprob_out.  The plan owns the scratch of the merge:
 * calls on one plan go to one stream, or are ordered by the caller. */
int hibag_hip_merge_device(hibag_hip_merge_plan *plan, const double *const *d_postprob, const double *const *d_matching,
	const double *weight, int use_matching, int n_samp, int32_t *d_H1, int32_t *d_H2, double *d_max_prob,
	double *d_matching_out, double *d_dosage, double *d_postprob_out, size_t ld_out, void *stream);
/* Host-pointer form, predictions included: uploads the cohort once, then per chunk of samples runs the k predictions
 * (vote_method as in hibag_hip_predict) and the merge behind them on one stream and copies down the outputs that are not
 * NULL (dosage [n_merged_hla][n_samp], postprob [rows][n_samp]).  models[i] are distinct finalized models on the plan's
 * device; the call holds their locks and repairs a failed hand-over like the other host-pointer entries.
 *   geno     the cohort's matrix: int32 [n_samp][n_geno_snp] (snp_major == 0, ld ignored) or [n_geno_snp][ld] (snp_major != 0)
 *   snp_col[i][model i's n_snp]  column / row of each SNP of model i in geno, -1 = absent; snp_col or snp_col[i] NULL =
 *            the model's SNPs are the first n_snp of the cohort, in order
 *   flip[i]  NULL, or != 0 where the allele count is reversed (as hibag_hip_predict_mapped)
 * The _bed form reads a PLINK BED file like hibag_hip_predict_bed (snp_col[i][.] = BED SNP index, required). */
int hibag_hip_predict_merge(hibag_hip_merge_plan *plan, hibag_hip_model *const *models, const int32_t *geno, int snp_major,
	size_t ld, int n_samp, int n_geno_snp, const int32_t *const *snp_col, const int32_t *const *flip, int vote_method,
	const double *weight, int use_matching, int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage,
	double *postprob);
int hibag_hip_predict_merge_bed(hibag_hip_merge_plan *plan, hibag_hip_model *const *models, const char *bed_fn, int n_samp,
	int n_snp, const int32_t *const *snp_col, const int32_t *const *flip, int vote_method, const double *weight,
	int use_matching, int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);

/* Device-pointer form of the same call: every pointer is device memory on the
 * model's device, work is enqueued on `stream` (a hipStream_t, NULL = default
 * stream) and the call returns without synchronising.  A return of 0 means
 * "enqueued": whether the launch could vouch for its sums is the model's status,
 * see "launch status" below (outputs are NA / NaN if it could not). */
int hibag_hip_predict_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp,
	int vote_method, int32_t *d_H1, int32_t *d_H2, double *d_max_prob,
	double *d_matching, double *d_dosage, double *d_postprob, void *stream);

/* hlaPredict()'s SNP selection and strand / allele-order fix-up (R/HIBAG.R:640-676: the rows of the
 * cohort's matrix picked by match(), absent SNPs as NA rows, hlaGenoSwitchStrand's g -> 2 - g) done on the
 * device while the genotypes are packed, instead of building a second matrix on the host:
 *   geno        int32 [n_samp][n_geno_snp]: the COHORT's matrix, its own SNPs in its own order
 *   snp_col[model n_snp]  0-based column of each model SNP in geno, -1 = the cohort lacks it
 *   flip[model n_snp]     NULL, or != 0 where the allele count must be reversed
 * Otherwise as hibag_hip_predict / hibag_hip_predict_device (the _device form takes every pointer,
 * snp_col and flip included, in device memory). */
int hibag_hip_predict_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);
int hibag_hip_predict_mapped_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int n_geno_snp,
	const int32_t *d_snp_col, const int32_t *d_flip, int vote_method,
	int32_t *d_H1, int32_t *d_H2, double *d_max_prob, double *d_matching, double *d_dosage,
	double *d_postprob, void *stream);

/* The same for a cohort matrix stored SNP-MAJOR -- geno[row * ld + sample], one row of n_samp genotypes per SNP, `ld` >= n_samp
 * elements from one row to the next: a C / numpy [snp][sample] array, i.e. the TRANSPOSE of the memory R hands
 * HIBAG_Predict_* (R/HIBAG.R:715-725), which a host that is not R would otherwise have to transpose first.
 *   snp_col[model n_snp]  row of each model SNP in geno, -1 = the cohort lacks it; NULL = row k holds model SNP k
 *   flip[model n_snp]     NULL, or != 0 where the allele count must be reversed
 * The host-pointer form uploads only the rows the model uses (one block of the caller's matrix when they are consecutive,
 * otherwise gathered through pinned staging); no transpose happens anywhere -- the kernels' packed form is SNP-major itself.
 * Results are bit-identical to hibag_hip_predict_mapped on the transposed matrix. */
int hibag_hip_predict_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);
int hibag_hip_predict_snp_major_device(hibag_hip_model *m, const int32_t *d_geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *d_snp_col, const int32_t *d_flip, int vote_method,
	int32_t *d_H1, int32_t *d_H2, double *d_max_prob, double *d_matching, double *d_dosage,
	double *d_postprob, void *stream);

/* ---- launch status of the device-pointer entries ---------------------------------------------------------
 *
 * The last rounds of a pass are cut into chunks that hand their running sums over through the L2 of one XCD
 * ("Hand-overs").  That rests on observed dispatch behaviour, so every hand-over is checked
 * on the device, and one that never arrives (or crosses XCDs) can NOT come back to the caller as numbers:
 *   - the launch's outputs are poisoned on the device: H1 = H2 = NA_integer_, max_prob / matching / dosage /
 *     postprob = NaN for every sample of the batch (partial sums: the three scalar rows are NaN, which survives an
 *     all-reduce and poisons hibag_hip_finish_device's outputs the same way);
 *   - the model gets a STICKY status HIBAG_HIP_EHANDOVER: hibag_hip_model_status() (which waits for the model's
 *     outstanding launches first), hibag_hip_get_timing() and every further compute entry on the model return it until
 *     hibag_hip_model_clear_status() -- the convention of the reference, whose entries never return garbage
 *     (CORE_TRY / CORE_CATCH, src/HIBAG.cpp:41-60; the RAII try_final_* guards, src/LibHLA.cpp:2307-2315);
 *   - from the first such fault on the model launches WITHOUT hand-overs (every work item undivided), so the
 *     caller's second attempt -- clear the status, call again, same process -- cannot fail the same way.
 * The host-pointer entries (hibag_hip_predict, _mapped, _bed, _multi) do all of that themselves:
 * they see the fault when they synchronise, run the call again without hand-overs and return the repaired result
 * with code 0; hibag_hip_model_handover_faults() counts how often that (or a sticky fault) happened.
 *
 * Protocol for a device-pointer caller:   enqueue ... ; synchronise the stream ;
 *     if (hibag_hip_model_status(m) == HIBAG_HIP_EHANDOVER) { hibag_hip_model_clear_status(m); enqueue again; }
 *
 * Streams: a model owns ONE workspace.  Calls on the same model from different streams (or host threads) are legal:
 * the library chains them on the device with an event, each waits for the one enqueued before it.  For concurrency
 * across streams or devices use one model per stream / device (hibag_hip_model_replicate). */
int hibag_hip_model_status(hibag_hip_model *m);
int hibag_hip_model_clear_status(hibag_hip_model *m);
int64_t hibag_hip_model_handover_faults(const hibag_hip_model *m);
/* Fault injection for the tests of the above: the next batch on the model drops the first hand-over of pass `pass`
 * (1 or 2; 0 = disarm) and uses a short time-out.  Not for production use. */
int hibag_hip_test_inject_handover_fault(hibag_hip_model *m, int pass);
/* The chunked tail at small shapes, for the tests (DESIGN.md "The chunked tail, replayed and forced").  Not for production use.
 *
 * hibag_hip_test_set_chunking: on a finalized model, a positive slots_pass1 / slots_pass2 replaces the number of resident
 * workgroups the device reported for pass 1 (all four builds of k_total) / pass 2 (k_accum) by min(reported, value) -- it can
 * only be lowered -- and tail_k in 1 .. 64 becomes the chunks per item of both passes (what HIBAG_TAIL_K sets process-wide).
 * 0 restores that argument's default.  Where the device reported nothing (0) chunking stays off, and a model that has had a
 * failed hand-over keeps launching without chunks.  Finalizing the model again forgets the hook.
 *
 * hibag_hip_test_last_launch: what the model's most recent passes 1 and 2 launched (a predict step's; zeros before the first).
 *
 * hibag_hip_test_plan_total / _accum: the launchers' arithmetic alone, every input given: no device, no model.  They fill
 * the p1_* resp. p2_* plan fields of `out` and zero the rest.  gx = group quads (of 4 x 64 samples), n_item = the model's
 * work items, slots_few / slots_many = resident workgroups of the five- and the six-per-CU build, k_req = chunks asked for
 * (1 .. 64); nx = pass-2 items per XCD (group quads x tiles), slots = resident workgroups of k_accum on the device. */
typedef struct hibag_hip_launch_info {
	int32_t p1_launches;   /* passes 1 of the model so far */
	int32_t p1_kernel;     /* 1: k_total was launched (0: no classifier, or none that k_total walks) */
	int32_t p1_n;          /* work items = group quads x items */
	int32_t p1_slots;      /* resident workgroups of the build chosen (0 = unknown) */
	int32_t p1_k;          /* chunks per cut item (1: none cut) */
	int32_t p1_n_whole;    /* undivided items: workgroups [0, n_whole) */
	int32_t p1_rest;       /* cut items (0: none) */
	int32_t p1_stride;     /* rest rounded up to a multiple of 8 */
	int32_t p1_grid;       /* workgroups = n_whole + K * stride */
	int32_t p1_many;       /* 1: the FP4-only build at six workgroups per CU */
	int32_t p1_walk;       /* the build's walk: 0 = every engine, 1 = FP4-only on generated rows, 2 = FP4-only on prebuilt rows */
	int32_t p1_store;      /* 1: the build that stores every cell sum */
	int32_t p1_vote;       /* 1: the majority vote's build */
	int32_t p2_launches;   /* passes 2 (vote_method 1) of the model so far */
	int32_t p2_kernel;     /* 0 = none, 1 = k_accum (the block stream), 2 = k_accum_cells (every cell read back: never chunked) */
	int32_t p2_nx;         /* items per XCD */
	int32_t p2_sx;         /* resident workgroups per XCD */
	int32_t p2_k;          /* chunks per cut item */
	int32_t p2_n_whole;    /* undivided items per XCD */
	int32_t p2_grid;       /* workgroups = 8 * (n_whole + K * (nx - n_whole)) */
} hibag_hip_launch_info;
int hibag_hip_test_set_chunking(hibag_hip_model *m, int slots_pass1, int slots_pass2, int tail_k);
int hibag_hip_test_last_launch(hibag_hip_model *m, hibag_hip_launch_info *out);
int hibag_hip_test_plan_total(int gx, int n_item, int slots_few, int slots_many, int k_req, int vote, int all_fp4, int split,
	hibag_hip_launch_info *out);
int hibag_hip_test_plan_accum(int nx, int slots, int k_req, hibag_hip_launch_info *out);
/* Kept for ABI compatibility: writes n (<= 40) zeros to `out` and returns 0.  (It read the clock sums of diagnostic kernel
 * builds that no longer exist.) */
int hibag_hip_test_read_diag(hibag_hip_model *m, unsigned long long *out, int n);

/* How classifier `classifier` of a finalized model computes its distances: *engine = HIBAG_HIP_ENGINE_VALU (bit logic +
 * popcount on the vector ALU), _FP4 (v_mfma_scale_f32_32x32x64_f8f6f4, *k_steps instructions per sample half and
 * 32-pair block) or _I8 / _I8S (v_mfma_i32_32x32x32_i8, two K blocks); what bench.py prices its issue floor with. */
#define HIBAG_HIP_ENGINE_VALU 0
#define HIBAG_HIP_ENGINE_FP4  1
#define HIBAG_HIP_ENGINE_I8   2
#define HIBAG_HIP_ENGINE_I8S  3
int hibag_hip_model_engine(const hibag_hip_model *m, int classifier, int *engine, int *k_steps);

/* ---- several devices of one node: replaces hlaPredict(cl = <cluster>) ----------------------------------------
 *
 * The reference spreads a cohort over the workers of a `parallel` cluster: contiguous sample slices, every worker
 * holding the whole model, results concatenated (R/HIBAG.R:764-808).  Here a "worker" is a device:
 *   hibag_hip_model_replicate  a finalized copy of `m` on `device` (the model takes about 12 bytes per listed haplotype pair -- 11 MB for the benchmark model; every device holds all of it)
 *   hibag_hip_predict_multi    hibag_hip_predict over `n_models` replicas at once: one host thread per replica, each
 *                              takes the contiguous slice hibag_hip_multi_slice gives it and writes its part of every
 *                              output in place.  Samples are independent (src/LibHLA.cpp:2362-2411): no collective, and
 *                              every output is bit-identical to the single-device call.  The replicas may sit on any
 *                              devices, also several on one.
 *   hibag_hip_multi_slice      the slice of replica i: [*first, *first + *count) -- boundaries on multiples of 64 samples. */
hibag_hip_model *hibag_hip_model_replicate(const hibag_hip_model *m, int device);
int hibag_hip_multi_slice(int n_samp, int n_models, int i, int *first, int *count);
int hibag_hip_predict_multi(hibag_hip_model *const *models, int n_models, const int32_t *geno, int n_samp,
	int vote_method, int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);

/* Classifier-sharded partial pass for multi-GPU runs: each rank owns a model
 * holding a subset of the classifiers but built with the FULL model's per-SNP
 * classifier counts (snp_weight[n_snp], _GetSNPWeights src/LibHLA.cpp:2484-2496,
 * which the classifier weights depend on).  Writes the un-normalised partial
 * ensemble sums so that one sum all-reduce merges ranks:
 *   d_partial [n_hla(n_hla+1)/2 + 3][n_pad]  (n_pad = n_samp rounded up to 64):
 *   rows 0..P-1 sum_c w_c*prob_c, row P sum_c w_c (_Sum_Weight), row P+1
 *   sum_c w_c*total_c (sum_matching), row P+2 sum_c w_c (num_matching,
 *   src/LibHLA.cpp:2458-2459).  hibag_hip_finish_device() turns merged partials into the
 *   PredictHLA outputs. */
int hibag_hip_model_set_snp_weights(hibag_hip_model *m, const int32_t *snp_weight);
int hibag_hip_predict_partial_device(hibag_hip_model *m, const int32_t *d_geno,
	int n_samp, double *d_partial, void *stream);
int hibag_hip_finish_device(hibag_hip_model *m, const double *d_partial, int n_samp,
	int32_t *d_H1, int32_t *d_H2, double *d_max_prob, double *d_matching,
	double *d_dosage, double *d_postprob, void *stream);

/* The same split driven from ONE process over the devices of a node, merged by RCCL (hibag_amd/csrc/hibag_shard.hip) --
 * what an R / C++ host uses where the model is too large to replicate, or a batch too small to be worth slicing:
 *   hibag_hip_shard_bounds      classifiers [*first, *first + *count) of shard `shard` of `n_shards` (sizes differ by at most one)
 *   hibag_hip_model_shard       that run of `src`'s classifiers as a model of its own on `device`, built with the FULL
 *                               model's per-SNP classifier counts; finalized if `src` is
 *   hibag_hip_model_batch_limit samples one call of hibag_hip_predict_partial_device takes (0 = not finalized)
 *   hibag_hip_shard_group_new   n shards of ONE model, each on its device: one RCCL rank per distinct device
 *                               (ncclCommInitAll; shards sharing a device are added up on it first, in shard order),
 *                               a stream and the batch buffers per rank.  RCCL (librccl.so.1) is loaded here, not before.
 *   hibag_hip_shard_group_predict   CAttrBag_Model::PredictHLA with vote_method 1 (averaged posteriors) on host pointers, as
 *                               hibag_hip_predict: per batch the genotypes go to every rank, every shard writes its
 *                               un-normalised partial sums (the sum split is src/LibHLA.cpp:2448-2476 with :1497-1518),
 *                               ONE ncclAllReduce(ncclDouble, ncclSum) of [P + 3][n_pad] doubles merges them over xGMI,
 *                               rank 0 finishes.  The order of the classifiers' additions changes with the split, and the
 *                               split defines it: shards on ONE device give the in-order sum (each shard its classifiers
 *                               in order from +0.0, then the shards in shard order) in its bits -- one classifier per shard
 *                               is the unsharded result, a shard without classifiers adds +0.0 --, TWO devices each their
 *                               in-order sum and then one commutative addition, in its bits too; over more than two ranks
 *                               the all-reduce's order is RCCL's: calls identical to the unsharded run's up to ties at
 *                               rounding level between a sample's two best cells, posteriors within 1e-10 relative.  A failed
 *                               hand-over on any shard reaches every rank as NaN through the sum and the batch is run again.
 *   hibag_hip_predict_multi_sharded   group_new + group_predict + group_free in one call (pays the communicator set-up each time)
 *   hibag_hip_shard_group_ranks / _allreduces   RCCL ranks of the group, all-reduces it has issued;  hibag_hip_rccl_version: NCCL_VERSION_CODE of the loaded library, 0 = none
 * The reference's own multi-worker branch (R/HIBAG.R:764-808) splits samples: that is hibag_hip_predict_multi above. */
typedef struct hibag_hip_shard_group hibag_hip_shard_group;
int hibag_hip_shard_bounds(int n_classifier, int n_shards, int shard, int *first, int *count);
hibag_hip_model *hibag_hip_model_shard(const hibag_hip_model *src, int shard, int n_shards, int device);
int hibag_hip_model_batch_limit(const hibag_hip_model *m);
hibag_hip_shard_group *hibag_hip_shard_group_new(hibag_hip_model *const *shards, int n_shards);
void hibag_hip_shard_group_free(hibag_hip_shard_group *g);
int hibag_hip_shard_group_ranks(const hibag_hip_shard_group *g);
int64_t hibag_hip_shard_group_allreduces(const hibag_hip_shard_group *g);
int hibag_hip_rccl_version(void);
int hibag_hip_shard_group_predict(hibag_hip_shard_group *g, const int32_t *geno, int n_samp,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);
int hibag_hip_predict_multi_sharded(hibag_hip_model *const *shards, int n_shards, const int32_t *geno, int n_samp,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);

/* ---- PLINK BED input: replaces HIBAG_BEDFlag + HIBAG_ConvBED --------------- */

/* HIBAG_BEDFlag(bed.fn) (src/HIBAG.cpp:1068-1081): returns the storage-mode byte
 * of the file (0 = individual-major, otherwise SNP-major) or a negative error
 * with the reference's messages ("Cannot open the file %s.", "Invalid prefix in
 * the PLINK BED file.").  Host only. */
int hibag_hip_bed_flag(const char *bed_fn);

/* HIBAG_ConvBED(bed.fn, n.samp, n.snp, n.save.snp, snp.flag) (src/HIBAG.cpp:1094-1191):
 * decodes the 2-bit genotypes of the SNPs with snp_flag[j] != 0 (R logical
 * vector, n_snp entries, n_save_snp of them set) on the device into
 *   geno  int32 [n_samp][n_save_snp]  (the memory of R's n_save_snp x n_samp matrix),
 * values 2 / NA_integer_ / 1 / 0 for the codes 0 / 1 / 2 / 3 (:1135).  Only the
 * selected SNP rows of a SNP-major file are read and uploaded.  Unlike the
 * reference, a file shorter than n_samp x n_snp genotypes is an error (EINVAL)
 * rather than a silent reuse of the previous row. */
int hibag_hip_conv_bed(const char *bed_fn, int n_samp, int n_snp, int n_save_snp,
	const int32_t *snp_flag, int32_t *geno);

/* hlaBED2Geno() + hlaPredict() fused: PredictHLA (as hibag_hip_predict) with the
 * genotypes decoded on the device straight from the BED file into the packed
 * form the kernels use, without materialising the int32 matrix (16x less
 * host->device traffic).
 *   n_samp, n_snp   dimensions of the BED file (.fam / .bim line counts)
 *   snp_col[model n_snp]  0-based BED SNP index of each model SNP, -1 = the
 *                   cohort lacks it (treated as missing, like the NA rows
 *                   hlaPredict builds, R/HIBAG.R:640-660)
 *   flip[model n_snp]     NULL, or != 0 where the allele count must be
 *                   reversed, g -> 2 - g (A/B order or strand differs between
 *                   cohort and model, R/HIBAG.R:661-676, src/HIBAG.cpp:221-342)
 * All samples of the file are predicted, in file order. */
int hibag_hip_predict_bed(hibag_hip_model *m, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method,
	int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage, double *postprob);

/* ---- top-k: each sample's k best allele pairs: hlaPredictTopK ----------------
 * Between "one pair" and "the whole posterior matrix": per sample the k largest cells of the NORMALISED ensemble matrix
 * -- exactly the values the postprob output of hibag_hip_predict holds for that vote_method -- as allele pairs with their
 * probabilities, selected on the device; k * 20 + 8 bytes per sample come back instead of 8 * n_hla (n_hla + 1) / 2.
 * The ranking rule:
 *   rank 0 is the call of hibag_hip_predict (BestGuessEnsemble, src/LibHLA.cpp:1549-1566): the first strict maximum in
 *   pair order, only values > 0; rank r is the first strict maximum among the pairs not yet listed, again only values > 0
 *   -- descending probability, equal probabilities in ascending pair order; a pair whose value is 0 or NaN is never listed.
 * Outputs, sample-major:
 *   h1, h2 [n_samp][k]   0-based allele indices (h1 <= h2), HIBAG_HIP_NA_INTEGER in the ranks no pair qualifies for
 *   prob   [n_samp][k]   the pairs' posterior probabilities, 0 in those ranks; h1[s][0], h2[s][0], prob[s][0] are
 *                        bit for bit the H1, H2, max_prob of hibag_hip_predict
 *   matching [n_samp]    as hibag_hip_predict; may be NULL
 * h1, h2 and prob are required; 1 <= k <= HIBAG_HIP_TOPK_MAX, vote_method 1 or 2; HIBAG_HIP_EINVAL otherwise.  No dosage
 * and no posterior matrix (ask hibag_hip_predict for those).  Everything else -- batches, the host-pointer pipeline, the
 * repair of a failed hand-over (poisoned outputs are NA pairs and NaN probabilities in every rank), the launch status of
 * the _device form -- is as for the sibling entry of the same suffix, whose other arguments these take in the same
 * order.  (Added within ABI version 7) */
#define HIBAG_HIP_TOPK_MAX 16
int hibag_hip_predict_topk(hibag_hip_model *m, const int32_t *geno, int n_samp, int vote_method, int k,
	int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_topk_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int vote_method, int k,
	int32_t *d_h1, int32_t *d_h2, double *d_prob, double *d_matching, void *stream);
int hibag_hip_predict_topk_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int k,
	int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_topk_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int k,
	int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_topk_bed(hibag_hip_model *m, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int k,
	int32_t *h1, int32_t *h2, double *prob, double *matching);

/* ---- posterior draws: allele pairs sampled from each sample's posterior: hlaPredictDraws ----------------
 * For analyses that carry the imputation's uncertainty (multiple imputation, haplotype or amino-acid models): per sample
 * n_draw allele pairs drawn from the NORMALISED ensemble matrix -- exactly the values the postprob output of
 * hibag_hip_predict holds for that vote_method -- sampled on the device; n_draw * 20 + 8 bytes per sample come back
 * instead of 8 * n_hla (n_hla + 1) / 2.  The rule, p[c] the sample's posterior in pair order:
 *   cum[c] = cum[c - 1] + p[c] in plain double additions in pair order (no FMA), S = the last cum;
 *   draw t of sample i uses u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, where (w0, w1, ., .) =
 *   Philox4x32-10(counter = (i & 0xffffffff, i >> 32, t, 0), key = (seed & 0xffffffff, seed >> 32));
 *   the drawn pair is the first c with cum[c] > u * S (one double multiply); a pair of probability 0 is never drawn.
 * i = sample0 + the sample's index in the call: sample0 >= 0 is the index of the call's first sample in the caller's own
 * numbering, so that a cohort cut into several calls (or a window of a resident cohort: the _cohort entry does NOT add
 * `first` itself) draws what one call over the whole cohort draws.  A sample's draws depend on (seed, i, t) and its
 * posterior alone -- not on batches, routes, a repaired hand-over or n_draw: the first n draws of a call with more are
 * the draws of a call with n.  (R's sample(prob =) stream is deliberately not mirrored: DESIGN.md section 16.)
 * Outputs, sample-major:
 *   h1, h2 [n_samp][n_draw]   0-based allele indices (h1 <= h2); HIBAG_HIP_NA_INTEGER in every draw of a sample whose
 *                             S > 0 is false (nothing positive, or NaN)
 *   prob   [n_samp][n_draw]   the drawn pairs' posterior probabilities; for such a sample NaN if S is NaN (an underflow
 *                             poisoned it), 0 otherwise
 *   matching [n_samp]         as hibag_hip_predict; may be NULL
 * h1, h2 and prob are required; 1 <= n_draw <= HIBAG_HIP_DRAW_MAX, sample0 >= 0, vote_method 1 or 2; HIBAG_HIP_EINVAL
 * otherwise.  Everything else is as for the top-k entry of the same suffix, whose other arguments these take in the same
 * order.  (Added within ABI version 7) */
#define HIBAG_HIP_DRAW_MAX 64
int hibag_hip_predict_draw(hibag_hip_model *m, const int32_t *geno, int n_samp, int vote_method, int n_draw, uint64_t seed,
	int64_t sample0, int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_draw_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int vote_method, int n_draw,
	uint64_t seed, int64_t sample0, int32_t *d_h1, int32_t *d_h2, double *d_prob, double *d_matching, void *stream);
int hibag_hip_predict_draw_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int n_draw, uint64_t seed, int64_t sample0,
	int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_draw_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int n_draw, uint64_t seed, int64_t sample0,
	int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_draw_bed(hibag_hip_model *m, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, int n_draw, uint64_t seed, int64_t sample0,
	int32_t *h1, int32_t *h2, double *prob, double *matching);

/* ---- resident cohort: one cohort's genotypes kept on a device for many calls -------
 * A run types one cohort at every locus, and then asks again (the k best pairs, both vote methods, a second ancestry's
 * model).  Every entry above takes the raw genotypes again on each call -- 4 bytes per genotype up the bus and a decode per
 * model.  A cohort keeps them on ONE device at 2 bits per genotype: SNP-major rows in PLINK's own codes (00 = 2, 01 = missing,
 * 10 = 1, 11 = 0; four samples per byte, lowest bits first), rows a multiple of 16 bytes apart, the slots behind the last
 * sample missing -- the payload of a SNP-major BED file, so a matrix and a file share the decode of hibag_hip_predict_bed
 * and everything behind it.  A cohort is immutable once built; calls on different models may share it from different threads.
 *   hibag_hip_cohort_new       from an int32 matrix: geno[snp * ld + sample] (snp_major != 0, ld >= n_samp) or
 *                              geno[sample * ld + snp] (snp_major == 0, the memory of R's SNP x sample matrix, ld >= n_snp);
 *                              anything outside 0..2 is missing (as hibag_hip_predict).  snp_rows[n_rows] selects the SNPs
 *                              that become rows 0 .. n_rows - 1 of the cohort, in that order (NULL: all n_snp, n_rows ignored).
 *                              The matrix goes up in slabs through pinned staging and is packed on the device: it is never
 *                              resident whole.  On the calling thread's device (hibag_hip_set_device).  At most 2^30 samples.
 *   hibag_hip_cohort_from_bed  the same from a PLINK BED file of n_samp x n_snp genotypes, either storage mode; checked like
 *                              hibag_hip_predict_bed (same messages; a short file is an error).  snp_rows: BED SNP indices.
 * Both return NULL on failure (hibag_hip_last_error says why).
 *   hibag_hip_cohort_snp_counts  per row the number of called genotypes (int32) and their sum (int64), exact; what the
 *                              allele frequencies of hlaPredict's strand check are made of
 *   hibag_hip_predict_cohort   hibag_hip_predict_mapped for samples [first, first + count) of the cohort, host-pointer
 *                              outputs: snp_col[model n_snp] = cohort row of each model SNP (-1 = absent), flip as there.
 *                              Batches, the download pipeline and the repair of a failed hand-over are those of the other
 *                              host-pointer entries; the call takes the model's lock.  Bit-identical to hibag_hip_predict_mapped
 *                              on the matrix the cohort was made from.  HIBAG_HIP_EINVAL (with a message) when cohort and
 *                              model are on different devices, the window leaves the cohort, or a snp_col entry is >= n_snp.
 *   hibag_hip_predict_topk_cohort  the same with the top-k output set (see "top-k" above).
 *   hibag_hip_predict_draw_cohort  the same with the draw output set (see "posterior draws" above); pass sample0 = first
 *                              to draw what a call over the whole cohort draws for these samples. */
typedef struct hibag_hip_cohort hibag_hip_cohort;
hibag_hip_cohort *hibag_hip_cohort_new(const int32_t *geno, int snp_major, size_t ld, int n_samp, int n_snp,
	const int32_t *snp_rows, int n_rows);
hibag_hip_cohort *hibag_hip_cohort_from_bed(const char *bed_fn, int n_samp, int n_snp, const int32_t *snp_rows, int n_rows);
void hibag_hip_cohort_free(hibag_hip_cohort *c);
int hibag_hip_cohort_device(const hibag_hip_cohort *c);     /* -1 for NULL */
int hibag_hip_cohort_n_samp(const hibag_hip_cohort *c);
int hibag_hip_cohort_n_snp(const hibag_hip_cohort *c);      /* rows held */
int64_t hibag_hip_cohort_bytes(const hibag_hip_cohort *c);  /* device memory of the rows */
int hibag_hip_cohort_snp_counts(const hibag_hip_cohort *c, int32_t *n_valid, int64_t *sum);
int hibag_hip_predict_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int32_t *H1, int32_t *H2, double *max_prob, double *matching, double *dosage,
	double *postprob);
int hibag_hip_predict_topk_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int k, int32_t *h1, int32_t *h2, double *prob, double *matching);
int hibag_hip_predict_draw_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, int n_draw, uint64_t seed, int64_t sample0, int32_t *h1, int32_t *h2, double *prob,
	double *matching);

/* ---- allele groups: calls under the posterior collapsed over groups of alleles: hlaPredictGroups ----------------
 * Imputed types are mostly analysed at a coarser level than the four-digit pair: two-digit types, P / G groups, serological
 * groups, the amino acid at a position of the protein.  Each is a PARTITION of the model's alleles into groups, and the call
 * at that level is the maximum of the collapsed posterior -- the pair posterior summed over the allele pairs that fall into
 * each pair of groups --, not the relabelled allele-level call.  A plan holds n_part partitions of one model's alleles; the
 * group entries compute, per sample and partition, on the device from the ensemble sums: the best pair of groups, its
 * probability and (optionally) the expected dosage of every group.  n_part * 16 + 8 bytes per sample come back (+ 8 per group
 * with the dosages) instead of 8 * n_hla (n_hla + 1) / 2.
 * The rule (exact), p[c] the sample's NORMALISED posterior in pair order -- the values the postprob output of
 * hibag_hip_predict holds for that vote_method --, cell c = the pair (h1 <= h2), m(h) in 0 .. G - 1 the group of allele h:
 *   bin (a <= b) has index b + a (2 G - a - 1) / 2; a cell belongs to the bin (min, max) of (m(h1), m(h2));
 *   B[bin] = the sum of p[c] over the bin's cells in increasing c, plain double additions from +0.0 (no FMA); empty: +0.0;
 *   the call is the first bin in bin order with best < B strictly, best starting at 0 (hibag_hip_predict's own rule, on
 *   bins); a bin whose sum is NaN never wins;
 *   D[g] = the sum, over the cells with m(h1) = g or m(h2) = g in increasing c, of p[c] -- or 2 p[c] where both are.
 * With m(h) = h this is hibag_hip_predict's H1, H2, max_prob and dosage bit for bit.  Results do not depend on batches,
 * routes, a repaired hand-over, the other partitions of the plan or on whether the dosages were asked for.
 *   hibag_hip_groups_create  group_of[n_part][n_hla]: the group of every allele in every partition, ids 0 .. n_hla - 1
 *                            (G = the largest id of the partition + 1; an id no allele has is an empty group that never
 *                            wins and has dosage 0).  1 <= n_part <= HIBAG_HIP_GROUPS_MAX_PART, the G of all partitions
 *                            together <= HIBAG_HIP_GROUPS_MAX_LEVELS; HIBAG_HIP_EINVAL otherwise.  The model must be
 *                            finalized; the plan lives on its device and is taken with THAT model only (EINVAL otherwise).
 *                            Freeing the model does not free its plans.
 *   hibag_hip_groups_levels  counts[n_part] = G of every partition
 *   hibag_hip_groups_tile    samples per workgroup of the finish kernel for this plan; *lds (may be NULL) = 1 if their
 *                            posteriors are staged in LDS, 0 if the kernel reads the ensemble sums directly (the model's
 *                            posterior does not fit, or HIBAG_GROUPS_NO_LDS=1 in the environment: read at every call)
 * Outputs of the entries, sample-major:
 *   g1, g2 [n_samp][n_part]   group indices (g1 <= g2); HIBAG_HIP_NA_INTEGER where no bin qualifies
 *   prob   [n_samp][n_part]   the called bin's B; 0 where no bin qualifies, NaN in a poisoned batch
 *   matching [n_samp]         as hibag_hip_predict; may be NULL
 *   dosage [n_samp][D]        D = the G of all partitions together, partition q's groups from the sum of the G before it;
 *                             may be NULL
 * g1, g2 and prob are required.  Everything else is as for the draw entry of the same suffix, whose other arguments these
 * take in the same order.  (Added within ABI version 7) */
#define HIBAG_HIP_GROUPS_MAX_PART 512
#define HIBAG_HIP_GROUPS_MAX_LEVELS 4096
typedef struct hibag_hip_groups hibag_hip_groups;
int hibag_hip_groups_create(hibag_hip_model *m, int n_part, const int32_t *group_of, hibag_hip_groups **plan);
void hibag_hip_groups_free(hibag_hip_groups *plan);
int hibag_hip_groups_levels(const hibag_hip_groups *plan, int32_t *counts);
int hibag_hip_groups_tile(const hibag_hip_groups *plan, int *lds);
int hibag_hip_predict_groups(hibag_hip_model *m, const int32_t *geno, int n_samp, int vote_method, const hibag_hip_groups *plan,
	int32_t *g1, int32_t *g2, double *prob, double *matching, double *dosage);
int hibag_hip_predict_groups_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int vote_method,
	const hibag_hip_groups *plan, int32_t *d_g1, int32_t *d_g2, double *d_prob, double *d_matching, double *d_dosage, void *stream);
int hibag_hip_predict_groups_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const hibag_hip_groups *plan,
	int32_t *g1, int32_t *g2, double *prob, double *matching, double *dosage);
int hibag_hip_predict_groups_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const hibag_hip_groups *plan,
	int32_t *g1, int32_t *g2, double *prob, double *matching, double *dosage);
int hibag_hip_predict_groups_bed(hibag_hip_model *m, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const hibag_hip_groups *plan,
	int32_t *g1, int32_t *g2, double *prob, double *matching, double *dosage);
int hibag_hip_predict_groups_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, const hibag_hip_groups *plan, int32_t *g1, int32_t *g2, double *prob, double *matching,
	double *dosage);

/* ---- partial typing: calls conditioned on what is already known of a sample's type: hlaPredictGiven ----------------
 * Many cohorts carry partial typing at the locus -- serology, two-digit types, one allele typed and the other not, an
 * ambiguity list of sequence-based typing -- and want the four-digit call CONSISTENT with it.  The constraint is a per-sample
 * input: two allele sets A and B, each a bit mask over the model's alleles.  The given entries compute, per sample, on the
 * device from the ensemble sums: the best pair among the consistent cells, its probability, the posterior mass of the
 * consistent cells and (optionally) every allele's dosage restricted to them.  24 bytes per sample come back (+ 8 n_hla with
 * the dosages) instead of 8 * n_hla (n_hla + 1) / 2.
 * The rule (exact), p[c] the sample's NORMALISED posterior in pair order -- the values the postprob output of
 * hibag_hip_predict holds for that vote_method --, cell c = the pair (h1 <= h2), c = h2 + h1 (2 n_hla - h1 - 1) / 2:
 *   cell (h1, h2) is consistent iff (h1 in A and h2 in B) or (h1 in B and h2 in A);
 *   support = the sum of p[c] over the consistent cells in increasing c: plain double additions from +0.0 (no FMA, no
 *   reassociation), one serial sum;
 *   the call is the first consistent cell in cell order with best < p[c] strictly, best starting at 0 (hibag_hip_predict's
 *   own rule, on the consistent cells); prob = p[that cell], the JOINT probability: it is not divided by support.  No such
 *   cell: NA / NA with prob 0.  A NaN cell never wins; where it is consistent it makes support NaN.  A NaN weight sum (a
 *   poisoned batch) gives NA / NA with prob and support NaN, whatever the sets;
 *   dosage[h] = the sum, over the consistent cells that contain h in increasing c, of p[c] -- 2 p[c] (exact) on the diagonal
 *   cell; joint values too.  A NaN weight sum gives that NaN, as in hibag_hip_predict.
 * The conditional probability is prob / support and the conditional dosage dosage / support, one IEEE division each; the
 * CALLER forms them.  (The sum of p over all cells is not exactly 1, so a device that divided could not keep the next line.)
 * With A and B both full, h1, h2, prob, dosage and matching are hibag_hip_predict's H1, H2, max_prob, dosage and matching bit
 * for bit, NaN cases included, and support is the running sum of the posterior row in pair order (the S of the draw
 * entries).  Swapping A and B changes nothing; an empty A or B gives the "no such cell" result with support +0.0.  Results do
 * not depend on batches, slices, routes, a repaired hand-over, the other samples' sets or on which optional outputs were
 * asked for.
 *   allow  uint32 [n_samp][2][W], W = (n_hla + 31) / 32: sample s, set A (0) or B (1); allele h is bit h % 32 of word h / 32;
 *          bits at or above n_hla are ignored.  Host memory for the host-pointer entries, device memory for _device.  In
 *          _bed and _cohort it is indexed like the outputs: by the call's sample, not by the file's or the cohort's.
 * Outputs, [n_samp] each unless stated:
 *   h1, h2    allele indices (h1 <= h2); HIBAG_HIP_NA_INTEGER where no consistent cell qualifies
 *   prob      the called cell's p (joint); 0 where none qualifies, NaN in a poisoned batch
 *   support   as above
 *   matching  as hibag_hip_predict; may be NULL
 *   dosage    [n_samp][n_hla]; may be NULL
 * h1, h2, prob and support are required.  HIBAG_HIP_EINVAL, with a message in hibag_hip_last_error: a NULL allow or a missing
 * required output together with n_samp > 0, a bad vote_method, a model that is not finalized.  n_samp == 0 with NULL
 * pointers returns 0.  There is no bound on n_hla beyond the model's own.  Everything else is as for the draw entry of the
 * same suffix, whose arguments these take in the same order with (n_draw, seed, sample0) replaced by allow.  (Added within
 * ABI version 7) */
int hibag_hip_predict_given(hibag_hip_model *m, const int32_t *geno, int n_samp, int vote_method, const uint32_t *allow,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_given_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int vote_method, const uint32_t *d_allow,
	int32_t *d_h1, int32_t *d_h2, double *d_prob, double *d_support, double *d_matching, double *d_dosage, void *stream);
int hibag_hip_predict_given_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const uint32_t *allow,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_given_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const uint32_t *allow,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_given_bed(hibag_hip_model *m, const char *bed_fn, int n_samp, int n_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const uint32_t *allow,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_given_cohort(hibag_hip_model *m, const hibag_hip_cohort *c, int first, int count, const int32_t *snp_col,
	const int32_t *flip, int vote_method, const uint32_t *allow, int32_t *h1, int32_t *h2, double *prob, double *support,
	double *matching, double *dosage);

/* ---- pedigrees: children's calls weighted by their parents' posteriors: hlaPredictFamily --------------------------
 * A child's two alleles are one allele of each parent, so the parents' SNPs say a great deal about a child whose own SNPs
 * are sparse.  The family entries take the call's pedigree and weight every sample's posterior, on the device, with the
 * Mendelian transmission probability its parents' results give each allele pair, divided by the pair's prior.  Parents are
 * finished before their children within the call; 24 bytes per sample come back (+ 8 n_hla with the dosages).
 * The rule (exact), p[c] the sample's NORMALISED posterior in pair order -- the values the postprob output of
 * hibag_hip_predict holds for that vote_method --, cell c = the pair (h1 <= h2), c = h2 + h1 (2 n_hla - h1 - 1) / 2:
 *   1 the ratio vector of a parent j with joint dosage D_j (rule 5) and support S_j (rule 3), S_j > 0:
 *       r_j[h] = (0.5 * (D_j[h] / S_j)) / prior[h]    one division, an exact halving, one division (skipped for a NULL prior);
 *     a parent index -1, or a parent whose S_j is not > 0 (zero or NaN), is UNKNOWN: r == 1.0;
 *   2 the weight of a cell:  a = rf[h1] * rm[h2], b = rf[h2] * rm[h1], w[c] = 0.5 * (a + b), x[c] = p[c] * w[c] -- plain double
 *     operations in that order, no FMA.  Both parents unknown: w == 1.0 and x[c] == p[c] bit for bit;
 *   3 support = the sum of x[c] over all cells in increasing c, one serial sum from +0.0;
 *   4 the call is the first cell in cell order with best < x[c] strictly, best starting at 0; prob = x[that cell], the JOINT
 *     value: it is not divided by support.  No such cell: NA / NA with prob 0.  A NaN x never wins and makes support NaN.  A
 *     NaN weight sum (a poisoned batch) gives NA / NA with prob and support NaN;
 *   5 dosage[h] = the sum of x[c] over the cells that contain h in increasing c, 2 x[c] (exact) on the diagonal cell; a NaN
 *     weight sum gives that NaN.  Always formed on the device (descendants need it), returned only if asked for;
 *   6 matching is hibag_hip_predict's.
 * The conditional probability is prob / support and the conditional dosage dosage / support where support > 0; the CALLER
 * forms them.  Information flows DOWN only: a parent that is itself a child transmits its own weighted (D, S); children
 * never change their parents' results, and siblings do not see each other.  For a sample with both parents unknown h1, h2,
 * prob, dosage and matching are hibag_hip_predict's H1, H2, max_prob, dosage and matching bit for bit, NaN cases included,
 * and support is the running sum of the posterior row in pair order.  Swapping father and mother changes nothing.  A
 * sample's result depends on its own genotypes and its ancestors' only: not on batches, slices, routes, a repaired
 * hand-over, the order of unrelated samples or on which optional outputs were asked for.
 * w is the Mendelian transmission probability of the pair under the parents' posteriors divided by the pair's prior
 * (2 - [h1 == h2]) q[h1] q[h2]; support is therefore a Bayes-factor-like "family fit", well below 1 where the child's own
 * SNPs contradict the parents (a sample swap, non-paternity).
 *   pedigree  int32 [n_samp][2]: (father, mother) of sample s as sample indices of THIS call, or -1 for "not in this call".
 *             Every index p of sample s must satisfy -1 <= p < s: parents precede their children.  HOST memory on every
 *             route, _device included: the entry checks it and orders the work by it before anything is launched.
 *   prior     double [n_hla], every entry finite and > 0, or NULL (all 1.0); host memory on every route.  The prior to
 *             give is the one the model's classifiers carry (hlaModelAllelePrior of the Python package).
 * Outputs, [n_samp] each unless stated (device memory for _device):
 *   h1, h2    allele indices (h1 <= h2); HIBAG_HIP_NA_INTEGER where no cell qualifies
 *   prob      the called cell's x (joint); 0 where none qualifies, NaN in a poisoned batch
 *   support   as above
 *   matching  as hibag_hip_predict; may be NULL
 *   dosage    [n_samp][n_hla]; may be NULL
 * h1, h2, prob and support are required.  HIBAG_HIP_EINVAL, with a message in hibag_hip_last_error and before any launch: a
 * NULL pedigree or a missing required output together with n_samp > 0, a parent index outside -1 .. s - 1, a prior entry that
 * is not finite and > 0, a bad vote_method, a model that is not finalized.  n_samp == 0 with NULL pointers returns 0.  The
 * _device entry waits for its upload of pedigree and prior on `stream` before it enqueues the kernels.  There are no _bed
 * and _cohort routes: their sample order is the file's or the cohort's, and the caller cannot arrange for parents to
 * precede children.  Everything else is as for the given entry of the same suffix, whose arguments these take in the same
 * order with allow replaced by (pedigree, prior).  (Added within ABI version 7) */
int hibag_hip_predict_family(hibag_hip_model *m, const int32_t *geno, int n_samp, int vote_method, const int32_t *pedigree,
	const double *prior, int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_family_device(hibag_hip_model *m, const int32_t *d_geno, int n_samp, int vote_method, const int32_t *pedigree,
	const double *prior, int32_t *d_h1, int32_t *d_h2, double *d_prob, double *d_support, double *d_matching, double *d_dosage,
	void *stream);
int hibag_hip_predict_family_mapped(hibag_hip_model *m, const int32_t *geno, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const int32_t *pedigree, const double *prior,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);
int hibag_hip_predict_family_snp_major(hibag_hip_model *m, const int32_t *geno, size_t ld, int n_samp, int n_geno_snp,
	const int32_t *snp_col, const int32_t *flip, int vote_method, const int32_t *pedigree, const double *prior,
	int32_t *h1, int32_t *h2, double *prob, double *support, double *matching, double *dosage);

/* ---- training: replaces HIBAG_Training + HIBAG_NewClassifiers ---------------- */

typedef struct hibag_hip_trainer hibag_hip_trainer;  /* opaque handle */

/* HIBAG_Training(n.snp, n.samp, snp.geno, n.hla, H1, H2) (src/HIBAG.cpp:516-535 ->
 * CAttrBag_Model::InitTraining, src/LibHLA.cpp:2196-2218): snp_geno int32
 * [n_samp][n_snp] (the memory of R's SNP x sample matrix; values outside 0..2 are
 * missing), H1/H2[n_samp] 0-based allele indices < n_hla.  The arrays are copied.
 * Errors carry the reference's messages ("Invalid number of samples: %d.", ...). */
hibag_hip_trainer *hibag_hip_trainer_new(int n_snp, int n_samp, const int32_t *snp_geno, int n_hla,
	const int32_t *H1, const int32_t *H2);
void hibag_hip_trainer_free(hibag_hip_trainer *t);

/* Host threads of the trainer: they pack, reduce and -- in EM mode 1 -- fit the candidate SNPs of a growth step
 * (CAlg_EM::ExpectationMaximization, src/LibHLA.cpp:1185-1255).  The count also SELECTS THE EM ROUTE while the mode is
 * automatic (hibag_hip_trainer_set_em_mode 0, the default; HIBAG_TRAIN_EM=host|device overrides): a trainer with two
 * threads or fewer -- what a torchrun rank on a small quota gets, or a caller passing 1 -- fits on the device, one
 * with more on its threads.  Both routes give the same classifiers bit for bit (the device decides the stopping test
 * with a margin for its own log() and hands the candidates it cannot decide back to a host thread).
 * Default: the CPUs the process may use (affinity mask, cgroup quota) divided by LOCAL_WORLD_SIZE, so that the ranks of
 * one node -- one process per GPU -- share the host instead of oversubscribing it; HIBAG_TRAIN_THREADS overrides the
 * default, n_threads <= 0 restores it.  The counterpart of HIBAG_NewClassifiers' `nthread` (src/HIBAG.cpp:599-634),
 * whose default in hlaAttrBagging is 1 (R/HIBAG.R:48-52): a deviation, see hibag_amd/train.py. */
int hibag_hip_trainer_set_threads(hibag_hip_trainer *t, int n_threads);
int hibag_hip_trainer_threads(const hibag_hip_trainer *t);
/* Where the EM fits of a growth step's candidate SNPs run (CAlg_EM::ExpectationMaximization, src/LibHLA.cpp:1185-1255):
 * 1 = on the trainer's host threads, 2 = on the device (hibag_amd/csrc/hibag_em.hip: workgroup = candidate, every sum in the
 * host's order; the stopping test decided with a margin for the device's log(), candidates it cannot decide handed back to the
 * host), 0 = automatic: the device where the trainer has two host threads or fewer.  Both give the same classifiers bit for bit. */
int hibag_hip_trainer_set_em_mode(hibag_hip_trainer *t, int mode);
/* Of the CALLING THREAD's last hibag_hip_trainer_new_classifiers call: out[0] = candidate SNPs fitted by the device kernel,
 * out[1] = how many of those it handed back to the host (status 2).  Both 0 where the host fitted everything (EM mode 1, or
 * steps too large for the kernel).  (Added within ABI version 7.) */
int hibag_hip_trainer_em_counts(const hibag_hip_trainer *t, long long out[2]);

/* Several trainers of ONE process on one device -- the decomposition of hlaParallelAttrBagging's workers (R/HIBAG.R:329-390:
 * independent classifiers, one random stream per worker) without a process per worker.  A trainer flagged `shared` hands
 * the device work of its growth steps -- the candidate pair lists (src/LibHLA.cpp:1569-1637), the EM fits (:1127-1255), the
 * scoring (:1639-1767) -- to the device's combiners: whichever trainer thread finds a combiner idle launches ONE fused
 * kernel per kind of operation for every trainer that has one pending (hibag_amd/csrc/hibag_combine.h), instead of each
 * trainer queueing short kernels behind the others' on the runtime's few hardware queues.  Classifiers are bit-identical to
 * a trainer that runs alone.  Each shared trainer is still driven by a host thread of its own (hibag_hip_trainer_new_classifiers
 * blocks), but those threads mostly wait: hibag_hip_train_set_thread_budget(n) lets at most n of them be runnable at a
 * time (0 = no limit; process-wide), so sixteen trainers fit the two host threads a rank of an eight-GPU node gets.
 * hibag_hip_train_combine_stats: fused launches and the operations in them since the last reset, by kind
 * (0 / 1 pair lists pass 0 / 1 as operations of their own, 2 scoring, 3 EM fits, 4 pair lists, both passes in one); out
 * arrays of 8 (either may be NULL). */
int hibag_hip_trainer_set_shared(hibag_hip_trainer *t, int shared);
int hibag_hip_train_set_thread_budget(int n_threads);
int hibag_hip_train_combine_stats(long long *launches, long long *ops, int reset);
/* seconds the shared trainers' operations took from hand-over to results, summed by kind [0..7]; seconds spent in fused
 * batches and their number, for the short operations' lane and the EM lane [8..9], [10..11] (measurement only) */
int hibag_hip_train_combine_times(double *out12, int reset);

/* Source of the uniform draws the reference takes from R's unif_rand()
 * (src/LibHLA.cpp:120-126; bootstrap :2236, SNP sampling :957).  An R binding
 * passes a trampoline to unif_rand between GetRNGstate()/PutRNGstate()
 * (src/HIBAG.cpp:611, :632); other hosts call set_seed, which reproduces R's
 * set.seed(seed) + default Mersenne-Twister stream exactly. */
int hibag_hip_trainer_set_rng(hibag_hip_trainer *t, double (*unif_rand)(void *ctx), void *ctx);
int hibag_hip_trainer_set_seed(hibag_hip_trainer *t, uint32_t seed);

/* HIBAG_NewClassifiers(model, nclassifier, mtry, prune, nthread, verbose,
 * verbose.detail, proc_ptr) (src/HIBAG.cpp:599-634 -> CAttrBag_Model::BuildClassifiers,
 * src/LibHLA.cpp:2268-2305): grows `nclassifier` more individual classifiers -- bootstrap,
 * greedy SNP selection, EM haplotype fit -- with the haplotype-pair scoring
 * (build_haplomatch / build_acc_oob / build_acc_ib) on the device.  Given the same
 * random stream the result is bit-identical to the reference's CPU training. */
int hibag_hip_trainer_new_classifiers(hibag_hip_trainer *t, int nclassifier, int mtry, int prune,
	int verbose, int verbose_detail);

/* HIBAG_GetNumClassifiers / HIBAG_GetClassifierList / HIBAG_Classifier_GetHaplos
 * (src/HIBAG.cpp:843-953): read the grown classifiers back.
 *   snpidx[n_snp_c] 0-based, samp_num[n_samp] bootstrap counts, freq/hla[n_haplo],
 *   bits[n_haplo][2] packed haplotypes (bit s = allele of SNP snpidx[s]).
 * Feed them to hibag_hip_model_add_classifier_packed to predict with the new model. */
int hibag_hip_trainer_n_classifier(const hibag_hip_trainer *t);
int hibag_hip_trainer_classifier_dims(const hibag_hip_trainer *t, int idx, int *n_snp_c, int *n_haplo);
int hibag_hip_trainer_classifier_get(const hibag_hip_trainer *t, int idx, int32_t *snpidx, int32_t *samp_num,
	double *freq, int32_t *hla, uint64_t *bits, double *outofbag_acc);

/* ---- kernel timing (HIP events on the launch stream) --------------------- */

#define HIBAG_HIP_K_PACK     0   /* genotype packing + classifier weights        */
#define HIBAG_HIP_K_TOTAL    1   /* pass 1: per-classifier in-order totals       */
#define HIBAG_HIP_K_ACCUM    2   /* pass 2: normalised weighted accumulation     */
#define HIBAG_HIP_K_FINISH   3   /* arg-max, dosage, transposed posterior output */
#define HIBAG_HIP_K_COUNT    4

/* enabled = 1: every kernel class is bracketed by hipEvents on its stream (classes that follow each other directly share
 * the event between them: five records per batch).  enabled = 2 * mask, mask = OR of (1 << HIBAG_HIP_K_*): only those
 * classes (an event record is a packet of its own on the queue and costs the step a few microseconds each: a caller that
 * wants one kernel's duration out of a timed region asks for that kernel alone).  0: off. */
int hibag_hip_set_timing(hibag_hip_model *m, int enabled);
/* Resolves pending events (synchronises on them) and returns, for kernel `k`,
 * the summed duration in ms and the number of launches since the last reset. */
int hibag_hip_get_timing(hibag_hip_model *m, int k, double *ms_total, int64_t *launches);
int hibag_hip_reset_timing(hibag_hip_model *m);

/* The instruction costs the kernels' issue floor is priced with, measured on the calling thread's
 * current device in about 50 ms: ns per wave64 instruction per SIMD with 8 wavefronts on every SIMD, for FP64 mul / add
 * (the one multiplication and one addition per haplotype pair of src/LibHLA.cpp:1786-1813 are the irreducible part of a
 * pass), v_mfma_i32_32x32x32_i8 and v_mfma_scale_f32_32x32x64_f8f6f4 (FP4 operands), and the time of a half / half mix of
 * FP64 and int8-MFMA wavefronts as a fraction of the serial sum (1 = the matrix pipe does not hide behind FP64 work).
 * Any pointer may be NULL.  Measurement only: nothing in the library reads these numbers. */
int hibag_hip_measure_issue_costs(double *fp64_op_ns, double *mfma_i8_ns, double *mfma_fp4_ns, double *mix_frac_of_serial);

/* ---- HIBAG plugin table (per-sample, drop-in for an unmodified HIBAG) ---- */

/* Returns a pointer to a static struct laid out exactly like
 * HLA_LIB::TypeGPUExtProc (inst/include/LibHLA_ext.h:358-388): ten function
 * pointers, all implemented.
 *   predict_init / predict_done / predict_avg_prob  (src/LibHLA.cpp:2498-2531, :2433-2441)
 *   build_init / build_done / build_set_bootstrap    (src/LibHLA.cpp:2256-2266, :2290-2293)
 *   build_haplomatch                                 (src/LibHLA.cpp:1037-1063)
 *   build_set_haplo_geno / build_acc_oob / build_acc_ib (src/LibHLA.cpp:1916-1920, :1938-1941, :1961-1964)
 * An R package hands it to hlaPredict() as attr(cl, "proc_ptr") (R/HIBAG.R:707) or
 * to HIBAG_NewClassifiers as its last argument (src/HIBAG.cpp:601-602); see
 * INTEGRATION.md.  Failures inside these void entries throw `const char *`, which
 * the host's CORE_CATCH turns into an R error (src/HIBAG.cpp:41-60).
 * The predict entries are called once per SAMPLE by the host; they run kernels of their own that
 * take their parallelism from the model instead of a batch (thread = allele-pair cell; no work items
 * are cut, so the launch status above does not apply to them) -- about 0.1 ms per call.
 * The table serves ONE model and ONE training state per process at a time, on the device
 * selected with hibag_hip_set_device by the calling thread: predict_init replaces the model of
 * the previous predict_init, build_init the previous build state -- the same restriction as the
 * reference's single staging buffer (gpu_geno_buf, src/LibHLA.h:680), which is why the host must
 * call with nthread = 1. */
const void *hibag_hip_gpu_ext_proc(void);

/* predict_avg_prob is ONE kernel whose workgroups meet at a barrier, so they must all be resident at once.  On a device the
 * process shares (another stream, another process, a profiler) that cannot be promised: a launch whose workgroups give up
 * waiting (a fifth of a second) is repeated on a single workgroup, which waits for nobody -- same results, slower -- and so
 * are the following calls, with the full width tried again every 64th.  Returns how many calls since the last predict_init
 * took that route in a row (0: the device is the process's own). */
long long hibag_hip_plugin_degraded_calls(void);

/* The loop an unmodified HIBAG runs around predict_avg_prob (src/LibHLA.cpp:2362-2411, :2433-2441), compiled like the host's:
 * n_samp calls through the table -- geno: TGenotype [n_samp][n_classifier] (48 bytes each), weight [n_samp][n_classifier] --
 * each followed by BestGuessEnsemble's scan (:1549-1566).  Returns the elapsed time of the loop in *seconds, the winning
 * posterior cell (-1: none) and the matching value per sample.  predict_init must have been called.  For measurements
 * (bench.py: what the zero-change route costs a compiled host, no interpreter between the calls) and tests. */
int hibag_hip_test_time_avg_prob(const void *geno, const double *weight, int n_samp, int n_classifier, int n_cell,
	int32_t *best_cell, double *matching, double *seconds);

/* One growth step's batched scoring on the caller's own arrays, for tests: what the training driver does per step with its
 * candidates -- build_init(n_hla, n_sample), build_set_bootstrap(boot), the scoring of n_cand candidate lists that extend
 * one genotype list by its SNP n_snp - 1 (1 <= n_snp <= 128), build_done -- and what a sequence of build_set_haplo_geno +
 * build_acc_oob + build_acc_ib calls returns for them (src/LibHLA.cpp:2018-2038).
 *   boot[n_sample]        bootstrap counts, 0 = out-of-bag
 *   base_geno             TGenotype [n_sample] (48 bytes each): the committed SNPs and the true alleles, position n_snp - 1 missing
 *   n_haplo[n_cand], haplo  the candidates' THaplotype lists back to back (32 bytes each), each grouped by ascending
 *                         allele with aux.hla_allele filled (SetHaploAux_GPU, src/LibHLA.cpp:565-578)
 *   columns               [n_cand][n_sample] the raw genotype of each candidate's SNP per sample (outside 0..2 = missing)
 *   geno_snp_major, n_matrix_snp, cand_snp[n_cand]   optional: a SNP-major int32 matrix [n_matrix_snp][n_sample] that is kept
 *                         on the device, and each candidate's row in it; the candidates then travel as row indices and
 *                         `columns` is not read (it may be NULL).  With geno_snp_major NULL the host packs `columns`.
 *   acc_floor             the search's best out-of-bag count so far
 *   acc_oob[n_cand]       out: correct alleles over the out-of-bag samples
 *   loss_ib[n_cand]       out: -2 * in-bag log-likelihood where acc_oob reaches the running maximum that starts at
 *                         acc_floor (:2033-2034), else 0
 * Replaces the calling thread's training state (like build_init); nothing else of the build entries may run on the thread
 * in between.  (Added within ABI version 7.) */
int hibag_hip_test_build_eval_batch(int n_hla, int n_sample, const int *boot, const void *base_geno, int n_snp,
	int n_cand, const int *n_haplo, const void *haplo, const int32_t *columns, const int32_t *geno_snp_major, int n_matrix_snp,
	const int *cand_snp, int acc_floor, int *acc_oob, double *loss_ib);

/* The EM fits of one growth step's candidate SNPs on the device, on the caller's own arrays, for tests: what the training
 * driver does per step in EM mode 2 (CAlg_EM::PrepareNewSNP + ExpectationMaximization per candidate, src/LibHLA.cpp:1127-1255)
 * -- one call of the kernel on the calling thread's selected device, with the transposed pair lists the driver's own builder
 * makes and the LDS layout the driver's own rule picks.
 *   n_ib, n_pair, n_hap   in-bag samples, their haplotype pairs, DOUBLED haplotypes (even: entry 2 i carries allele 0 of the
 *                         new SNP, 2 i + 1 allele 1)
 *   n_samp_total          all samples of the cohort (the M step scales by 0.5 / n_samp_total)
 *   h1, h2 [n_pair]       the pairs, indices into the doubled list; sample i owns pairs [off[i], off[i + 1]); off [n_ib + 1]
 *   boot [n_ib]           bootstrap counts, >= 1
 *   cur_freq [n_hap / 2]  frequencies of the current (undoubled) haplotypes
 *   geno [n_cand][n_ib]   int8: the in-bag samples' genotype at each candidate, 0, 1, 2, or 3 = missing
 *   afreq [n_cand]        each candidate's allele frequency in the bag, strictly inside (0, 1)
 *   out_freq [n_cand][n_hap]   out: the fitted frequencies
 *   status [n_cand]       out: 1 = fitted, bit-identical to the host's fit; 2 = the stopping test was too close to its
 *                         tolerance (or the log-likelihood not finite) for the device's log() to decide it: the host must fit
 *                         this candidate, out_freq[c] is not to be used
 *   iters [n_cand]        out, optional: the 0-based number of the last iteration whose frequencies are returned (the
 *                         reference's loop counter at its `break`); 501 where 500 iterations passed without convergence
 *   layout                out, optional: the LDS layout that ran, as hibag_hip_test_em_layout names it
 * Every size, offset, index, count, genotype and frequency is checked before the device is touched (HIBAG_HIP_EINVAL, also
 * where hibag_hip_test_em_layout() is 0), so no input reaches the kernel that could make it index out of bounds.  Releases
 * the calling thread's EM arena when it returns, also on an error.  (Added within ABI version 7.) */
int hibag_hip_test_em_fit(int n_ib, int n_pair, int n_hap, int n_samp_total, const int *h1, const int *h2, const int *off,
	const int *boot, const double *cur_freq, int n_cand, const int8_t *geno, const double *afreq, double *out_freq, int *status,
	int *iters, int *layout);

/* The LDS layout the device EM fit uses for a growth step of these dimensions -- the rule the driver itself applies, pure
 * arithmetic, no device access: 0 = the step does not fit the kernel (the host fits it), 1 = "staged" (every haplotype's
 * pair values have a contiguous copy the M step reads in order), 2 = "gather" (the M step reads them through offsets). */
int hibag_hip_test_em_layout(int n_ib, int n_pair, int n_hap);

/* Test entries: the layout hibag_hip_model_finalize would upload for the model as it stands -- the planning stages run on
 * the host, with the same environment overrides (HIBAG_PASS2, HIBAG_STORE_PAIRS, HIBAG_PREBUILT_MB), no device is touched
 * and the model stays unfinalized and usable.  The plan is a list of named entries: every array of the layout, the bytes
 * reserved for each ("room:<array>"), and its scalars as arrays of one int64 or double; it does not depend on the model
 * once made.  NULL (a plan the stages reject: their error; a finalized model: HIBAG_HIP_ESTATE) or a plan the caller frees.
 * tests/layout_reference.py interprets it.  (Added within ABI version 7.) */
typedef struct hibag_hip_layout hibag_hip_layout;
hibag_hip_layout *hibag_hip_test_layout_plan(hibag_hip_model *m);
int hibag_hip_test_layout_count(const hibag_hip_layout *plan);
/* entry `index` in [0, count): its name, first byte, size in bytes and bytes per element (each out pointer optional) */
int hibag_hip_test_layout_get(const hibag_hip_layout *plan, int index, const char **name, const void **data, uint64_t *bytes,
	int *elem_size);
void hibag_hip_test_layout_free(hibag_hip_layout *plan);

#ifdef __cplusplus
}
#endif
#endif /* HIBAG_HIP_H_ */
