// hibag_kernels.h -- launchers of the gfx950 kernels (hibag_kernels.hip).
// All launchers enqueue on `st` and return; they never allocate or synchronise.
#ifndef HIBAG_KERNELS_H_
#define HIBAG_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hibag_device.h"
#include "hibag_plan.h"

// d_col / d_flip (optional): the cohort's own matrix with `row_len` SNPs per sample, gathered and flipped on the device
void hibag_launch_pack(const HibagModelView &M, const HibagBatchView &B, const int32_t *d_geno, int row_len,
	const int32_t *d_col, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st);
// the same for a SNP-major matrix: int32 [rows][ld], row d_col[k] (nullptr: k) holds model SNP k
void hibag_launch_pack_rows(const HibagModelView &M, const HibagBatchView &B, const int32_t *d_geno, size_t ld,
	const int32_t *d_col, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st);
// PLINK BED sources: `d_bed` is the payload after the 3-byte prefix, rows of `stride` bytes
void hibag_launch_pack_bed(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_bed, int mode,
	size_t stride, int samp0, const int32_t *d_snp_row, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st);
void hibag_launch_bed_geno(const uint8_t *d_bed, int mode, size_t stride, int n_samp, int n_save,
	const int32_t *d_sel, int32_t *d_geno, hipStream_t st);
// The resident cohort (hibag_k_cohort.h).  _pack: a slab of the host's int32 matrix -- [n_snp][ld] (snp_major, ld a multiple
// of 4, at most 65,535 rows) or [n_samp][ld] with the SNP fastest (at most 65,535 x 64 SNPs) -- into the 2-bit rows that start
// at d_out, `stride` bytes apart, from byte `byte0` of each row on.  _counts: called genotypes and their sum per row.
void hibag_launch_cohort_pack(const int32_t *d_slab, int snp_major, size_t ld, int n_snp, int n_samp, uint8_t *d_out,
	size_t stride, size_t byte0, hipStream_t st);
void hibag_launch_cohort_counts(const uint8_t *d_rows, size_t stride, int n_snp, int32_t *d_n_valid, int64_t *d_sum, hipStream_t st);
// `side`: a second stream and two events of the caller's, for the kernel that runs beside pass 1 where the model has
// FP4 classifiers of several K steps (fork behind what is already on `st`, join before anything that follows)
struct HibagSideStream { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
// vote: the call is a majority vote (vote_method = 2) -- pass 1 logs the records of the cell sums (HibagBatchView::vrec) for
// hibag_launch_vote, stores no cell sums for a second pass and cuts no work items
// (returns what it launched: the plan of hibag_plan.h and the build of k_total -- for hibag_hip_test_last_launch)
HibagLaunchTotal hibag_launch_total(const HibagModelView &M, const HibagBatchView &B, hipStream_t st, const HibagSideStream &side, bool vote = false);
// resident workgroups of k_total<STORE, occupancy> -- [0] <false, 5>, [1] <false, 6>, [2] <true, 5>, [3] <true, 6> -- and of
// k_accum on the current device (0 = unknown)
void hibag_query_slots(int total[4], int *accum);
HibagLaunchAccum hibag_launch_accum(const HibagModelView &M, const HibagBatchView &B, hipStream_t st);
void hibag_launch_vote(const HibagModelView &M, const HibagBatchView &B, int *d_best_cell, hipStream_t st);
void hibag_launch_scalars(const HibagModelView &M, const HibagBatchView &B, const int *d_best_cell, hipStream_t st);
void hibag_launch_finish(const HibagModelView &M, const HibagBatchView &B, double *d_part,
	int32_t *d_H1, int32_t *d_H2, double *d_max_prob, double *d_matching,
	double *d_dosage, double *d_postprob, hipStream_t st);
// The finish of the top-k entries (hibag_k_topk.h), launched INSTEAD of hibag_launch_finish: per sample the k largest
// cells of the normalised ensemble matrix as pairs d_H1 / d_H2 [n_samp][k] with d_prob [n_samp][k], and d_matching [n_samp]
// (may be nullptr); 1 <= k <= HIBAG_TOPK_MAX (= HIBAG_HIP_TOPK_MAX of the public header).
#define HIBAG_TOPK_MAX 16
void hibag_launch_finish_topk(const HibagModelView &M, const HibagBatchView &B, double *d_part, int k,
	int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_matching, hipStream_t st);
// The finish of the draw entries (hibag_k_draw.h), launched INSTEAD of hibag_launch_finish: per sample n_draw pairs drawn
// from the normalised ensemble matrix, d_H1 / d_H2 / d_prob [n_samp][n_draw], and d_matching [n_samp] (may be nullptr);
// 1 <= n_draw <= HIBAG_DRAW_MAX (= HIBAG_HIP_DRAW_MAX of the public header).  Lane 0 of the batch is sample
// `sample_index_of_first_lane` of the caller's numbering: the index the counter-based generator is keyed with.
#define HIBAG_DRAW_MAX 64
void hibag_launch_finish_draw(const HibagModelView &M, const HibagBatchView &B, double *d_part, int n_draw, uint64_t seed,
	int64_t sample_index_of_first_lane, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_matching, hipStream_t st);
// The finish of the group entries (hibag_k_groups.h), launched INSTEAD of hibag_launch_finish: per sample and partition the
// best pair of groups under the collapsed posterior, d_G1 / d_G2 / d_prob [n_samp][n_part], d_matching [n_samp] (may be
// nullptr) and the group dosages d_dosage [n_samp][n_level] (may be nullptr).  The view is a plan's lists on the device
// (hibag_groups.hip builds them): entries are a cell index with the GRP_* marks of hibag_k_groups.h.
struct HibagGroupsView {
	int n_part;                        // Q
	int n_dose;                        // entries per partition of the dosage list (the longest partition's; the others padded)
	int n_level;                       // D: the groups of all partitions
	const uint32_t *call;              // [n_cell][n_part]: the cells by (bin, cell), the last of each bin marked
	const uint32_t *dose;              // [n_dose][n_part]: the cells by (group, cell), marks for "twice", "group ends", "empty group"
	const int32_t *group_of;           // [n_part][n_hla]
	const int32_t *offset;             // [n_part + 1]: where a partition's groups start in a row of d_dosage
};
#define HIBAG_GROUPS_TILE_MAX 64                   // samples per workgroup at most
#define HIBAG_GROUPS_LDS_DOUBLES 8064              // posterior values a workgroup stages in LDS (63 KiB; with the kernel's 1 KiB of per-sample scalars 64 KiB: two workgroups per CU)
// samples per workgroup the launcher takes for a plan of n_part partitions on a model of n_cell cells, and whether their
// posteriors are staged in LDS (*lds = 0: the walk reads the ensemble sums themselves -- n_cell > HIBAG_GROUPS_LDS_DOUBLES, or
// HIBAG_GROUPS_NO_LDS=1 in the environment, read at every call)
int hibag_groups_tile(int n_cell, int n_part, int *lds);
void hibag_launch_finish_groups(const HibagModelView &M, const HibagBatchView &B, double *d_part, const HibagGroupsView &V,
	int32_t *d_G1, int32_t *d_G2, double *d_prob, double *d_matching, double *d_dosage, hipStream_t st);
// The finish of the given entries (hibag_k_given.h), launched INSTEAD of hibag_launch_finish: per sample the best allele pair
// among the cells consistent with the sample's two allele sets, d_H1 / d_H2 / d_prob (joint) / d_support [n_samp], d_matching
// [n_samp] (may be nullptr) and the restricted dosages d_dosage [n_samp][n_hla] (may be nullptr).  d_allow: the batch's sets,
// uint32 [n_samp][2][W] with W = (n_hla + 31) / 32, on the device; d_masks: 2 W n_pad words of workspace.
void hibag_launch_finish_given(const HibagModelView &M, const HibagBatchView &B, double *d_part, const uint32_t *d_allow,
	uint32_t *d_masks, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_support, double *d_matching, double *d_dosage,
	hipStream_t st);
// The finish of the family entries (hibag_k_family.h), launched INSTEAD of hibag_launch_finish: per sample the best allele
// pair under its posterior weighted by its parents' results, d_H1 / d_H2 / d_prob (joint) / d_support [n_samp], d_matching
// [n_samp] (may be nullptr) and the weighted dosages d_dosage [n_samp][n_hla] (may be nullptr).  The call-wide state on the
// device: the pedigree, the depths and the prior as the entry uploaded them, and every finished sample's (D, S).
struct HibagFamilyView {
	const int32_t *ped = nullptr;      // [n_call][2]: (father, mother) in the call's numbering, -1 = not in this call
	const int32_t *depth = nullptr;    // [n_call]: generations above the sample within the call
	const double *prior = nullptr;     // [n_hla], or nullptr (all 1.0)
	double *fam_D = nullptr;           // [n_call][n_hla]: the finished samples' joint dosages
	double *fam_S = nullptr;           // [n_call]: ... and supports
	double *ratios = nullptr;          // workspace of one batch: [2 n_hla][n_pad]
	size_t call0 = 0;                  // the call's index of the batch's sample 0
};
// rounds[n_rounds]: the distinct depths among the batch's samples, ascending (one round of three launches each)
void hibag_launch_finish_family(const HibagModelView &M, const HibagBatchView &B, double *d_part, const HibagFamilyView &F,
	const int *rounds, int n_rounds, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_support, double *d_matching,
	double *d_dosage, hipStream_t st);
// hlaOutOfBag (hibag_k_oob.h): each classifier predicts its own out-of-bag samples.  The per-classifier arrays are
// [C][ld] with the batch's sample 0 at column 0 (the caller offsets the pointers); the plain haplotype table (grouped by
// allele, hla_start[c][n_hla + 1] relative to hap_off[c]) serves the rare lane whose record log cannot settle its call.
struct HibagOobOut {
	const int32_t *samp_num;           // bootstrap counts: 0 = out of bag
	int32_t *h1, *h2;                  // 0-based alleles or NA_integer_
	double *prob;
	size_t ld;
	const uint64_t *hap_bits;          // [H][2]
	const double *hap_freq;            // [H]
	const int *hap_off;                // [C]
	const int *hla_start;              // [C][n_hla + 1]
};
// after a pack of the batch: the one-classifier weights, pass 1 with its record log, the picks -- no second pass, no finish
void hibag_launch_oob(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_codes, const HibagOobOut &O,
	int force_rescan, const HibagSideStream &side, hipStream_t st);
// The per-sample classifier mask of hibag_hip_predict_masked (hibag_k_mask.h).  `use` is [C][ld] bytes with the batch's
// sample 0 at column 0 (the caller offsets the pointer); the users of a SNP are the classifiers that hold it, in model order.
struct HibagMaskView {
	const uint8_t *use;                // != 0: the classifier takes part for the sample
	size_t ld;
	const int *user_off;               // [n_snp + 1]
	const int *user_cls;               // [user_off[n_snp]]
	int32_t *cnt;                      // [n_snp][n_pad] workspace: the sample's sub-model's classifiers per SNP
};
// after a pack of the batch, before pass 1: the sub-models' SNP counts, then their classifier weights into B.cw / B.winv
void hibag_launch_mask_weights(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_codes, const HibagMaskView &K,
	hipStream_t st);
// The out-of-bag SNP knock-out of hibag_hip_oob_knock (hibag_k_knock.h).  The call's table of virtual
// 64-lane groups -- (snp, block): samples 64 block .. 64 block + 63 of the cohort with SNP `snp` set to missing, snp = -1
// for a base group -- and what its three kernels read and write; a batch is groups g0 .. g0 + B.n_pad / 64 of the table.
struct HibagKnockView {
	const int2 *group;                 // [groups of the call]
	int g0;                            // the batch's first group
	int n_cohort, n_pad0;              // the cohort's samples, and their number rounded up to 64
	const uint8_t *base;               // [n_snp][n_pad0]: the cohort's byte codes (k_codes)
	const int32_t *samp_num;           // [C][n_cohort] bootstrap counts: 0 = out of bag
	const int32_t *truth;              // [n_cohort][2]: the true pair as indices of the model's alleles, NA_integer_ = not counted
	const int *user_off;               // [n_snp + 1]: the users of a SNP in model order ...
	const int *user_cls;               // ... their classifiers ...
	const int *user_var;               // ... and the variant snp_off[c] + j of each
	int32_t *base_h1, *base_h2;        // [C][n_pad0]: the base groups' calls, kept for the call
	long long *tally;                  // [n_variant + C][5]: n_ind, n_call, crt_ind, crt_haplo, n_changed; base rows last
	int n_variant;
	int use_threshold;                 // 0: every call counts
	double threshold;
	int32_t *H1, *H2;                  // optional (both or none) [n_variant + C][n_cohort]
	double *prob;                      // optional, the same shape
};
// the cohort's codes, once per call: k_codes over all of d_geno [n_samp][n_snp] into d_base [n_snp][round_up(n_samp, 64)]
void hibag_launch_knock_base(const HibagModelView &M, const int32_t *d_geno, int n_samp, uint8_t *d_base, hipStream_t st);
// one batch of virtual groups (B from make_batch(m, 64 * groups, true, B)): the virtual codes, k_pack, the weights, pass 1
// with its record log and the picks of hibag_launch_oob into O ([C][B.n_pad], O.ld = B.n_pad), the tallies -- the batch's
// first `n_base` groups are base groups
void hibag_launch_knock(const HibagModelView &M, const HibagBatchView &B, const HibagKnockView &K, uint8_t *d_codes,
	const HibagOobOut &O, int n_base, int force_rescan, const HibagSideStream &side, hipStream_t st);

#endif
