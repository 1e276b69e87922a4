// hibag_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4) for HIBAG's
// attribute-bagging prediction hot path: the haplotype-pair posterior loop of
// CAlg_Prediction::_PostProb2 (src/LibHLA.cpp:1769-1830) and the ensemble step
// of CAttrBag_Model::_PredictHLA / PredictHLA (src/LibHLA.cpp:2317-2482).
//
// Mapping: LANE = SAMPLE.  A wavefront holds 64 samples and walks the model's
// loop nest (classifier -> allele pair -> haplotype pair) in the reference's
// order.  The nest depends only on the model, so control flow is wave-uniform, and each lane reproduces the
// reference's rounding sequence for its own sample: results are bit-identical
// to the CPU kernels by construction, with no cross-lane reduction anywhere on
// the numeric path.
//
// Two engines compute the distance d of a pair (bit-identical results):
//   matrix engine 8 d = A . B over 2k+1 positions (h1+h2 against the genotype's signs, h1&h2 -- on the FP4 path a stand-in
//                 for it that is a plain sum of two images -- against [g = 1], an offset term): a small GEMM of 32 records
//                 x 64 samples per block --
//                 up to 30 SNPs on the FP4 matrix path (v_mfma_scale_f32_32x32x64_f8f6f4, e2m1 operands: all 64 K
//                 positions in one instruction per sample half; block scales of 2^-73 make the f32 result the
//                 denormal 8 d * 2^-149, whose bit pattern IS the integer 8 d), 31..32 SNPs on
//                 v_mfma_i32_32x32x32_i8 (two K blocks) -- plus 16 v_permlane32_swap to give every lane its own
//                 sample's column.  The records are generated: each lane gathers its pair's two haplotype
//                 images (nibbles / bytes) from an O(H) table through a 4-byte index pair; what is the same for all lanes
//                 -- the pair's frequency factor, the block's end-of-cell masks -- comes through the scalar cache into
//                 scalar registers.  33..112 SNPs: FP4 again, 28 SNPs per K step, chained through the accumulator.  All real classifiers; the default.
//   VALU engine   d = sum_w popc((W[w] ^ T'[w]) & M'[w]): v_bitop3_b32 + v_bcnt_u32_b32 per 32-bit
//                 word of the stored 3k-bit pair string (W uniform in SGPRs, T'/M' the lane's genotype
//                 masks); classifiers with more than 112 SNPs.  (The per-sample plugin route has kernels of its own:
//                 hibag_sample.hip.)
// In both, what the contract fixes stays on the vector ALU, per lane and in the reference's order:
//     cell += prod * TAB[d]          ds_read_b64 (table in LDS), v_mul_f64 (prod a scalar-register operand), v_add_f64
//
// The normalisation 1/sum of a classifier's posterior needs all of its cells,
// and 64 samples x P cells do not fit on chip, so the pair loop runs twice:
// pass 1 (k_total) produces the in-order total per (sample, classifier) and stores the sums of the cells with many
// pairs, pass 2 (k_accum) evaluates the other cells again (or reads the stored sums back), scales each cell and adds it to
// the ensemble sum of its tile of cells, held in LDS (DESIGN.md "Why two passes").
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no FMA fusion: the
// reference multiplies and adds with separate roundings).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "hibag_device.h"
#include "hibag_kernels.h"

#define NA_INTEGER (-2147483647 - 1)
#define CH HIBAG_CHUNK
#define BLOCK_WAVES HIBAG_BLOCK_WAVES         // wavefronts per workgroup (each on its own work item; hibag_device.h)
#define BLOCK_THREADS (BLOCK_WAVES * HIBAG_WAVE)
#ifndef TOTAL_G
#define TOTAL_G 8                           // records of pass 1 whose look-ups are in flight together (and whose factors arrive in one scalar load)
#endif
// Workgroups per CU pass 1 is compiled for, twice: 5 (96 VGPRs: every engine) and 6 (80 VGPRs: the one-step FP4 block loop
// fits, the int8 and VALU-engine loops would spill, so that build carries the FP4 loop alone and serves models whose work
// items are all one-step FP4 classifiers -- k_total's FP4ONLY; no kernel of the path has a private segment).  Six wavefronts per SIMD are 1.5 - 4 % faster once a pass is two rounds of resident
// workgroups or more (10,000 samples of the HLA-B shape: 0.80 -> 0.775 ms; 8,192 of DRB1: 14.1 -> 13.6 ms), and slower below that,
// where a pass lasts as long as its longest work item, which six wavefronts sharing a SIMD stretch (4,096 samples of DRB1:
// 7.1 -> 7.9 ms): the launcher chooses by the number of work items (hibag_launch_total).  (4 -> 128 VGPRs: measured slower.)
#ifndef HIBAG_TOT_OCC
#define HIBAG_TOT_OCC 5
#endif
#ifndef HIBAG_TOT_OCC_MANY
#define HIBAG_TOT_OCC_MANY 6
#endif
#ifndef ACCUM_AHEAD
#define ACCUM_AHEAD true                    // pass 2: the next group's table look-ups requested before this group is added up (-0.6 %, six registers; false: the wait right behind the look-ups)
#endif
#ifndef ACCUM_G
#define ACCUM_G 4                           // the same for pass 2
#endif
#define ACCUM_TAB_N 64                      // table entries pass 2 stages: it evaluates one-step FP4 classifiers only
static_assert(2 * HIBAG_FP4_MAX_SNPS + 1 <= ACCUM_TAB_N, "pass 2's table must cover every distance of a one-step FP4 classifier");
#define ACCUM_WAVES HIBAG_ACCUM_WAVES         // wavefronts per workgroup of pass 2 (sample groups that share a tile's blocks in L1)

// The device code, in the order of a step (each file says what it holds):
#include "hibag_k_engine.h"
#include "hibag_k_pack.h"
#include "hibag_k_pass1.h"
#include "hibag_k_pass2.h"
#include "hibag_k_vote.h"
#include "hibag_k_finish.h"
#include "hibag_k_topk.h"
#include "hibag_k_draw.h"
#include "hibag_k_groups.h"
#include "hibag_k_given.h"
#include "hibag_k_family.h"
#include "hibag_k_oob.h"
#include "hibag_k_mask.h"
#include "hibag_k_knock.h"
#include "hibag_k_cohort.h"

// ---------------------------------------------------------------------------
// launchers (host side, no synchronisation, no allocation)

static inline dim3 grid1(int n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

void hibag_launch_pack(const HibagModelView &M, const HibagBatchView &B, const int32_t *d_geno, int row_len,
	const int32_t *d_col, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0) return;
	hipLaunchKernelGGL(k_codes, dim3(B.n_pad / 64, (M.n_snp + 63) / 64), dim3(256), 0, st, M, B, d_geno,
		d_col ? row_len : M.n_snp, d_col, d_flip, d_codes);
	hipLaunchKernelGGL(k_pack, dim3(B.n_pad / HIBAG_WAVE, (M.n_classifier + PACK_WAVES - 1) / PACK_WAVES), dim3(PACK_WAVES * HIBAG_WAVE), 0, st, M, B,
		(const uint8_t *)d_codes);
}

// the genotypes as a SNP-major matrix int32 [rows][ld] (k_codes_rows)
void hibag_launch_pack_rows(const HibagModelView &M, const HibagBatchView &B, const int32_t *d_geno, size_t ld,
	const int32_t *d_col, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0) return;
	hipLaunchKernelGGL(k_codes_rows, dim3((B.n_pad + 255) / 256, M.n_snp), dim3(256), 0, st, M, B, d_geno, ld, d_col, d_flip, d_codes);
	hipLaunchKernelGGL(k_pack, dim3(B.n_pad / HIBAG_WAVE, (M.n_classifier + PACK_WAVES - 1) / PACK_WAVES), dim3(PACK_WAVES * HIBAG_WAVE), 0, st, M, B,
		(const uint8_t *)d_codes);
}

void hibag_launch_pack_bed(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_bed, int mode,
	size_t stride, int samp0, const int32_t *d_snp_row, const int32_t *d_flip, uint8_t *d_codes, hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0) return;
	hipLaunchKernelGGL(k_bed_codes, dim3(B.n_pad / 64, (M.n_snp + 3) / 4), dim3(256), 0, st, M, B, d_bed, mode, stride,
		samp0, d_snp_row, d_flip, d_codes);
	hipLaunchKernelGGL(k_pack, dim3(B.n_pad / HIBAG_WAVE, (M.n_classifier + PACK_WAVES - 1) / PACK_WAVES), dim3(PACK_WAVES * HIBAG_WAVE), 0, st, M, B,
		(const uint8_t *)d_codes);
}

void hibag_launch_bed_geno(const uint8_t *d_bed, int mode, size_t stride, int n_samp, int n_save,
	const int32_t *d_sel, int32_t *d_geno, hipStream_t st)
{
	if (n_samp <= 0 || n_save <= 0) return;
	hipLaunchKernelGGL(k_bed_geno, dim3((n_samp + 63) / 64, (n_save + 63) / 64), dim3(256), 0, st, d_bed, mode, stride,
		n_samp, n_save, d_sel, d_geno);
}

// the resident cohort (hibag_k_cohort.h): one slab of the host matrix into the 2-bit rows; the per-row counts
void hibag_launch_cohort_pack(const int32_t *d_slab, int snp_major, size_t ld, int n_snp, int n_samp, uint8_t *d_out,
	size_t stride, size_t byte0, hipStream_t st)
{
	if (n_snp <= 0 || n_samp <= 0) return;
	if (snp_major)
		hipLaunchKernelGGL(k_cohort_pack<true>, dim3(((n_samp + 3) / 4 + 255) / 256, n_snp), dim3(256), 0, st, d_slab, ld, n_snp,
			n_samp, d_out, stride, byte0);
	else
		hipLaunchKernelGGL(k_cohort_pack<false>, dim3((n_samp + COHORT_TILE_SAMP - 1) / COHORT_TILE_SAMP,
			(n_snp + COHORT_TILE_SNP - 1) / COHORT_TILE_SNP), dim3(256), 0, st, d_slab, ld, n_snp, n_samp, d_out, stride, byte0);
}

void hibag_launch_cohort_counts(const uint8_t *d_rows, size_t stride, int n_snp, int32_t *d_n_valid, int64_t *d_sum, hipStream_t st)
{
	if (n_snp <= 0) return;
	hipLaunchKernelGGL(k_cohort_counts, dim3((n_snp + 3) / 4), dim3(256), 0, st, d_rows, stride, n_snp, d_n_valid, d_sum);
}

// resident workgroups of a kernel on the current device (0 = unknown)
template <class F>
static int resident_blocks(F kernel, int threads)
{
	int per_cu = 0, cus = 0, dev = 0;
	(void)hipGetDevice(&dev);
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess) return 0;
	return per_cu > 0 && cus > 0 ? per_cu * cus : 0;
}

// chunks per item of the last rounds of passes 1 and 2 ("hand-overs"; HIBAG_TAIL_K=1: undivided items only).
// A hand-over costs about as much as a tenth of a block list of the benchmark model, so 4 chunks there (2 and 8 measure 1-3 %
// worse); items of several thousand blocks (the DRB1 shape: 3,900) take 8 - 16 (-4 % against 4): one chunk per
// `blocks_per_item` / 256, between 4 and 12.
// `forced` = HibagBatchView::tail_k: 1 after a failed hand-over on the model (its launches then have no hand-overs at all).
// (Pass 2, whose items are a tile's ~85 short blocks: 2 chunks -- 0.522-0.527 ms against 0.532 with 4, same box, three runs each.)
static int tail_chunks(int forced, long long blocks_per_item = 0, int at_least = 4)
{
	if (forced > 0) return forced;
	static const int k = getenv("HIBAG_TAIL_K") ? std::max(1, std::min(64, atoi(getenv("HIBAG_TAIL_K")))) : 0;
	return k ? k : (int)std::max<long long>(at_least, std::min(12ll, blocks_per_item / 256));
}

// Resident workgroups of the chunked kernels on the current device; the model keeps them (HibagModelView::slots_*), so
// that models on different devices, and the two instantiations of k_total, each get their own figure.
void hibag_query_slots(int total[4], int *accum)
{
	// [STORE][many]: k_total<false, 5>, <false, 6>, <true, 5>, <true, 6>
	total[0] = resident_blocks(k_total<false, HIBAG_TOT_OCC, 0>, BLOCK_THREADS);
	total[1] = resident_blocks(k_total<false, HIBAG_TOT_OCC_MANY, 2>, BLOCK_THREADS);
	total[2] = resident_blocks(k_total<true, HIBAG_TOT_OCC, 0>, BLOCK_THREADS);
	total[3] = resident_blocks(k_total<true, HIBAG_TOT_OCC_MANY, 2>, BLOCK_THREADS);
	*accum = resident_blocks(k_accum, ACCUM_WAVES * HIBAG_WAVE);
}

HibagLaunchTotal hibag_launch_total(const HibagModelView &M, const HibagBatchView &B, hipStream_t st, const HibagSideStream &side, bool vote)
{
	HibagLaunchTotal R;
	if (M.n_classifier == 0) return R;
	const bool wide = M.n_wide > 0;
	if (wide) {
		// the classifiers of several K steps: their own kernel, beside k_total (more registers than k_total's hot loop may have)
		const unsigned gq = (unsigned)((B.n_pad / HIBAG_WAVE + BLOCK_WAVES - 1) / BLOCK_WAVES);
		HibagModelView W = M;                         // k_total_scan over the classifiers of several K steps that were cut into segments
		W.split_cls = M.wide_scan;
		const hipStream_t ws = side.stream ? side.stream : st;
		if (side.stream) {
			(void)hipEventRecord(side.fork, st);
			(void)hipStreamWaitEvent(side.stream, side.fork, 0);
		}
		// (a classifier of several K steps without haplotypes has no segment: its total still has to be written)
		// (segments are either all whole classifiers or none: hibag_model.hip finalize_model)
		if (M.n_wide_seg > 0 && M.n_wide_scan < M.n_wide) hipLaunchKernelGGL(k_total_wide<true>, dim3(gq, M.n_wide_seg), dim3(BLOCK_THREADS), 0, ws, M, B);
		else if (M.n_wide_seg > 0) hipLaunchKernelGGL(k_total_wide<false>, dim3(gq, M.n_wide_seg), dim3(BLOCK_THREADS), 0, ws, M, B);
		if (M.n_wide_scan > 0) hipLaunchKernelGGL(k_total_scan, dim3(B.n_pad / 64, M.n_wide_scan), dim3(64), 0, ws, W, B);
		if (side.stream) (void)hipEventRecord(side.join, side.stream);
	}
	if (M.n_item_whole == 0) {                        // (every classifier is one of those)
		if (wide && side.stream) (void)hipStreamWaitEvent(st, side.join, 0);
		return R;
	}
	const unsigned gx = (unsigned)((B.n_pad / HIBAG_WAVE + BLOCK_WAVES - 1) / BLOCK_WAVES);
	// A classifier far heavier than the rest (VALU engine, > 112 SNPs) is only worth cutting up when its
	// single-wavefront walk would outlast the rest of the pass, i.e. for small batches.
	HibagModelView V = M;
	const double groups = (double)(B.n_pad / HIBAG_WAVE);
	// (the heavy walk starts with the pass, so it only matters once it lasts about as long as everything else)
	const bool split = M.n_split > 0 && 1.25 * M.split_heavy_ns > M.split_rest_ns * groups / 4096.0;
	V.item = split ? M.item_split : M.item_whole;
	V.n_item = split ? M.n_item_split : M.n_item_whole;
	if (!split) V.n_split = 0;
	// which items go whole, which in chunks, and the build: hibag_plan_total (hibag_plan.h)
	const int sbase = (M.store_cells && !vote) ? 2 : 0;       // (the vote's build stores no cell sums: the occupancy figures of the non-storing one)
	const HibagPlanTotal P = hibag_plan_total(gx, (unsigned)V.n_item, M.slots_total[sbase], M.slots_total[sbase + 1],
		tail_chunks(B.tail_k, M.p1_blocks / std::max(M.n_classifier, 1)), vote, M.all_fp4 != 0, split);
	const bool many = P.many != 0;
	const dim3 grid(P.grid);
	// the build: storing (models whose pass 2 reads cell sums back) / plain / voting (no second pass: nothing stored, records
	// logged) x the walk -- every engine at five workgroups per CU, or one of the two FP4-only builds at six
#define LAUNCH_TOTAL(STORE, OCC, WALK, VOTE) hipLaunchKernelGGL((k_total<STORE, OCC, WALK, VOTE>), grid, dim3(BLOCK_THREADS), 0, st, V, B, (int)gx, (int)P.n_whole, (int)P.rest, (int)P.stride, (int)P.K)
#define LAUNCH_WALK(STORE, VOTE) do { if (!many) LAUNCH_TOTAL(STORE, HIBAG_TOT_OCC, 0, VOTE);                                 \
		else if (M.p1_prebuilt) LAUNCH_TOTAL(STORE, HIBAG_TOT_OCC_MANY, 2, VOTE); else LAUNCH_TOTAL(STORE, HIBAG_TOT_OCC_MANY, 1, VOTE); } while (0)
	if (vote) LAUNCH_WALK(false, true);
	else if (M.store_cells) LAUNCH_WALK(true, false);
	else LAUNCH_WALK(false, false);
#undef LAUNCH_WALK
#undef LAUNCH_TOTAL
	if (split)
		hipLaunchKernelGGL(k_total_scan, dim3(B.n_pad / 64, V.n_split), dim3(64), 0, st, V, B);
	if (wide && side.stream) (void)hipStreamWaitEvent(st, side.join, 0);
	R.plan = P;
	R.launched = 1;
	R.walk = !many ? 0 : M.p1_prebuilt ? 2 : 1;
	R.store = !vote && M.store_cells;
	R.vote = vote;
	return R;
}

HibagLaunchAccum hibag_launch_accum(const HibagModelView &M, const HibagBatchView &B, hipStream_t st)
{
	HibagLaunchAccum R;
	if (M.store_cells == 1 && M.n_classifier > 0) {    // pass 1 stored every cell: read them back
		const unsigned groups_x = (unsigned)((B.n_pad / HIBAG_WAVE + 7) / 8), tq = (unsigned)((M.n_tile + CELLS_WAVES - 1) / CELLS_WAVES);
		hipLaunchKernelGGL(k_accum_cells, dim3(8 * groups_x * tq), dim3(CELLS_WAVES * HIBAG_WAVE), 0, st, M, B);
		R.kernel = 2;
		return R;
	}
	const unsigned n_group = (unsigned)(B.n_pad / HIBAG_WAVE);
	const unsigned n = 8u * (((n_group + 7) / 8 + ACCUM_WAVES - 1) / ACCUM_WAVES) * (unsigned)M.n_tile;   // work items, see k_accum
	if (n == 0 || M.n_classifier == 0) {
		// no classifier: the ensemble sums are all zero (src/LibHLA.cpp:1491-1495)
		(void)hipMemsetAsync(B.part, 0, (size_t)M.n_cell * B.n_pad * sizeof(double), st);
		return R;
	}
	// which items go whole and which in chunks: hibag_plan_accum (hibag_plan.h)
	const HibagPlanAccum P = hibag_plan_accum(n / 8, M.slots_accum, tail_chunks(B.tail_k, 0, 2));
	hipLaunchKernelGGL(k_accum, dim3(P.grid), dim3(ACCUM_WAVES * HIBAG_WAVE), 0, st, M, B, (int)P.n_whole, (int)P.K);
	R.plan = P;
	R.kernel = 1;
	return R;
}

void hibag_launch_vote(const HibagModelView &M, const HibagBatchView &B, int *d_best_cell, hipStream_t st)
{
	if (M.n_classifier > 0) {
		// pass 1 (hibag_launch_total with vote = true) has logged the records of every one-step matrix-engine classifier
		hipLaunchKernelGGL(k_vote_pick, dim3(B.n_pad / 64, M.n_classifier), dim3(64), 0, st, M, B, d_best_cell);
		if (M.n_wide > 0) hipLaunchKernelGGL(k_vote_scan, dim3(B.n_pad / 64, M.n_wide), dim3(64), 0, st, M, B, d_best_cell);
		if (M.n_valu > 0) {
			const unsigned gx = (unsigned)((B.n_pad / HIBAG_WAVE + BLOCK_WAVES - 1) / BLOCK_WAVES);
			hipLaunchKernelGGL(k_vote_best_valu, dim3(gx, M.n_classifier), dim3(BLOCK_THREADS), 0, st, M, B, d_best_cell);
		}
	}
	hipLaunchKernelGGL(k_vote_tally, grid1(B.n_pad, 64), dim3(64), 0, st, M, B, (const int *)d_best_cell);
}

void hibag_launch_scalars(const HibagModelView &M, const HibagBatchView &B, const int *d_best_cell, hipStream_t st)
{
	if (!d_best_cell && M.store_cells != 1 && M.n_classifier > 0 && M.n_tile > 0) {
		// pass 2 was k_accum: its tile-0 workgroups have written the scalars; what is left is the rare NaN work and the mark
		// of a failed hand-over
		hipLaunchKernelGGL(k_nan_cells, dim3((unsigned)std::max(M.n_tile, B.n_pad / 64)), dim3(64), 0, st, M, B);
		return;
	}
	hipLaunchKernelGGL(k_scalars, grid1(B.n_pad, 64), dim3(64), 0, st, M, B, d_best_cell);
}

void hibag_launch_finish(const HibagModelView &M, const HibagBatchView &B, double *d_part,
	int32_t *d_H1, int32_t *d_H2, double *d_max_prob, double *d_matching,
	double *d_dosage, double *d_postprob, hipStream_t st)
{
	// (One read of the ensemble sums instead of three -- call and dosage from LDS chunks of 128 cells, 32 samples x 32 threads per
	// workgroup -- was built and measured in round 5: 76 us against 47.  The three-read kernel has 785 workgroups of independent
	// loads and runs at 6.5 TB/s; the one-read one has 314 workgroups with a barrier per chunk.  profiles/r05_pass2_notes.txt item 9.)
	if (d_dosage) {
		const unsigned n_group = (unsigned)(B.n_pad / 64);
		hipLaunchKernelGGL(k_finish, dim3(n_group * (1u + (unsigned)((M.n_hla + FIN_SEG - 1) / FIN_SEG))), dim3(64 * FIN_SEG), 0, st,
			M, B, (const double *)d_part, d_H1, d_H2, d_max_prob, d_matching, d_dosage);
	} else {
		hipLaunchKernelGGL(k_finish_call, dim3(B.n_pad / 64), dim3(64 * FIN_SEG), 0, st, M, B, (const double *)d_part,
			d_H1, d_H2, d_max_prob, d_matching);
	}
	if (d_postprob)
		hipLaunchKernelGGL(k_finish_prob, dim3(B.n_pad / 64, (M.n_cell + 63) / 64), dim3(256), 0, st,
			M, B, (const double *)d_part, d_postprob);
}

// the finish of the top-k entries, in place of hibag_launch_finish: the smallest list bound that holds k (hibag_k_topk.h)
void hibag_launch_finish_topk(const HibagModelView &M, const HibagBatchView &B, double *d_part, int k,
	int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_matching, hipStream_t st)
{
	static_assert(HIBAG_TOPK_MAX == 16, "one instantiation of k_finish_topk per list bound up to HIBAG_TOPK_MAX");
	if (k < 1 || k > HIBAG_TOPK_MAX) return;            // (the entries have checked k)
#define LAUNCH_TOPK(KMAX) hipLaunchKernelGGL(k_finish_topk<KMAX>, dim3(B.n_pad / 64), dim3(64 * (64 / KMAX)), 0, st, M, B, \
		(const double *)d_part, k, d_H1, d_H2, d_prob, d_matching)
	if (k <= 4) LAUNCH_TOPK(4);
	else if (k <= 8) LAUNCH_TOPK(8);
	else LAUNCH_TOPK(16);
#undef LAUNCH_TOPK
}

// the finish of the draw entries, in place of hibag_launch_finish: the fewest wavefronts per workgroup that hold n_draw (hibag_k_draw.h)
void hibag_launch_finish_draw(const HibagModelView &M, const HibagBatchView &B, double *d_part, int n_draw, uint64_t seed,
	int64_t sample_index_of_first_lane, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_matching, hipStream_t st)
{
	static_assert(HIBAG_DRAW_MAX == 4 * DRAW_PER_WAVE, "one instantiation of k_finish_draw per wavefront count up to HIBAG_DRAW_MAX / DRAW_PER_WAVE");
	if (n_draw < 1 || n_draw > HIBAG_DRAW_MAX) return;  // (the entries have checked n_draw)
#define LAUNCH_DRAW(NW) hipLaunchKernelGGL(k_finish_draw<NW>, dim3(B.n_pad / 64), dim3(64 * NW), 0, st, M, B, \
		(const double *)d_part, n_draw, seed, sample_index_of_first_lane, d_H1, d_H2, d_prob, d_matching)
	if (n_draw <= DRAW_PER_WAVE) LAUNCH_DRAW(1);
	else if (n_draw <= 2 * DRAW_PER_WAVE) LAUNCH_DRAW(2);
	else LAUNCH_DRAW(4);
#undef LAUNCH_DRAW
}

// the finish of the group entries, in place of hibag_launch_finish (hibag_k_groups.h).  A workgroup takes `tile` samples: as many
// as give each of its 256 threads at most ONE (sample, partition) pair (one sample for more than 256 partitions: several
// rounds), at most what fits in LDS.  Small tiles on purpose: a walk is a chain of dependent loads, so what counts is the
// number of wavefronts in flight, and a workgroup's LDS is what bounds them (HLA-B shape, 100 partitions: 2 samples, 20 KB).
int hibag_groups_tile(int n_cell, int n_part, int *lds)
{
	const char *e = getenv("HIBAG_GROUPS_NO_LDS");
	const int fit = HIBAG_GROUPS_LDS_DOUBLES / std::max(n_cell, 1);
	const bool use_lds = fit >= 1 && !(e && atoi(e) != 0);
	int tile = std::min(HIBAG_GROUPS_TILE_MAX, GROUPS_THREADS / std::max(n_part, 1));
	if (use_lds) tile = std::min(tile, fit);
	if (lds) *lds = use_lds ? 1 : 0;
	return std::max(tile, 1);
}

void hibag_launch_finish_groups(const HibagModelView &M, const HibagBatchView &B, double *d_part, const HibagGroupsView &V,
	int32_t *d_G1, int32_t *d_G2, double *d_prob, double *d_matching, double *d_dosage, hipStream_t st)
{
	if (V.n_part < 1 || B.n_samp < 1) return;           // (the entries have checked the plan)
	int lds = 0;
	const int tile = hibag_groups_tile(M.n_cell, V.n_part, &lds);
	const dim3 grid((unsigned)((B.n_samp + tile - 1) / tile));
	if (lds)
		hipLaunchKernelGGL(k_finish_groups<true>, grid, dim3(GROUPS_THREADS), (size_t)tile * M.n_cell * sizeof(double), st, M, B,
			(const double *)d_part, V, tile, d_G1, d_G2, d_prob, d_matching, d_dosage);
	else
		hipLaunchKernelGGL(k_finish_groups<false>, grid, dim3(GROUPS_THREADS), 0, st, M, B,
			(const double *)d_part, V, tile, d_G1, d_G2, d_prob, d_matching, d_dosage);
}

// the finish of the given entries, in place of hibag_launch_finish (hibag_k_given.h): the batch's constraint transposed into
// d_masks ([2 W][n_pad] words of the caller's workspace), the walk, and -- if asked for -- the dosage as a second launch
void hibag_launch_finish_given(const HibagModelView &M, const HibagBatchView &B, double *d_part, const uint32_t *d_allow,
	uint32_t *d_masks, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_support, double *d_matching, double *d_dosage,
	hipStream_t st)
{
	if (B.n_samp < 1 || M.n_hla < 1) return;
	const int W = (M.n_hla + 31) / 32;
	const size_t words = (size_t)2 * W * (size_t)B.n_pad;
	hipLaunchKernelGGL(k_given_masks, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, d_allow, B.n_samp, B.n_pad, 2 * W, d_masks);
	hipLaunchKernelGGL(k_finish_given, dim3(B.n_pad / 64), dim3(64), 0, st, M, B, (const double *)d_part,
		(const uint32_t *)d_masks, W, d_H1, d_H2, d_prob, d_support, d_matching);
	if (d_dosage)
		hipLaunchKernelGGL(k_given_dosage, dim3(B.n_pad / 64, (M.n_hla + FIN_SEG - 1) / FIN_SEG), dim3(64 * FIN_SEG), 0, st, M, B,
			(const double *)d_part, (const uint32_t *)d_masks, W, d_dosage);
}

// the finish of the family entries, in place of hibag_launch_finish (hibag_k_family.h): per depth present in the batch,
// ascending, the ratio vectors of that depth's samples from their parents' finished (D, S), the walk, and the dosage --
// always: it is what the samples' children read, into the caller's array too if that is asked for
void hibag_launch_finish_family(const HibagModelView &M, const HibagBatchView &B, double *d_part, const HibagFamilyView &F,
	const int *rounds, int n_rounds, int32_t *d_H1, int32_t *d_H2, double *d_prob, double *d_support, double *d_matching,
	double *d_dosage, hipStream_t st)
{
	if (B.n_samp < 1 || M.n_hla < 1) return;
	const size_t n_ratio = (size_t)2 * (size_t)M.n_hla * (size_t)B.n_pad;
	const int32_t *ped = F.ped + 2 * F.call0, *depth = F.depth + F.call0;
	double *fam_D = F.fam_D + F.call0 * (size_t)M.n_hla, *fam_S = F.fam_S + F.call0;
	for (int r = 0; r < n_rounds; r++) {
		hipLaunchKernelGGL(k_family_ratios, dim3((unsigned)((n_ratio + 255) / 256)), dim3(256), 0, st, (const double *)F.fam_D,
			(const double *)F.fam_S, ped, depth, F.prior, B.n_samp, B.n_pad, M.n_hla, rounds[r], F.ratios);
		hipLaunchKernelGGL(k_finish_family, dim3(B.n_pad / 64), dim3(64), 0, st, M, B, (const double *)d_part,
			(const double *)F.ratios, depth, rounds[r], d_H1, d_H2, d_prob, d_support, d_matching, fam_S);
		hipLaunchKernelGGL(k_family_dosage, dim3(B.n_pad / 64, (M.n_hla + FIN_SEG - 1) / FIN_SEG), dim3(64 * FIN_SEG), 0, st, M, B,
			(const double *)d_part, (const double *)F.ratios, depth, rounds[r], fam_D, d_dosage);
	}
}

void hibag_launch_oob(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_codes, const HibagOobOut &O,
	int force_rescan, const HibagSideStream &side, hipStream_t st)
{
	if (M.n_classifier == 0) return;
	hipLaunchKernelGGL(k_oob_weight, dim3(B.n_pad / 64, M.n_classifier), dim3(64), 0, st, M, B, d_codes, O);
	hibag_launch_total(M, B, st, side, true);
	hipLaunchKernelGGL(k_oob_pick, dim3(B.n_pad / 64, M.n_classifier), dim3(64), 0, st, M, B, d_codes, O, force_rescan);
	if (M.n_wide > 0) hipLaunchKernelGGL(k_oob_scan, dim3(B.n_pad / 64, M.n_wide), dim3(64), 0, st, M, B, O);
	if (M.n_valu > 0) {
		const unsigned gx = (unsigned)((B.n_pad / HIBAG_WAVE + BLOCK_WAVES - 1) / BLOCK_WAVES);
		hipLaunchKernelGGL(k_oob_best_valu, dim3(gx, M.n_classifier), dim3(BLOCK_THREADS), 0, st, M, B, O);
	}
}

void hibag_launch_mask_weights(const HibagModelView &M, const HibagBatchView &B, const uint8_t *d_codes, const HibagMaskView &K,
	hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0) return;
	hipLaunchKernelGGL(k_mask_counts, dim3(B.n_pad / 64, M.n_snp), dim3(64), 0, st, M, B, K);
	hipLaunchKernelGGL(k_mask_weight, dim3(B.n_pad / 64, M.n_classifier), dim3(64), 0, st, M, B, d_codes, K);
}

void hibag_launch_knock_base(const HibagModelView &M, const int32_t *d_geno, int n_samp, uint8_t *d_base, hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0 || n_samp <= 0) return;
	HibagBatchView B0{};                              // (k_codes reads the two sizes only)
	B0.n_samp = n_samp;
	B0.n_pad = (n_samp + 63) / 64 * 64;
	hipLaunchKernelGGL(k_codes, dim3(B0.n_pad / 64, (M.n_snp + 63) / 64), dim3(256), 0, st, M, B0, d_geno, M.n_snp,
		(const int32_t *)nullptr, (const int32_t *)nullptr, d_base);
}

// The launcher of a knock-out batch beside hibag_launch_oob: its pass 1 and picks, launched the same way, between the
// virtual pack and the tallies.
#define KNOCK_TALLY_Y 16                            // workgroups that share the users of a group's SNP
void hibag_launch_knock(const HibagModelView &M, const HibagBatchView &B, const HibagKnockView &K, uint8_t *d_codes,
	const HibagOobOut &O, int n_base, int force_rescan, const HibagSideStream &side, hipStream_t st)
{
	if (M.n_classifier == 0 || M.n_snp == 0) return;
	const unsigned groups = (unsigned)(B.n_pad / 64);
	hipLaunchKernelGGL(k_knock_codes, dim3(groups, (M.n_snp + 3) / 4), dim3(256), 0, st, M, B, K, d_codes);
	hipLaunchKernelGGL(k_pack, dim3(B.n_pad / HIBAG_WAVE, (M.n_classifier + PACK_WAVES - 1) / PACK_WAVES), dim3(PACK_WAVES * HIBAG_WAVE), 0, st, M, B,
		(const uint8_t *)d_codes);
	hipLaunchKernelGGL(k_knock_weight, dim3(groups, M.n_classifier), dim3(64), 0, st, M, B, (const uint8_t *)d_codes, K);
	hibag_launch_total(M, B, st, side, true);
	hipLaunchKernelGGL(k_oob_pick, dim3(B.n_pad / 64, M.n_classifier), dim3(64), 0, st, M, B, (const uint8_t *)d_codes, O, force_rescan);
	if (M.n_wide > 0) hipLaunchKernelGGL(k_oob_scan, dim3(B.n_pad / 64, M.n_wide), dim3(64), 0, st, M, B, O);
	if (M.n_valu > 0) {
		const unsigned gx = (unsigned)((B.n_pad / HIBAG_WAVE + BLOCK_WAVES - 1) / BLOCK_WAVES);
		hipLaunchKernelGGL(k_oob_best_valu, dim3(gx, M.n_classifier), dim3(BLOCK_THREADS), 0, st, M, B, O);
	}
	// the base groups first: the variants of this and of every later batch read the calls they keep
	const unsigned nb = (unsigned)std::min<int>(std::max(n_base, 0), (int)groups);
	if (nb > 0) hipLaunchKernelGGL(k_knock_tally, dim3(nb, KNOCK_TALLY_Y), dim3(64), 0, st, M, B, K, O, 0);
	if (groups > nb) hipLaunchKernelGGL(k_knock_tally, dim3(groups - nb, KNOCK_TALLY_Y), dim3(64), 0, st, M, B, K, O, (int)nb);
}
