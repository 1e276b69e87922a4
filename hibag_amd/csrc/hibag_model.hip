// hibag_model.hip -- the model of libhibag_hip.so: classifiers come in through hibag_hip_model_new / _add_classifier
// (HIBAG_New, HIBAG_NewClassifierHaplo, src/HIBAG.cpp:486-503, :817-841), hibag_hip_model_finalize lays them out for the
// kernels (hibag_device.h: haplotype tables, pair lists with their factors and headers, prebuilt A-operand rows, the
// second pass's block stream, tiles, work items) and decides which cell sums pass 1 stores; replicas and classifier shards
// are models built from the same classifiers on another device.  No compute here.

#include "hibag_internal.h"

namespace hibag_detail {

// The mutation/error weights exp(d*log(1e-5)), TAB[0]=1, non-finite -> 0:
// the same expression, evaluated by the host libm like the reference does in
// its static initialiser (src/LibHLA.cpp:166-183).
void build_table(double *tab)
{
	const double min_rare_freq = 1e-5;   // inst/include/LibHLA_ext.h:230
	for (int i = 0; i < HIBAG_TAB_N; i++) tab[i] = std::exp(i * std::log(min_rare_freq));
	tab[0] = 1;
	for (int i = 0; i < HIBAG_TAB_N; i++)
		if (!std::isfinite(tab[i])) tab[i] = 0;
}

int check_classifier_args(hibag_hip_model *m, int n_snp_c, const int32_t *snpidx, int n_haplo,
	const double *freq, const int32_t *hla)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model already finalized");
	if (n_snp_c < 0 || n_snp_c > HIBAG_HIP_MAX_SNP_IN_CLASSIFIER)
		return hibag_fail(HIBAG_HIP_EINVAL, "there are too many SNP markers in a classifier (%d > %d).",
			n_snp_c, HIBAG_HIP_MAX_SNP_IN_CLASSIFIER);
	if (n_haplo < 0 || (n_haplo > 0 && (!freq || !hla)))
		return hibag_fail(HIBAG_HIP_EINVAL, "invalid haplotype list");
	if (snpidx)
		for (int i = 0; i < n_snp_c; i++)
			if (snpidx[i] < 0 || snpidx[i] >= m->n_snp)
				return hibag_fail(HIBAG_HIP_EINVAL, "SNP index %d out of range [0,%d)", snpidx[i], m->n_snp);
	for (int i = 0; i < n_haplo; i++) {
		if (hla[i] < 0 || hla[i] >= m->n_hla)
			return hibag_fail(HIBAG_HIP_EINVAL, "HLA allele index %d out of range [0,%d)", hla[i], m->n_hla);
		if (i > 0 && hla[i] < hla[i - 1])
			return hibag_fail(HIBAG_HIP_EINVAL, "haplotypes must be grouped by ascending HLA allele index");
	}
	return 0;
}

void push_classifier(hibag_hip_model *m, int n_snp_c, const int32_t *snpidx, int n_haplo,
	const double *freq, const int32_t *hla, std::vector<uint64_t> &&bits)
{
	HostClassifier c;
	c.n_snp = n_snp_c;
	if (snpidx) c.snpidx.assign(snpidx, snpidx + n_snp_c);
	else m->have_snpidx = false;
	c.freq.assign(freq, freq + n_haplo);
	c.hla.assign(hla, hla + n_haplo);
	c.bits = std::move(bits);
	m->cls.push_back(std::move(c));
	m->oob_hap_ready = false;                // hibag_hip_model_distance may have built the table of an unfinalized model
	m->snp_users_ready = false;
}

// Words per pair record: ceil(3k/32) rounded up to a width the kernels are
// specialised for (HIBAG_DISPATCH_NWP in hibag_kernels.hip).
int round_nwp(int n)
{
	for (int v : {1, 2, 3, 4, 6, 8, 10, 12})
		if (n <= v) return v;
	return HIBAG_MAX_NWP;
}

// OR the low `nbits` bits of the 128-bit value src into the multiword string dst at bit `pos`.
void or_bits(uint32_t *dst, const uint64_t src[2], int nbits, int pos)
{
	for (int i = 0; i < nbits; i++)
		if ((src[i >> 6] >> (i & 63)) & 1) dst[(pos + i) >> 5] |= 1u << ((pos + i) & 31);
}

// Flatten one classifier's _PostProb2 loop nest (src/LibHLA.cpp:1776-1821) into
// pair records in the reference's visiting order.  For every allele-pair cell
// (posterior order) appends whole chunks to `stream` and returns the chunk count
// per cell in `cell_chunks[P]`.  The frequency factor is rounded exactly as the
// reference does: f1*f1 for the leading diagonal term (:1786), (2*f1)*f2 else
// (:1789-1793, :1808-1812); this file is compiled with -ffp-contract=off.
void build_pair_stream(const HostClassifier &k, int n_hla, int nwp, const int *st,
	std::vector<uint32_t> &stream, std::vector<uint32_t> &cell_chunks)
{
	const int ks = k.n_snp;
	const uint64_t lowmask[2] = {
		ks >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << ks) - 1),
		ks >= 128 ? ~(uint64_t)0 : (ks <= 64 ? 0 : (((uint64_t)1 << (ks - 64)) - 1)) };
	std::vector<uint32_t> recw;       // records of the current cell: nwp words each
	std::vector<double> recp;
	auto emit = [&](int a, int b, double prod) {
		const uint64_t *A = &k.bits[2 * (size_t)a], *Bb = &k.bits[2 * (size_t)b];
		const uint64_t same[2] = { ~(A[0] ^ Bb[0]) & lowmask[0], ~(A[1] ^ Bb[1]) & lowmask[1] };
		const size_t at = recw.size();
		recw.resize(at + nwp, 0);
		or_bits(&recw[at], A, ks, 0);
		or_bits(&recw[at], Bb, ks, ks);
		or_bits(&recw[at], same, ks, 2 * ks);
		recp.push_back(prod);
	};
	auto flush = [&]() -> uint32_t {
		const size_t n = recp.size();
		const size_t nchunk = (n + HIBAG_CHUNK - 1) / HIBAG_CHUNK;
		for (size_t ch = 0; ch < nchunk; ch++) {
			const size_t base = stream.size();
			stream.resize(base + HIBAG_CHUNK_DWORDS(nwp), 0);
			for (int r = 0; r < HIBAG_CHUNK; r++) {
				const size_t i = ch * HIBAG_CHUNK + r;
				double prod = 0.0;                    // padding record: + (+0.0 * TAB[d]) is exact
				if (i < n) {
					for (int w = 0; w < nwp; w++) stream[base + (size_t)w * HIBAG_CHUNK + r] = recw[i * nwp + w];
					prod = recp[i];
				}
				memcpy(&stream[base + (size_t)nwp * HIBAG_CHUNK + 2 * (size_t)r], &prod, sizeof(double));
			}
		}
		recw.clear(); recp.clear();
		return (uint32_t)nchunk;
	};
	size_t p = 0;
	for (int h1 = 0; h1 < n_hla; h1++) {
		const int a0 = st[h1], a1 = st[h1 + 1];
		for (int a = a0; a < a1; a++) {
			emit(a, a, k.freq[a] * k.freq[a]);
			const double ff = 2 * k.freq[a];
			for (int b = a + 1; b < a1; b++) emit(a, b, ff * k.freq[b]);
		}
		cell_chunks[p++] = flush();
		for (int h2 = h1 + 1; h2 < n_hla; h2++) {
			const int b0 = st[h2], b1 = st[h2 + 1];
			for (int a = a0; a < a1; a++) {
				const double ff = 2 * k.freq[a];
				for (int b = b0; b < b1; b++) emit(a, b, ff * k.freq[b]);
			}
			cell_chunks[p++] = flush();
		}
	}
}

// Matrix-core engine: the pair list of a run of cells [p0, p0 + n) of one classifier, appended to `out`
// as blocks of 32 slots (i1 | i2 << 16 | end << 31).  The visiting order inside a
// cell is the reference's (src/LibHLA.cpp:1776-1821: i1 ascending, then i2; the leading diagonal pair
// (i, i) first on the diagonal cells).  Cells are padded to an even slot count with the classifier's
// all-zero haplotype `pad` (frequency 0: the slot adds +0.0); the end flag marks the slot that closes
// a cell; the unused slots behind the last cell point at `pad` too.  (h1, h2) of the first cell p0 are given; returns the number of blocks.
int append_pair_blocks(const int *st, int n_hla, int h1, int h2, int p0, int n_cells, uint32_t pad, std::vector<uint32_t> &out,
	const uint8_t *mark, const uint8_t *skip)
{
	// mark[p]: the closing slot of cell p carries the STORE flag; skip[p]: cell p is left out (pass-2 lists: its sum
	// comes from memory); both indexed by posterior cell, either may be null
	const uint32_t pad_idx = pad | (pad << 16);
	size_t base = 0;
	int fill = 32, n_blocks = 0;                 // slots used in the open block (32 = none open)
	uint32_t end_flags = HIBAG_PLIST_END;
	auto slot = [&](uint32_t idx, bool end) {
		if (fill == 32) {
			base = out.size();
			out.resize(base + HIBAG_PLIST_DWORDS, pad_idx);
			fill = 0; n_blocks++;
		}
		out[base + fill++] = idx | (end ? end_flags : 0u);
	};
	for (int c = 0; c < n_cells; c++) {
		const int a0 = st[h1], a1 = st[h1 + 1], b0 = st[h2], b1 = st[h2 + 1];
		const uint64_t n = h1 == h2 ? (uint64_t)(a1 - a0) * (a1 - a0 + 1) / 2 : (uint64_t)(a1 - a0) * (b1 - b0);
		if (n && !(skip && skip[p0 + c])) {
			end_flags = HIBAG_PLIST_END | (mark && mark[p0 + c] ? HIBAG_PLIST_STORE : 0u);
			uint64_t i = 0;
			const uint64_t total = n + (n & 1);
			if (h1 == h2) {
				for (int a = a0; a < a1; a++) {
					i++; slot((pad + 1 + (uint32_t)a) | ((uint32_t)a << 16), i == total);      // (a, a): factor f * f
					for (int b = a + 1; b < a1; b++) { i++; slot((uint32_t)a | ((uint32_t)b << 16), i == total); }
				}
			} else {
				for (int a = a0; a < a1; a++)
					for (int b = b0; b < b1; b++) { i++; slot((uint32_t)a | ((uint32_t)b << 16), i == total); }
			}
			if (n & 1) slot(pad_idx, true);
		}
		if (++h2 == n_hla) { h1++; h2 = h1; }
	}
	return n_blocks;
}

// Tiles for pass 2: consecutive posterior cells, at most HIBAG_TILE each, cut so
// that the chunk counts (summed over classifiers, plus a per-cell constant) are
// balanced.
// `cap`: cells per tile at most (<= HIBAG_TILE, what a wavefront of pass 2 has LDS rows for).  Pass 2's parallelism is
// (groups of 64 samples) x (tiles): a model of few alleles cut into tiles of fifteen leaves most of the device idle -- the
// reference's bundled HLA-A model, 14 alleles = 105 cells = 7 tiles, made 1,100 wavefronts of a 10,000-sample batch for
// 1,024 SIMDs that hold five each, and pass 2 took 1.7 x pass 1 -- so such a model gets smaller tiles (plan_tiles).
void build_tiles(int P, const std::vector<uint64_t> &cell_work, std::vector<int> &tile_p0, std::vector<int> &tile_n, int cap)
{
	uint64_t total = 0;
	for (int p = 0; p < P; p++) total += cell_work[p] + 1;
	const int TILE = std::max(1, std::min(cap, HIBAG_TILE));
	const int min_tiles = (P + TILE - 1) / TILE;
	const uint64_t target = std::max<uint64_t>(1, total / (uint64_t)std::max(min_tiles, 1));
	// A tile is a wavefront of pass 2, and four tiles make a workgroup: every tile beyond the minimum
	// is another wavefront per sample group (and possibly another, mostly empty, workgroup).  A tile is
	// therefore closed early for balance only while the cells it leaves unused still fit into the
	// minimum number of tiles.
	int slack = min_tiles * TILE - P;
	tile_p0.clear(); tile_n.clear();
	int p = 0;
	while (p < P) {
		int n = 0;
		uint64_t w = 0;
		while (p + n < P && n < TILE) {
			const uint64_t cw = cell_work[p + n] + 1;
			if (n > 0 && w + cw > target + target / 4 && TILE - n <= slack) break;
			w += cw; n++;
		}
		if (p + n < P) slack -= TILE - n;
		tile_p0.push_back(p); tile_n.push_back(n);
		p += n;
	}
}

// The overrides finalize_model honours, read from the environment at every finalize (the tests change them between models).
struct FinalizeOptions {
	enum Pass2 { AUTO, STREAM, HYBRID, RECOMPUTE } pass2 = AUTO;   // HIBAG_PASS2: which cell sums pass 1 stores (plan_store)
	uint64_t store_above = 12;       // HIBAG_STORE_PAIRS: cells of more haplotype pairs are stored (plan_store)
	double prebuilt_mb = 128;        // HIBAG_PREBUILT_MB: prebuilt rows for the pass-1 lists below this size (plan_parow)
	FinalizeOptions()
	{
		if (const char *e = getenv("HIBAG_PASS2"))
			pass2 = !strcmp(e, "stream") ? STREAM : !strcmp(e, "hybrid") ? HYBRID : !strcmp(e, "recompute") ? RECOMPUTE : AUTO;
		if (const char *e = getenv("HIBAG_STORE_PAIRS")) store_above = (uint64_t)std::max(0, atoi(e));
		if (const char *e = getenv("HIBAG_PREBUILT_MB")) prebuilt_mb = atof(e);
	}
};

// The kernels' tables and scalars, built without a HIP call by the plan_* stages (trailing comments: which), then uploaded.
struct ModelLayout {
	struct ClassifierPlan {                 // what the stages keep per classifier besides the kernels' arrays
		std::vector<int> st;                    // [n_hla + 1] first haplotype of every allele
		std::vector<uint32_t> chunks, npairs;   // [P] 4-record chunks and haplotype pairs (matrix engines only) of every cell
		std::vector<uint8_t> stored;            // [P] pass 1 stores the cell's sum
		int64_t pairs = 0;                      // haplotype pairs of the classifier
	};
	struct SlotRange { size_t first, n; int c; };   // which classifier's haplotype table the slots of plist[first, first + n) index
	int C, nh, S, P;
	std::vector<ClassifierPlan> cp;
	std::vector<int> n_snp_c, nwp, snp_off, mask_row, c_order, snp_index, snp_weight, engine, bt_row, cls_nblk, n_step;   // plan_classifiers
	std::vector<uint64_t> stream_off, cell_work;
	std::vector<uint32_t> stream, hap, hap_off;
	int rows = 0, bt_rows = 0;
	int64_t pair_evals = 0;
	std::vector<int> tile_p0, tile_n, tile_h1, tile_h2;      // plan_tiles; tile_h1, tile_h2: (h1, h2) of every tile's first cell
	int n_tile = 0, store_mode = 0;                          // store_mode: plan_store
	std::vector<uint32_t> cls_cnt, cls_cell, tile_meta, tile_k0, tile_nlist, tile_nstored;   // plan_cell_lists
	std::vector<uint64_t> tile_jpack;
	std::vector<int> cls_off, cls_n, n_stored_c;             // n_stored_c: cells of the classifier pass 1 stores in mode 2
	int64_t second_pass_pairs = 0;
	std::vector<int> item, item_whole, split_row, split_cls, wide_cls;   // plan_work_items
	double split_heavy_ns = 0, split_rest_ns = 0;
	std::vector<uint32_t> plist, ehdr, etile_cstart, blk_close;          // plan_pair_lists
	std::vector<uint64_t> etile_blk0, blk_off, wseg_off;
	std::vector<SlotRange> slot_ranges;
	std::vector<int> cell_row, wseg, wide_scan;             // wide_scan: the classifiers of several K steps whose total k_total_scan forms
	uint64_t estream_blocks = 0, p1_base = 0;
	long long p1_blocks = 0;
	std::vector<double> pfac;                                // plan_factors, plan_parow, plan_ctile
	std::vector<uint32_t> phdr, parow, ctile;
	size_t parow_blocks = 0;
	bool p1_prebuilt = false;
	explicit ModelLayout(const hibag_hip_model *m)
		: C((int)m->cls.size()), nh(m->n_hla), S(m->n_snp), P(nh * (nh + 1) / 2), cp(C), n_snp_c(C), nwp(C), snp_off(C), mask_row(C),
		  c_order(C), snp_weight(std::max(S, 1), 0), engine(std::max(C, 1), 0), bt_row(std::max(C, 1), 0), cls_nblk(std::max(C, 1), 0),
		  n_step(std::max(C, 1), 1), stream_off(std::max(C, 1), 0), cell_work(P, 0), hap_off(std::max(C, 1), 0) {}
	// Pass 2 evaluates the pairs of one-step FP4 classifiers only (k_accum's block stream); a classifier on any other engine
	// -- int8 (29..32 SNPs), FP4 in several K steps, VALU -- has all its cells stored by pass 1 and read back.
	bool evaluates(int c) const { return engine[c] == HIBAG_ENGINE_FP4 && n_step[c] == 1; }
	bool stored_big(int c, int p) const { return store_mode == 2 && cp[c].stored[p] != 0; }   // mode 2: pass 2 reads the cell's sum
};

// Appends the table entry {ff, f} of haplotype i (-1: the all-zero padding entry) of a matrix-engine classifier to `hap`.
void append_hap_entry(const HostClassifier &k, int engine, int steps, double ff, int i, double f, std::vector<uint32_t> &hap)
{
	const bool fp4 = engine == HIBAG_ENGINE_FP4;
	// bits of a haplotype: SNPs [lo, lo + 32) of its 128-bit string
	auto window = [&](int i, int lo) -> uint32_t {
		if (i < 0) return 0u;
		const unsigned __int128 v = ((unsigned __int128)k.bits[2 * (size_t)i + 1] << 64) | k.bits[2 * (size_t)i];
		return (uint32_t)(v >> lo);
	};
	uint32_t w[12 + 4 * (HIBAG_FP4_MAX_STEPS - 1)] = {0};
	int n = 0;
	if (fp4 && steps == 1) {       // two nibble images, both ADDED by the kernel (K layout in hibag_device.h):
		// the "sum" image has nibble s = 2 (the e2m1 code of 1.0) where bit s is set, the "pair" image the code 3 (1.5) --
		// two of them make the code 6 (4.0), so the sum of two pair images is w = 0 / 1.5 / 4 for 0 / 1 / 2 set bits
		const uint32_t bits = window(i, 0);
		for (int sb = 0; sb < 32; sb++) {
			w[sb >> 3] |= ((bits >> sb) & 1u) << (4 * (sb & 7) + 1);
			w[4 + (sb >> 3)] |= (((bits >> sb) & 1u) * 3u) << (4 * (sb & 7));
		}
		if (i >= 0) {
			// ... plus the A-row constants of the offset digits at nibbles k, k + 1: each image carries half of each (sum
			// image: codes 1 and 3, 0.5 + 0.5 = 1 and 3 + 3 = code 6 = 4; pair image: 3 and 3 -> 4, 4).  (Not the padding
			// entry: its rows must stay zero.)
			const int ks = k.n_snp;
			for (int q = 0; q < 2; q++) {
				const int nib = ks + q;
				w[nib >> 3] |= (q == 0 ? 1u : 3u) << (4 * (nib & 7));
				w[4 + (nib >> 3)] |= 3u << (4 * (nib & 7));
			}
		}
		n = 8;
	} else if (fp4) {              // nibble s = 2 (the e2m1 code of 1.0) where bit s is set
		const uint32_t bits = window(i, 0) & ((1u << HIBAG_FP4_STEP_SNPS) - 1);
		for (int sb = 0; sb < 32; sb++) w[sb >> 3] |= ((bits >> sb) & 1u) << (4 * (sb & 7) + 1);
		n = 4;
	} else {                       // byte s = 1 where bit s is set
		const uint32_t bits = window(i, 0);
		for (int sb = 0; sb < 32; sb++) w[sb >> 2] |= ((bits >> sb) & 1u) << (8 * (sb & 3));
		n = 8;
	}
	memcpy(&w[n], &ff, sizeof(double)); memcpy(&w[n + 2], &f, sizeof(double));
	n += 4;
	for (int j = 1; j < steps; j++, n += 4) {      // further K steps: the next 28 SNPs each
		const uint32_t bits = window(i, HIBAG_FP4_STEP_SNPS * j) & ((1u << HIBAG_FP4_STEP_SNPS) - 1);
		for (int sb = 0; sb < 32; sb++) w[n + (sb >> 3)] |= ((bits >> sb) & 1u) << (4 * (sb & 7) + 1);
	}
	hap.insert(hap.end(), w, w + n);
}

// Stage 1, per classifier: engine, rows, allele starts, the cells' pairs and chunks, its table entries or pair records.
int plan_classifiers(const hibag_hip_model *m, const FinalizeOptions &opt, ModelLayout &L)
{
	const int nh = L.nh, P = L.P;
	for (int c = 0; c < L.C; c++) {
		const HostClassifier &k = m->cls[c];
		ModelLayout::ClassifierPlan &cp = L.cp[c];
		const int H = (int)k.freq.size();
		L.n_snp_c[c] = k.n_snp;
		L.nwp[c] = round_nwp((3 * k.n_snp + 31) / 32);
		L.snp_off[c] = (int)L.snp_index.size();
		for (int v : k.snpidx) { L.snp_index.push_back(v); L.snp_weight[v]++; }
		if (k.snpidx.empty()) L.snp_index.insert(L.snp_index.end(), (size_t)k.n_snp, 0);
		L.mask_row[c] = L.rows;
		L.rows += 2 * L.nwp[c];
		cp.st.assign(nh + 1, 0);
		for (int i = 0; i < H; i++) cp.st[k.hla[i] + 1]++;
		for (int h = 0; h < nh; h++) cp.st[h + 1] += cp.st[h];
		// matrix-core engines: at most 112 SNPs; table indices: first haplotype < 2H + 1 in 16 bits, second < H + 1 in 14
		L.engine[c] = (m->use_mfma && H < 16384) ? HIBAG_ENGINE_OF(k.n_snp, m->use_fp4) : HIBAG_ENGINE_VALU;
		// (several K steps need their cells stored: not with pass 2 forced to evaluate every pair)
		if (L.engine[c] == HIBAG_ENGINE_FP4 && k.n_snp > HIBAG_FP4_MAX_SNPS && opt.pass2 == FinalizeOptions::RECOMPUTE) L.engine[c] = HIBAG_ENGINE_VALU;
		L.n_step[c] = HIBAG_ENGINE_STEPS(L.engine[c], k.n_snp);
		L.bt_row[c] = L.bt_rows;
		L.bt_rows += HIBAG_ENGINE_ROWS(L.engine[c], k.n_snp);
		cp.chunks.assign(P, 0);
		cp.npairs.assign(P, 0);
		if (L.engine[c] != HIBAG_ENGINE_VALU) {
			// no record stream: the kernels generate the records from the haplotype table
			L.hap_off[c] = (uint32_t)L.hap.size();
			for (int i = 0; i < H; i++) append_hap_entry(k, L.engine[c], L.n_step[c], 2 * k.freq[i], i, k.freq[i], L.hap);
			append_hap_entry(k, L.engine[c], L.n_step[c], 0.0, -1, 0.0, L.hap);                   // H: the padding entry (frequency +0.0)
			for (int i = 0; i < H; i++) append_hap_entry(k, L.engine[c], L.n_step[c], k.freq[i], i, k.freq[i], L.hap);   // H+1+i: first of a diagonal pair
			size_t p = 0;
			for (int h1 = 0; h1 < nh; h1++)
				for (int h2 = h1; h2 < nh; h2++) {
					const uint64_t n1 = (uint64_t)(cp.st[h1 + 1] - cp.st[h1]), n2 = (uint64_t)(cp.st[h2 + 1] - cp.st[h2]);
					const uint64_t n = h1 == h2 ? n1 * (n1 + 1) / 2 : n1 * n2;
					if (n > 0xFFFFFFull * HIBAG_CHUNK) return hibag_fail(HIBAG_HIP_EINVAL, "an allele pair of classifier %d has too many haplotype pairs", c);
					cp.npairs[p] = (uint32_t)n;
					cp.chunks[p++] = (uint32_t)((n + HIBAG_CHUNK - 1) / HIBAG_CHUNK);
				}
		} else {
			if (L.stream.size() & 1) L.stream.push_back(0);          // 8-byte alignment of the doubles inside
			L.stream_off[c] = L.stream.size();
			build_pair_stream(k, nh, L.nwp[c], cp.st.data(), L.stream, cp.chunks);
		}
		for (int p = 0; p < P; p++) L.cell_work[p] += (uint64_t)cp.chunks[p] * (L.nwp[c] + 2);
		cp.pairs = (int64_t)H * (H + 1) / 2;
		L.pair_evals += cp.pairs;
		L.c_order[c] = c;
	}
	if (!m->snp_weight_override.empty()) L.snp_weight = m->snp_weight_override;
	std::stable_sort(L.c_order.begin(), L.c_order.end(), [&](int a, int b) { return L.cp[a].pairs * L.nwp[a] > L.cp[b].pairs * L.nwp[b]; });
	// the walker fetches one chunk ahead: keep a widest-record chunk of slack behind the last record
	L.stream.insert(L.stream.end(), HIBAG_CHUNK_DWORDS(HIBAG_MAX_NWP), 0);
	if (L.snp_index.empty()) L.snp_index.push_back(0);
	if (L.hap.empty()) L.hap.insert(L.hap.end(), 12, 0u);
	if (L.hap.size() * sizeof(uint32_t) > 0x7FFFFF00ull) return hibag_fail(HIBAG_HIP_EINVAL, "the model's haplotype tables exceed 2 GB");
	// (an all-zero FP4 entry behind the tables: reads of the haplotype table through a slot of a padding block land here)
	L.hap.insert(L.hap.end(), HIBAG_ENGINE_HAP_DWORDS(HIBAG_ENGINE_FP4), 0u);
	while (L.hap.size() % 4) L.hap.push_back(0u);
	return 0;
}

// Stage 2: the tiles of pass 2 (build_tiles) and the (h1, h2) of every tile's first cell.
void plan_tiles(ModelLayout &L)
{
	// cells per tile: fifteen where that still makes ~48 tiles or more (50 alleles: 85), fewer for models of few alleles, down
	// to four (a visit of fewer cells is mostly block overhead)
	const int tile_cap = std::max(4, std::min(HIBAG_TILE, (L.P + 47) / 48));
	build_tiles(L.P, L.cell_work, L.tile_p0, L.tile_n, tile_cap);
	L.n_tile = (int)L.tile_p0.size();
	L.tile_h1.assign(L.n_tile, 0); L.tile_h2.assign(L.n_tile, 0);
	for (int h1 = 0, t = 0, p = 0; h1 < L.nh && t < L.n_tile; h1++)
		for (int h2 = h1; h2 < L.nh && t < L.n_tile; h2++, p++)
			if (p == L.tile_p0[t]) { L.tile_h1[t] = h1; L.tile_h2[t] = h2; t++; }
}

// Stage 3: which cell sums pass 1 stores for pass 2 (HibagModelView::store_cells, and `stored` of every classifier).  Measured
// on MI355X: evaluating a haplotype pair again costs ~0.25 ps per sample, a stored cell ~2.2 ps (written in pass 1, read in
// pass 2, both at HBM speed).  A model with many pairs per non-empty cell (the DRB1 shape: 73) stores every cell and pass 2
// only reads; otherwise (the HLA-B benchmark model: 8.5) the cells with more than `store_above` pairs of the matrix-engine
// classifiers are stored -- 15 % of its cells hold 62 % of its pairs -- and pass 2 evaluates the rest (thresholds 8 .. 16
// measure the same; below, the stores slow pass 1 down more than pass 2 gains).  HIBAG_PASS2 = stream | hybrid | recompute
// and HIBAG_STORE_PAIRS override.
void plan_store(const FinalizeOptions &opt, ModelLayout &L)
{
	const int C = L.C, P = L.P;
	const bool recompute = opt.pass2 == FinalizeOptions::RECOMPUTE;       // (no cell of theirs is stored)
	const uint64_t store_above = recompute ? ~(uint64_t)0 : opt.store_above;
	const uint32_t fit_min = recompute ? ~0u : 5u;           // the fit rule below (swept 0 .. 5: flat around 5, 4 % slower without it)
	long long n_cells = 0, n_big = 0;
	double cost = 0;                                   // pairs, a VALU-engine pair counted five times (what it costs)
	bool any_eval = false;                             // (none: e.g. HIBAG_ENGINE=valu)
	for (int c = 0; c < C; c++) {
		cost += (double)L.cp[c].pairs * (L.engine[c] ? 1.0 : 5.0);
		any_eval |= L.evaluates(c);
		for (int p = 0; p < P; p++) {
			n_cells += L.cp[c].chunks[p] != 0;
			n_big += L.evaluates(c) ? L.cp[c].npairs[p] > store_above : L.cp[c].chunks[p] != 0;
		}
	}
	L.store_mode = C == 0 ? 0 : cost >= 14.0 * (double)std::max<long long>(n_cells, 1) ? 1 : n_big ? 2 : 0;
	if (opt.pass2 == FinalizeOptions::STREAM) L.store_mode = C > 0;
	else if (opt.pass2 != FinalizeOptions::AUTO) L.store_mode = n_big ? 2 : 0;     // (recompute: only what pass 2 cannot evaluate is stored)
	if (L.store_mode == 2 && !any_eval) L.store_mode = 1;       // nothing pass 2 could evaluate: read everything back
	// stored[p]: pass 1 stores the sum of cell p of the classifier.  Mode 2: the cells of a matrix-engine classifier with
	// more than `store_above` pairs, at most HIBAG_STORED_PER_VISIT per (classifier, tile) -- the ones with the most pairs --
	// which is what pass 2 keeps in registers for a visit, and every cell of a VALU-engine classifier; mode 1: every non-empty cell.
	for (int c = 0; c < C; c++) {
		std::vector<uint8_t> &stored = L.cp[c].stored;
		stored.assign(P, 0);
		if (L.store_mode == 1 || (L.store_mode == 2 && !L.evaluates(c)))    // (mode 2: all the cells of a classifier pass 2 cannot evaluate)
			for (int p = 0; p < P; p++) stored[p] = L.cp[c].chunks[p] != 0;
		else if (L.store_mode == 2)
			for (int t = 0; t < L.n_tile; t++) {
				// Largest cells first: a cell with more than `store_above` pairs is stored; so is -- while the visit's
				// remaining pair slots would not fit ONE 32-slot block -- any cell of at least `fit_min` pairs: a second,
				// mostly empty block costs pass 2 more than a stored sum.
				std::vector<std::pair<uint32_t, int>> cells;
				uint32_t slots = 0;                            // pair slots of the visit (cells padded to an even count)
				for (int j = 0; j < L.tile_n[t]; j++) {
					const uint32_t n = L.cp[c].npairs[L.tile_p0[t] + j];
					if (n) { cells.push_back({n, L.tile_p0[t] + j}); slots += n + (n & 1u); }
				}
				std::stable_sort(cells.begin(), cells.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
				for (size_t i = 0; i < cells.size() && i < HIBAG_STORED_PER_VISIT; i++) {
					const uint32_t n = cells[i].first;
					if (!(n > store_above || (slots > HIBAG_PLIST_DWORDS && n >= fit_min))) break;
					stored[cells[i].second] = 1;
					slots -= n + (n & 1u);
				}
			}
	}
}

// Stage 4: pass 1 lists (non-empty cells per classifier) and pass 2 tile entries.
int plan_cell_lists(ModelLayout &L)
{
	const size_t CT = (size_t)std::max(L.C, 1) * L.n_tile;
	L.tile_meta.assign(CT * HIBAG_TILE_META + 1, 0);
	L.tile_k0.assign(CT, 0); L.tile_nlist.assign(CT, 0); L.tile_nstored.assign(CT, 0); L.tile_jpack.assign(CT, 0);
	L.cls_off.assign(std::max(L.C, 1), 0); L.cls_n.assign(std::max(L.C, 1), 0); L.n_stored_c.assign(std::max(L.C, 1), 0);
	for (int c = 0; c < L.C; c++) {
		const std::vector<uint32_t> &chunks = L.cp[c].chunks;
		L.cls_off[c] = (int)L.cls_cnt.size();
		for (int p = 0; p < L.P; p++)
			if (chunks[p]) { L.cls_cnt.push_back(chunks[p]); L.cls_cell.push_back((uint32_t)p); }
		L.cls_n[c] = (int)L.cls_cnt.size() - L.cls_off[c];
		L.cls_cnt.push_back(0); L.cls_cell.push_back(0);        // the walker reads one count ahead
		uint64_t off = 0;
		int k_first = 0;                                    // non-empty cells of the classifier in earlier tiles
		for (int t = 0; t < L.n_tile; t++) {
			const size_t ct = (size_t)c * L.n_tile + t;
			const int p0 = L.tile_p0[t];
			uint32_t *me = &L.tile_meta[ct * HIBAG_TILE_META];
			if (off > 0xFFFFFFFFull) return hibag_fail(HIBAG_HIP_EINVAL, "classifier %d has too many haplotype pairs", c);
			me[1] = (uint32_t)off;
			int k = 0;
			uint64_t jpack = 0;
			for (int j = 0; j < L.tile_n[t]; j++) {
				const uint32_t n = chunks[p0 + j];
				if (n > 0xFFFFFFu) return hibag_fail(HIBAG_HIP_EINVAL, "an allele pair of classifier %d has too many haplotype pairs", c);
				if (n) { jpack |= (uint64_t)j << (4 * k); me[4 + k++] = ((uint32_t)j << 24) | n; off += n; }
			}
			me[0] = (uint32_t)k;
			me[2] = (uint32_t)jpack; me[3] = (uint32_t)(jpack >> 32);
			// what pass 2 gets per (classifier, tile): the cells it evaluates (in closing order), then those it reads
			uint64_t jp = 0;
			int nl = 0, ns = 0;
			for (int j = 0; j < L.tile_n[t]; j++)
				if (chunks[p0 + j] && !L.stored_big(c, p0 + j)) {
					jp |= (uint64_t)j << (4 * nl++);
					if (L.store_mode != 1) L.second_pass_pairs += L.evaluates(c) ? L.cp[c].npairs[p0 + j] : 0;
				}
			for (int j = 0; j < L.tile_n[t]; j++)
				if (L.stored_big(c, p0 + j)) jp |= (uint64_t)j << (4 * (nl + ns++));
			L.tile_jpack[ct] = jp;
			L.tile_nlist[ct] = (uint32_t)nl;
			L.tile_nstored[ct] = (uint32_t)ns;
			L.tile_k0[ct] = (uint32_t)(L.store_mode == 2 ? L.n_stored_c[c] : k_first);   // mode 2: first stored row of the tile
			L.n_stored_c[c] += ns;
			k_first += k;
			for (int j = 0; j < L.tile_n[t]; j++)
				if (!chunks[p0 + j]) me[4 + k++] = (uint32_t)j << 24;
		}
	}
	if (L.cls_cnt.empty()) { L.cls_cnt.push_back(0); L.cls_cell.push_back(0); }
	return 0;
}

// Stage 5: the pass-1 work items.  One per classifier, except VALU-engine classifiers (more than 112 SNPs) whose work
// dwarfs the typical one: a single wavefront per sample group would walk them for many times the duration of the rest of
// the pass, so they are cut into items of typical size that store per-cell sums, added in order afterwards (k_total_scan).
void plan_work_items(ModelLayout &L)
{
	L.split_row.assign(std::max(L.C, 1), -1);
	// rough wavefront-time per record: matrix engine 50 ns at full occupancy, VALU engine 18 ns per
	// 32-bit word while other wavefronts share its SIMD (measured), 48 ns at full occupancy
	std::vector<double> work(L.C, 0.0);
	double typical = 0;
	int n_typ = 0;
	for (int c = 0; c < L.C; c++) {
		work[c] = (double)L.cp[c].pairs * (L.engine[c] ? 50.0 * (0.5 + 0.5 * L.n_step[c]) : 48.0 * L.nwp[c]);
		if (L.engine[c]) { typical += work[c]; n_typ++; }
		L.split_rest_ns += work[c];
	}
	typical = n_typ ? typical / n_typ : 0;
	std::vector<std::pair<double, std::vector<int>>> items, whole;
	for (int c = 0; c < L.C; c++) {
		if (L.n_step[c] > 1) { L.wide_cls.push_back(c); continue; }        // pass 1 in k_total_wide
		const int n = L.cls_n[c];
		const uint32_t *cnt = &L.cls_cnt[L.cls_off[c]];
		whole.push_back({work[c], {c, 0, n, 0}});
		int nseg = 1;
		if (!L.engine[c] && typical > 0 && work[c] > 3 * typical)
			nseg = (int)std::min<double>(64, std::max(2.0, std::floor(work[c] / typical)));
		if (nseg == 1 || n < 2) {
			items.push_back({work[c], {c, 0, n, 0}});
			continue;
		}
		L.split_heavy_ns = std::max(L.split_heavy_ns, (double)L.cp[c].pairs * 18.0 * L.nwp[c]);       // measured: 1.1 ms for 5,050 pairs x 12 words
		L.split_row[c] = 1;                              // (>= 0: split; its cells have rows in HibagBatchView::cells)
		L.split_cls.push_back(c);
		uint64_t total = 0, acc = 0, chunk0 = 0;
		for (int i = 0; i < n; i++) total += cnt[i] + 1;
		int i0 = 0, k = 1;
		for (int i = 0; i < n; i++) {
			acc += cnt[i] + 1;
			if (i + 1 == n || acc * nseg >= total * k) {
				uint64_t chunks = 0;
				for (int j = i0; j <= i; j++) chunks += cnt[j];
				items.push_back({work[c] * (double)(chunks + 1) / (double)total, {c, i0, i + 1, (int)chunk0}});
				chunk0 += chunks;
				i0 = i + 1;
				while (k < nseg && acc * nseg >= total * k) k++;
			}
		}
	}
	std::stable_sort(whole.begin(), whole.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
	for (const auto &it : whole) L.item_whole.insert(L.item_whole.end(), it.second.begin(), it.second.end());
	std::stable_sort(items.begin(), items.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
	for (const auto &it : items) L.item.insert(L.item.end(), it.second.begin(), it.second.end());
}

// Stage 6: the stored rows of every classifier and the pair lists of the matrix-core engine.  Pass 2 first, tile-major: the
// segments (tile t, classifier 0), (t, 1), ... follow each other, which is the order a pass-2 wavefront reads them in; then, per
// classifier, all cells back to back for pass 1 (no block left half empty at a tile boundary).
int plan_pair_lists(const hibag_hip_model *m, ModelLayout &L)
{
	const int C = L.C, n_tile = L.n_tile;
	L.cell_row.assign((size_t)C + 1, 0);
	for (int c = 0; c < C; c++)
		L.cell_row[c + 1] = L.cell_row[c] + (L.store_mode == 1 || L.split_row[c] >= 0 ? L.cls_n[c] : L.store_mode == 2 ? L.n_stored_c[c] : 0);
	// The E-stream of pass 2: per tile the blocks of classifier 0, 1, 2 ... (hibag_device.h).  A (classifier, tile) visit is
	// the blocks of its evaluated cells' pair slots -- one-step FP4 classifiers only -- with the visit's stored sums attached
	// four per block; a visit with more stored sums than its slot blocks carry (any classifier of another engine) gets
	// blocks of padding slots for the rest.
	L.etile_cstart.assign((size_t)n_tile * (C + 1), 0);
	L.etile_blk0.assign(std::max(n_tile, 1), 0);
	std::vector<uint32_t> &plist = L.plist, &ehdr = L.ehdr;
	for (int t = 0; t < n_tile && L.store_mode != 1; t++) {
		L.etile_blk0[t] = plist.size() / HIBAG_PLIST_DWORDS;
		for (int c = 0; c < C; c++) {
			const size_t ct = (size_t)c * n_tile + t;
			L.etile_cstart[(size_t)t * (C + 1) + c] = (uint32_t)(plist.size() / HIBAG_PLIST_DWORDS - L.etile_blk0[t]);
			const size_t first = plist.size();
			int nb = 0;
			if (L.evaluates(c) && L.tile_nlist[ct] > 0)
				nb = append_pair_blocks(L.cp[c].st.data(), L.nh, L.tile_h1[t], L.tile_h2[t], L.tile_p0[t], L.tile_n[t],
					(uint32_t)m->cls[c].freq.size(), plist, nullptr, L.store_mode == 2 ? L.cp[c].stored.data() : nullptr);
			if (nb > 0) L.slot_ranges.push_back({first, plist.size() - first, c});
			const int ns = (int)L.tile_nstored[ct];
			const int nvb = std::max(nb, (ns + HIBAG_STORED_PER_VISIT - 1) / HIBAG_STORED_PER_VISIT);
			for (int b = nb; b < nvb; b++) plist.insert(plist.end(), HIBAG_PLIST_DWORDS, 0u);     // padding slots: entry 0 of the zero entry's "table"
			// the visit's cells in closing order, then its stored ones (tile_jpack)
			uint64_t jp = L.tile_jpack[ct];
			uint64_t jps = jp >> (4 * L.tile_nlist[ct]);
			uint32_t srow = (uint32_t)L.cell_row[c] + L.tile_k0[ct];
			for (int b = 0; b < nvb; b++) {
				// the tile rows of the cells that close in this block, each at the place of its closing slot: slot i (odd: cells
				// are padded to an even number of slots) -> field i / 2
				uint64_t jq = 0;
				if (b < nb)
					for (int i = 0; i < HIBAG_PLIST_DWORDS; i++)
						if (plist[first + (size_t)b * HIBAG_PLIST_DWORDS + i] >> 31) {
							if (!(i & 1)) return hibag_fail(HIBAG_HIP_ESTATE, "internal: a cell of classifier %d closes at an even slot", c);
							jq |= (jp & 15u) << (4 * (i >> 1));
							jp >>= 4;
						}
				const int nsb = std::max(0, std::min(HIBAG_STORED_PER_VISIT, ns - HIBAG_STORED_PER_VISIT * b));
				if (c > 0xFFFF) return hibag_fail(HIBAG_HIP_EINVAL, "too many classifiers (%d) for the second pass's block headers", C);
				// (pass 2 requests the operand rows of every block it passes, also of blocks that only carry stored sums: a
				// classifier of the vector engine has no rows -- bt_row[c] is then the NEXT classifier's first row, or one past
				// the last row of the batch's array for the model's last classifiers: rows 0 and 1 instead)
				const uint32_t bt = (uint32_t)(HIBAG_ENGINE_ROWS(L.engine[c], L.n_snp_c[c]) > 0 ? L.bt_row[c] : 0);
				if (bt > 0xFFFFu) return hibag_fail(HIBAG_HIP_EINVAL, "too many classifiers for the matrix engine's operand rows");
				const uint32_t h[8] = {
					(uint32_t)c | (bt << 16), srow | ((uint32_t)nsb << 25),
					0u, 0u,                                   // (the next block's first two words: plan_factors)
					(uint32_t)jq, (uint32_t)(jq >> 32),
					(uint32_t)jps, 0u};
				ehdr.insert(ehdr.end(), h, h + 8);
				jps >>= 4 * nsb;
				srow += (uint32_t)nsb;
			}
		}
		L.etile_cstart[(size_t)t * (C + 1) + C] = (uint32_t)(plist.size() / HIBAG_PLIST_DWORDS - L.etile_blk0[t]);
	}
	// look-ahead slack: the loop requests block b + 1 whole and the slots / header of block b + 2
	L.estream_blocks = plist.size() / HIBAG_PLIST_DWORDS + 4;
	plist.insert(plist.end(), 4 * HIBAG_PLIST_DWORDS, 0u);
	ehdr.resize(L.estream_blocks * 8, 0u);
	L.p1_base = plist.size();
	L.blk_off.assign(std::max(C, 1), 0);
	for (int c = 0; c < C; c++) {
		if (!L.engine[c]) continue;
		const uint32_t pad = (uint32_t)m->cls[c].freq.size();
		L.blk_off[c] = plist.size();
		if (L.n_step[c] > 1) {
			// A classifier of several K steps: its list in segments of whole cells, each starting a block of its own, so
			// that different workgroups can walk them (their cell sums are stored, k_total_scan adds them in order);
			// walked as one list (majority vote) the padding between the segments adds nothing.
			// (pairs per segment: about what a typical one-step classifier of 5,000 pairs costs)
			// A model with many such classifiers has parallelism enough: then a classifier is ONE segment, its walk forms the
			// in-order total itself (wide_seg[3] = 1) and k_total_scan -- a second pass over every stored sum, HBM-bound --
			// is not needed for it.
			const bool whole = (int)L.wide_cls.size() >= 8;
			const long long seg_pairs = whole ? (1ll << 62) : std::max<long long>(512, 6000 / L.n_step[c]);
			bool any_seg = false;
			int p_lo = 0, h1_lo = 0, h2_lo = 0, row = 0, h1 = 0, h2 = 0;
			long long acc_pairs = 0;
			int rows_in_seg = 0;
			for (int p = 0; p < L.P; p++) {
				acc_pairs += L.cp[c].npairs[p];
				rows_in_seg += L.cp[c].npairs[p] != 0;
				int nh1 = h1, nh2 = h2 + 1;
				if (nh2 == L.nh) { nh1++; nh2 = nh1; }
				if (acc_pairs >= seg_pairs || p + 1 == L.P) {
					const size_t off = plist.size();
					const int nb = append_pair_blocks(L.cp[c].st.data(), L.nh, h1_lo, h2_lo, p_lo, p + 1 - p_lo, pad, plist, L.cp[c].stored.data(), nullptr);
					if (nb > 0) { L.wseg.insert(L.wseg.end(), {c, row, nb, whole ? 1 : 0}); L.wseg_off.push_back(off); any_seg = true; }
					row += rows_in_seg; rows_in_seg = 0; acc_pairs = 0;
					p_lo = p + 1; h1_lo = nh1; h2_lo = nh2;
				}
				h1 = nh1; h2 = nh2;
			}
			if (!whole || !any_seg) L.wide_scan.push_back(c);          // (a classifier without haplotypes has no segment: the scan writes its zero total)
		} else
			append_pair_blocks(L.cp[c].st.data(), L.nh, 0, 0, 0, L.P, pad, plist, L.store_mode ? L.cp[c].stored.data() : nullptr, nullptr);
		L.cls_nblk[c] = (int)((plist.size() - L.blk_off[c]) / HIBAG_PLIST_DWORDS);
		L.slot_ranges.push_back({(size_t)L.blk_off[c], plist.size() - (size_t)L.blk_off[c], c});
		L.p1_blocks += L.cls_nblk[c];
		uint32_t closed = 0;
		for (int b = 0; b < L.cls_nblk[c] && L.store_mode; b++) {      // stored cells closed before block b (0 for the segmented lists: not used)
			L.blk_close.push_back(L.n_step[c] > 1 ? 0u : closed);
			for (int i = 0; i < HIBAG_PLIST_DWORDS; i++) closed += (plist[L.blk_off[c] + (size_t)b * HIBAG_PLIST_DWORDS + i] >> 30) & 1u;
		}
	}
	if (L.blk_close.empty()) L.blk_close.push_back(0);
	plist.insert(plist.end(), 4 * HIBAG_PLIST_DWORDS, 0u);   // look-ahead slack of the block walker
	return 0;
}

// Stage 7: what the kernels take from a block through the SCALAR cache (hibag_device.h): the frequency factor of every slot --
// ff[i1] * f[i2], the one rounded multiplication of src/LibHLA.cpp:1786-1813, made here once instead of by every wavefront
// that walks the list -- and a header {cell ends, stored cell ends, slots worth evaluating}; then the E-stream's headers.
void plan_factors(const hibag_hip_model *m, ModelLayout &L)
{
	L.pfac.assign(L.plist.size(), 0.0);
	for (const auto &r : L.slot_ranges) {
		const std::vector<double> &freq = m->cls[r.c].freq;
		const uint32_t H = (uint32_t)freq.size();
		// table entries (plan_classifiers): [0, H) = {2 f, f}, H = the padding entry {0, 0}, H + 1 + i = {f, f} (first of a diagonal pair)
		auto ff_of = [&](uint32_t e) { return e < H ? 2 * freq[e] : e == H ? 0.0 : freq[e - H - 1]; };
		auto f_of = [&](uint32_t e) { return e < H ? freq[e] : e == H ? 0.0 : freq[e - H - 1]; };
		for (size_t i = r.first; i < r.first + r.n; i++) L.pfac[i] = ff_of(L.plist[i] & 0xFFFFu) * f_of((L.plist[i] >> 16) & 0x3FFFu);
	}
	L.phdr.assign(L.plist.size() / HIBAG_PLIST_DWORDS * 4, 0u);
	for (size_t b = 0; b < L.plist.size() / HIBAG_PLIST_DWORDS; b++) {
		uint32_t ends = 0, stores = 0, live = 0;
		for (int i = 0; i < HIBAG_PLIST_DWORDS; i++) {
			const uint32_t w = L.plist[b * HIBAG_PLIST_DWORDS + i];
			if (w & HIBAG_PLIST_END) ends |= 1u << i;
			if (w >= (HIBAG_PLIST_END | HIBAG_PLIST_STORE)) stores |= 1u << i;
			if (L.pfac[b * HIBAG_PLIST_DWORDS + i] != 0.0) live |= 1u << i;      // (a zero factor adds +0.0: skipping it is exact)
		}
		live |= ends;
		int n_valid = 0;
		while (n_valid < 32 && (live >> n_valid)) n_valid++;
		L.phdr[4 * b] = ends; L.phdr[4 * b + 1] = stores; L.phdr[4 * b + 2] = (uint32_t)n_valid;
	}
	// Pass 2 takes everything of a block from its E-stream header alone (hibag_device.h): the end mask goes where the block's
	// own request words were (word 0; they move to word 7 -- a walk needs them for its first block only, every other block
	// is requested through the words 2, 3 of the header before it), the groups of four records worth evaluating above the stored cells' rows.
	// Bit 29 of word 1: the record before the block's first one -- the last record gone through of the nearest block before it
	// that has any -- closed a cell, so the block's first product STARTS a sum (block_accumulate); a block that is passed over
	// (nobody uses its classifier) resets the sum instead, and a walk that begins at the block begins at zero: the bit is
	// right whichever blocks came before.
	uint32_t closed_before = 0;
	for (uint64_t b = 0; b < L.estream_blocks; b++) {
		const uint32_t groups = (L.phdr[4 * b + 2] + 3) / 4;
		L.ehdr[b * 8 + 7] = L.ehdr[b * 8];
		L.ehdr[b * 8] = L.phdr[4 * b];
		L.ehdr[b * 8 + 1] |= closed_before << 29;
		L.ehdr[b * 8 + 6] = (L.ehdr[b * 8 + 6] & 0x0FFFFFFFu) | (groups << 28);
		if (groups > 0) closed_before = (L.phdr[4 * b] >> (4 * groups - 1)) & 1u;
	}
	for (uint64_t b = 0; b + 1 < L.estream_blocks; b++) { L.ehdr[b * 8 + 2] = L.ehdr[(b + 1) * 8 + 7]; L.ehdr[b * 8 + 3] = L.ehdr[(b + 1) * 8 + 1]; }
}

// Stage 8: prebuilt A-operand rows (HibagModelView::parow): for every slot of a one-step FP4 classifier the element-wise sum of
// its two haplotypes' images -- the "sum" images for the lower K half (lanes 0..31), the "pair" images for the upper one
// (lanes 32..63); nibble sums never carry (codes 0..3 + 0..3).  Blocks outside a slot range (padding blocks) stay zero.
void plan_parow(const FinalizeOptions &opt, ModelLayout &L)
{
	const size_t n_blocks_all = L.plist.size() / HIBAG_PLIST_DWORDS;
	size_t fp4_p1_blocks = 0;
	for (int c = 0; c < L.C; c++) if (L.evaluates(c)) fp4_p1_blocks += (size_t)L.cls_nblk[c];
	L.p1_prebuilt = fp4_p1_blocks > 0 && (double)(n_blocks_all) * 1024.0 <= opt.prebuilt_mb * 1e6;
	L.parow_blocks = L.p1_prebuilt ? n_blocks_all : (size_t)L.estream_blocks;
	L.parow.assign(L.parow_blocks * 256, 0u);
	for (const auto &r : L.slot_ranges) {
		if (!L.evaluates(r.c)) continue;
		const uint32_t *tab_c = L.hap.data() + L.hap_off[r.c];
		for (size_t i = r.first; i < r.first + r.n; i++) {
			const size_t b = i / HIBAG_PLIST_DWORDS, sl = i % HIBAG_PLIST_DWORDS;
			if (b >= L.parow_blocks) break;
			const uint32_t *e1 = tab_c + (size_t)(L.plist[i] & 0xFFFFu) * 12, *e2 = tab_c + (size_t)((L.plist[i] >> 16) & 0x3FFFu) * 12;
			for (int h = 0; h < 2; h++)
				for (int d = 0; d < 4; d++) L.parow[(b * 64 + (size_t)h * 32 + sl) * 4 + d] = e1[4 * h + d] + e2[4 * h + d];
		}
	}
}

// Stage 9: the per (classifier, tile) record of pass 2 (one s_load_dwordx8), and the bounds of the stored rows.
int plan_ctile(ModelLayout &L)
{
	L.ctile.assign((size_t)std::max(L.C, 1) * L.n_tile * 8 + 8, 0);
	for (int c = 0; c < L.C; c++)
		for (int t = 0; t < L.n_tile; t++) {
			const size_t ct = (size_t)c * L.n_tile + t;
			uint32_t *r = &L.ctile[ct * 8];
			if (L.bt_row[c] > 0xFFFF) return hibag_fail(HIBAG_HIP_EINVAL, "too many classifiers for the matrix engine's operand rows");
			const int k_last = L.n_snp_c[c] - HIBAG_FP4_STEP_SNPS * (L.n_step[c] - 1);        // SNPs of the last K step (all of them for one step)
			r[0] = (uint32_t)L.engine[c] | ((uint32_t)k_last << 2 & 0xFCu) | (L.tile_nlist[ct] << 8) |
			       ((uint32_t)(L.n_step[c] - 1) << 13) | ((uint32_t)L.bt_row[c] << 16);
			r[1] = L.hap_off[c];
			r[2] = 0u; r[3] = 0u; r[4] = 0u;                 // (read by no kernel)
			// first stored row of the (classifier, tile) among all stored cells of the model
			const uint64_t row = (uint64_t)L.cell_row[c] + L.tile_k0[ct];
			if (row >> 27) return hibag_fail(HIBAG_HIP_EINVAL, "the model has too many allele pairs to store their sums");
			r[5] = (uint32_t)row | (L.tile_nstored[ct] << 27);
			r[6] = (uint32_t)L.tile_jpack[ct]; r[7] = (uint32_t)(L.tile_jpack[ct] >> 32);
		}
	if (L.store_mode != 1 && (uint64_t)L.cell_row[L.C] >= (1ull << 23))      // (k_accum: a stored row's byte offset within a sample group in 32 bits)
		return hibag_fail(HIBAG_HIP_EINVAL, "the model stores too many cell sums per sample (%d) for the second pass", L.cell_row[L.C]);
	return 0;
}

// One array of a device buffer: `bytes` from `src` in `room` (>= bytes) at an `align`-byte boundary, pointed at by `field`;
// `name` and `elem` (bytes per element) are what the layout export (hibag_hip_test_layout_*) hands out.
struct Part { const char *name; const void *src; size_t bytes, room, align, elem; void *field; };
template <class F, class T> Part part(const char *name, const F *&field, const std::vector<T> &v, size_t align, size_t min_n = 0)
{
	return {name, v.data(), v.size() * sizeof(T), std::max(v.size(), min_n) * sizeof(T), align, sizeof(T), &field};
}

// The arrays of the layout, one list per device buffer (in the order of LayoutTables::buf), with the room each gets and the
// field of `V` that will point at it: what upload_layout uploads and what the layout export shows, from the same list.
struct LayoutTables {
	enum { INT, TILE, STREAM, BLK, PFAC, PHDR, PAROW, N_BUF };
	std::vector<Part> buf[N_BUF];
};
LayoutTables layout_tables(const ModelLayout &L, HibagModelView &V)
{
	LayoutTables T;
	T.buf[LayoutTables::INT] = {      // the int arrays back to back (an empty one as a single 0)
		part("n_snp_c", V.n_snp_c, L.n_snp_c, 4, 1), part("nwp", V.nwp, L.nwp, 4, 1), part("snp_off", V.snp_off, L.snp_off, 4, 1),
		part("snp_index", V.snp_index, L.snp_index, 4, 1), part("snp_weight", V.snp_weight, L.snp_weight, 4, 1), part("mask_row", V.mask_row, L.mask_row, 4, 1),
		part("c_order", V.c_order, L.c_order, 4, 1), part("tile_p0", V.tile_p0, L.tile_p0, 4, 1), part("tile_n", V.tile_n, L.tile_n, 4, 1), part("cls_off", V.cls_off, L.cls_off, 4, 1),
		part("cls_n", V.cls_n, L.cls_n, 4, 1), part("engine", V.engine, L.engine, 4, 1), part("n_step", V.n_step, L.n_step, 4, 1), part("bt_row", V.bt_row, L.bt_row, 4, 1),
		part("cls_nblk", V.cls_nblk, L.cls_nblk, 4, 1), part("hap_off", V.hap_off, L.hap_off, 4, 1), part("item_split", V.item_split, L.item, 4, 1), part("split_row", V.split_row, L.split_row, 4, 1),
		part("split_cls", V.split_cls, L.split_cls, 4, 1), part("item_whole", V.item_whole, L.item_whole, 4, 1), part("cell_row", V.cell_row, L.cell_row, 4, 1),
		part("wide_cls", V.wide_cls, L.wide_cls, 4, 1), part("wide_seg", V.wide_seg, L.wseg, 4, 1), part("wide_scan", V.wide_scan, L.wide_scan, 4, 1)};
	T.buf[LayoutTables::TILE] = {     // the tables of the pass-1 walkers and of pass 2, at the alignment of their loads
		part("stream_off", V.stream_off, L.stream_off, 8), part("tile_meta", V.tile_meta, L.tile_meta, 4), part("cls_cnt", V.cls_cnt, L.cls_cnt, 4),
		part("cls_cell", V.cls_cell, L.cls_cell, 4), part("blk_off", V.blk_off, L.blk_off, 8), part("ctile", V.ctile, L.ctile, 32), part("hap", V.hap, L.hap, 16),
		part("ehdr", V.ehdr, L.ehdr, 32), part("etile_cstart", V.etile_cstart, L.etile_cstart, 4, 1), part("etile_blk0", V.etile_blk0, L.etile_blk0, 8),
		part("blk_close", V.blk_close, L.blk_close, 4), part("wide_seg_off", V.wide_seg_off, L.wseg_off, 8, 1)};
	T.buf[LayoutTables::STREAM] = {part("stream", V.stream, L.stream, 4)};
	T.buf[LayoutTables::BLK] = {part("plist", V.plist, L.plist, 4)};
	T.buf[LayoutTables::PFAC] = {part("pfac", V.pfac, L.pfac, 8)};
	T.buf[LayoutTables::PHDR] = {part("phdr", V.phdr, L.phdr, 4)};
	T.buf[LayoutTables::PAROW] = {{"parow", L.parow.data(), L.parow.size() * 4, std::max<size_t>(L.parow.size(), 256) * 4, 16, 4, &V.parow}};
	return T;
}

// The scalars of the layout: those of `V`, and those the model keeps beside its view.
struct LayoutScalars {
	uint32_t spin_limit = 0;
	int64_t pair_evals = 0, second_pass_pairs = 0;
	int store_mode = 0, cell_rows = 0, bt_rows = 0, mask_rows = 0;
	size_t stream_bytes = 0;
	std::vector<int> engine_of, steps_of;
};
void layout_scalars(const ModelLayout &L, HibagModelView &V, LayoutScalars &s)
{
	V.n_hla = L.nh; V.n_classifier = L.C; V.n_snp = L.S; V.n_cell = L.P; V.mask_rows = L.rows; V.n_tile = L.n_tile;
	V.n_item_split = (int)L.item.size() / 4; V.n_item_whole = (int)L.item_whole.size() / 4; V.n_split = (int)L.split_cls.size();
	V.n_item = V.n_item_whole;
	V.all_fp4 = 1; V.n_valu = 0;
	for (int c = 0; c < L.C; c++) {
		if (L.n_step[c] == 1 && !(L.engine[c] == HIBAG_ENGINE_FP4)) V.all_fp4 = 0;      // (classifiers of several K steps are not work items of k_total)
		V.n_valu += L.engine[c] == HIBAG_ENGINE_VALU;
	}
	V.n_wide = (int)L.wide_cls.size();
	V.n_wide_scan = (int)L.wide_scan.size();
	V.n_wide_seg = (int)L.wseg.size() / 4;
	V.split_heavy_ns = L.split_heavy_ns; V.split_rest_ns = L.split_rest_ns;
	V.hap_dwords = (uint32_t)L.hap.size();
	V.estream_blocks = L.estream_blocks;
	V.p1_base = L.p1_base;
	V.p1_blocks = L.p1_blocks;
	V.store_cells = L.store_mode;
	V.plist_dwords = L.plist.size();
	V.parow_blocks = L.parow_blocks;
	V.p1_prebuilt = L.p1_prebuilt ? 1 : 0;
	// A chunk waits for the chunk before it, which was dispatched a whole round earlier; in the worst case the chunks of
	// an item run one after the other, so the wait is bounded by the item's own length.  One poll lasts ~1 us (s_sleep +
	// an L2 round trip), a 32-slot block ~1.5 us of elapsed time at full occupancy: 16 polls per block of the longest
	// item is an order of magnitude of slack on top of the fixed 2^19 (~0.5 s).
	long long longest = 0;
	for (int c = 0; c < L.C; c++) longest = std::max<long long>(longest, L.engine[c] ? L.cls_nblk[c] : L.cp[c].pairs / 8);
	s.spin_limit = (uint32_t)std::min<long long>(0xFFFFFFF0ll, (1ll << 19) + 16 * longest);
	s.pair_evals = L.pair_evals;
	s.store_mode = L.store_mode;
	s.second_pass_pairs = L.second_pass_pairs;
	s.cell_rows = L.cell_row[L.C];
	s.bt_rows = L.bt_rows;
	s.mask_rows = L.rows;
	s.stream_bytes = L.stream.size() * sizeof(uint32_t);
	s.engine_of.assign(L.engine.begin(), L.engine.begin() + L.C);
	s.steps_of.assign(L.n_step.begin(), L.n_step.begin() + L.C);
}

// Lays `parts` out back to back in `buf` at their alignments, copies them (several: in one host image) and points their fields.
int upload_parts(DevBuf &buf, const std::vector<Part> &parts)
{
	std::vector<size_t> at;
	size_t end = 0;
	for (const Part &p : parts) { at.push_back((end + p.align - 1) / p.align * p.align); end = at.back() + p.room; }
	if (int rc = buf.reserve(end)) return rc;
	const Part *p = parts.data();
	if (parts.size() == 1 && p->bytes) HIP_TRY(hipMemcpy(buf.p, p->src, p->bytes, hipMemcpyHostToDevice));     // (big arrays: no staging)
	else if (parts.size() > 1) {
		std::vector<char> img(end, 0);
		for (size_t i = 0; i < parts.size(); i++) if (p[i].bytes) memcpy(&img[at[i]], p[i].src, p[i].bytes);
		HIP_TRY(hipMemcpy(buf.p, img.data(), end, hipMemcpyHostToDevice));
	}
	for (size_t i = 0; i < parts.size(); i++) { const char *d = buf.as<char>() + at[i]; memcpy(p[i].field, &d, sizeof d); }
	return 0;
}

// Reserves the device buffers, uploads the layout, points m->view at it and sets the model's scalars (and its side stream).
int upload_layout(hibag_hip_model *m, const ModelLayout &L)
{
	HIP_TRY(hipSetDevice(m->device));
	HibagModelView &V = m->view;
	const LayoutTables T = layout_tables(L, V);
	DevBuf *const bufs[LayoutTables::N_BUF] = {&m->d_int, &m->d_tile, &m->d_stream, &m->d_blk, &m->d_pfac, &m->d_phdr, &m->d_parow};
	for (int i = 0; i < LayoutTables::N_BUF; i++)
		if (int rc = upload_parts(*bufs[i], T.buf[i])) return rc;
	if (int rc = upload_parts(m->d_tab, {{"tab", m->tab, sizeof(m->tab), sizeof(m->tab), 8, 8, &V.tab}})) return rc;
	LayoutScalars s;
	layout_scalars(L, V, s);
	V.item = V.item_whole;
	if (V.n_wide > 0 && !m->side.stream) {
		HIP_TRY(hipStreamCreateWithFlags(&m->side.stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&m->side.fork, hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&m->side.join, hipEventDisableTiming));
	}
	hibag_query_slots(V.slots_total, &V.slots_accum);
	for (int i = 0; i < 4; i++) m->slots_queried[i] = V.slots_total[i];
	m->slots_queried[4] = V.slots_accum;
	m->test_slots[0] = m->test_slots[1] = m->test_tail_k = 0;     // (the tests' chunking hook is set on a finalized model)
	m->spin_limit = s.spin_limit;
	m->pair_evals = s.pair_evals;
	m->store_mode = s.store_mode;
	m->second_pass_pairs = s.second_pass_pairs;
	m->cell_rows = s.cell_rows;
	m->bt_rows = s.bt_rows;
	m->mask_rows = s.mask_rows;
	m->stream_bytes = s.stream_bytes;
	m->engine_of = s.engine_of;
	m->steps_of = s.steps_of;
	m->finalized = true;
	return 0;
}

// The planning stages in order: fills `L` from the model without a HIP call; any of them may reject the model.
int plan_layout(const hibag_hip_model *m, const FinalizeOptions &opt, ModelLayout &L)
{
	if (int rc = plan_classifiers(m, opt, L)) return rc;
	plan_tiles(L);
	plan_store(opt, L);
	if (int rc = plan_cell_lists(L)) return rc;
	plan_work_items(L);
	if (int rc = plan_pair_lists(m, L)) return rc;
	plan_factors(m, L);
	plan_parow(opt, L);
	return plan_ctile(L);
}

// The plan (before anything is allocated), then the upload.
static int finalize_with(hibag_hip_model *m, const FinalizeOptions &opt)
{
	if (m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model already finalized");
	ModelLayout L(m);
	if (int rc = plan_layout(m, opt, L)) return rc;
	return upload_layout(m, L);
}

int finalize_model(hibag_hip_model *m) { return finalize_with(m, FinalizeOptions()); }

int finalize_model_stream(hibag_hip_model *m)
{
	FinalizeOptions opt;
	opt.pass2 = FinalizeOptions::STREAM;
	return finalize_with(m, opt);
}

} // namespace hibag_detail

// What plan_layout makes of the model, as upload_layout would hand it to the device: the arrays of layout_tables with the
// room each is given, and the scalars of layout_scalars (hibag_hip_test_layout_*).
struct hibag_hip_layout {
	ModelLayout L;
	HibagModelView V{};
	LayoutScalars s;
	struct Entry { std::string name; const void *data; uint64_t bytes; int elem; };
	std::vector<Entry> entries;
	std::vector<int64_t> ints;           // the integer scalars, one array of one element each
	std::vector<double> dbls;
	explicit hibag_hip_layout(const hibag_hip_model *m) : L(m) {}
};

// ===========================================================================
// C ABI: the model

extern "C" {

hibag_hip_model *hibag_hip_model_new(int n_hla, int n_snp)
{
	if (n_hla <= 0 || n_hla > 46340 || n_snp < 0) {
		hibag_fail(HIBAG_HIP_EINVAL, "invalid model dimensions (n_hla=%d, n_snp=%d)", n_hla, n_snp);
		return nullptr;
	}
	hibag_hip_model *m = new (std::nothrow) hibag_hip_model;
	if (!m) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	m->device = hibag_selected_device();
	const char *engine = getenv("HIBAG_ENGINE");         // "valu": bit logic + popcount on the vector ALU for every classifier
	m->use_mfma = !(engine && strcmp(engine, "valu") == 0);
	m->use_fp4 = !(engine && strcmp(engine, "i8") == 0);
	m->n_hla = n_hla;
	m->n_snp = n_snp;
	build_table(m->tab);
	// every entry from d = 65 on must be the exact zero IEEE arithmetic makes of exp(65 log 1e-5) = 1e-325 -- a libm that
	// returned a denormal there would be a different table from the reference's
	for (int i = 65; i < HIBAG_TAB_N; i++)
		if (m->tab[i] != 0.0) {
			delete m;
			hibag_fail(HIBAG_HIP_ESTATE, "this libm's exp() does not underflow to zero at exp(%d * log(1e-5)): the mutation table differs from the reference's", i);
			return nullptr;
		}
	return m;
}

int hibag_hip_model_add_classifier(hibag_hip_model *m, int n_snp_c, const int32_t *snpidx,
	int n_haplo, const double *freq, const int32_t *hla, const char *const *haplo)
{
	if (int rc = check_classifier_args(m, n_snp_c, snpidx, n_haplo, freq, hla)) return rc;
	if (n_snp_c > 0 && !snpidx) return hibag_fail(HIBAG_HIP_EINVAL, "snpidx is NULL");
	if (n_haplo > 0 && !haplo) return hibag_fail(HIBAG_HIP_EINVAL, "haplo is NULL");
	std::vector<uint64_t> bits((size_t)n_haplo * 2, 0);
	for (int i = 0; i < n_haplo; i++) {
		const char *s = haplo[i];
		const size_t len = s ? strlen(s) : 0;
		if (len > HIBAG_HIP_MAX_SNP_IN_CLASSIFIER)   // src/LibHLA.cpp:328-329
			return hibag_fail(HIBAG_HIP_EINVAL, "THaplotype::StrToHaplo, the input string is too long.");
		if ((int)len != n_snp_c)
			return hibag_fail(HIBAG_HIP_EINVAL, "haplotype %d has %zu alleles, expected %d", i, len, n_snp_c);
		for (size_t j = 0; j < len; j++) {
			if (s[j] == '1') bits[2 * (size_t)i + (j >> 6)] |= (uint64_t)1 << (j & 63);
			else if (s[j] != '0')                    // src/LibHLA.cpp:333-334
				return hibag_fail(HIBAG_HIP_EINVAL, "THaplotype::StrToHaplo, the input string should be '0' or '1'");
		}
	}
	push_classifier(m, n_snp_c, snpidx, n_haplo, freq, hla, std::move(bits));
	return 0;
}

int hibag_hip_model_add_classifier_packed(hibag_hip_model *m, int n_snp_c, const int32_t *snpidx,
	int n_haplo, const double *freq, const int32_t *hla, const uint64_t *bits_in)
{
	if (int rc = check_classifier_args(m, n_snp_c, snpidx, n_haplo, freq, hla)) return rc;
	if (n_haplo > 0 && !bits_in) return hibag_fail(HIBAG_HIP_EINVAL, "bits is NULL");
	// clear bits >= n_snp_c: the reference leaves them uninitialised (src/LibHLA.cpp:287-292)
	uint64_t mask[2];
	for (int w = 0; w < 2; w++) {
		const int lo = 64 * w;
		mask[w] = n_snp_c >= lo + 64 ? ~(uint64_t)0 : (n_snp_c <= lo ? 0 : (((uint64_t)1 << (n_snp_c - lo)) - 1));
	}
	std::vector<uint64_t> bits((size_t)n_haplo * 2);
	for (int i = 0; i < n_haplo; i++)
		for (int w = 0; w < 2; w++) bits[2 * (size_t)i + w] = bits_in[2 * (size_t)i + w] & mask[w];
	push_classifier(m, n_snp_c, snpidx, n_haplo, freq, hla, std::move(bits));
	return 0;
}

int hibag_hip_model_set_snp_weights(hibag_hip_model *m, const int32_t *snp_weight)
{
	if (!m || !snp_weight) return hibag_fail(HIBAG_HIP_EINVAL, "NULL argument");
	if (m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model already finalized");
	m->snp_weight_override.assign(snp_weight, snp_weight + std::max(m->n_snp, 1));
	return 0;
}

int hibag_hip_model_finalize(hibag_hip_model *m)
{
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	std::lock_guard<std::mutex> g(m->lock);
	return finalize_model(m);
}

void hibag_hip_model_free(hibag_hip_model *m) { delete m; }

int hibag_hip_model_device(const hibag_hip_model *m) { return m ? m->device : -1; }
int hibag_hip_model_n_hla(const hibag_hip_model *m) { return m ? m->n_hla : 0; }
int hibag_hip_model_n_snp(const hibag_hip_model *m) { return m ? m->n_snp : 0; }
int hibag_hip_model_n_classifier(const hibag_hip_model *m) { return m ? (int)m->cls.size() : 0; }

int64_t hibag_hip_model_pair_evals(const hibag_hip_model *m)
{
	if (!m) return 0;
	int64_t n = 0;
	for (const auto &c : m->cls) n += (int64_t)c.freq.size() * ((int64_t)c.freq.size() + 1) / 2;
	return n;
}

int64_t hibag_hip_model_stored_cells(const hibag_hip_model *m)
{
	return m && m->finalized && m->store_mode ? (int64_t)m->cell_rows : 0;
}

int64_t hibag_hip_model_second_pass_pairs(const hibag_hip_model *m)
{
	return m && m->finalized ? m->second_pass_pairs : 0;
}

int hibag_hip_model_mutation_table(const hibag_hip_model *m, double *out)
{
	if (!m || !out) return hibag_fail(HIBAG_HIP_EINVAL, "NULL argument");
	memcpy(out, m->tab, sizeof(m->tab));
	return 0;
}

// ---- the planned layout, for the host tests (tests/test_layout_host.py) -------------------------------------------

hibag_hip_layout *hibag_hip_test_layout_plan(hibag_hip_model *m)
{
	if (!m) { hibag_fail(HIBAG_HIP_EINVAL, "model is NULL"); return nullptr; }
	std::lock_guard<std::mutex> g(m->lock);
	if (m->finalized) { hibag_fail(HIBAG_HIP_ESTATE, "model already finalized"); return nullptr; }
	hibag_hip_layout *p = new (std::nothrow) hibag_hip_layout(m);
	if (!p) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	if (plan_layout(m, FinalizeOptions(), p->L)) { delete p; return nullptr; }
	const LayoutTables T = layout_tables(p->L, p->V);
	layout_scalars(p->L, p->V, p->s);
	for (const auto &parts : T.buf)
		for (const Part &q : parts) p->entries.push_back({q.name, q.src, q.bytes, (int)q.elem});
	const ModelLayout &L = p->L;
	const HibagModelView &V = p->V;
	std::vector<std::pair<std::string, int64_t>> iv;
	for (const auto &parts : T.buf)
		for (const Part &q : parts) iv.push_back({std::string("room:") + q.name, (int64_t)q.room});
	for (const auto &kv : std::initializer_list<std::pair<const char *, int64_t>>{
		{"n_hla", V.n_hla}, {"n_classifier", V.n_classifier}, {"n_snp", V.n_snp}, {"n_cell", V.n_cell}, {"mask_rows", V.mask_rows},
		{"n_tile", V.n_tile}, {"n_item_split", V.n_item_split}, {"n_item_whole", V.n_item_whole}, {"n_split", V.n_split},
		{"all_fp4", V.all_fp4}, {"n_valu", V.n_valu}, {"n_wide", V.n_wide}, {"n_wide_scan", V.n_wide_scan}, {"n_wide_seg", V.n_wide_seg},
		{"hap_dwords", V.hap_dwords}, {"estream_blocks", (int64_t)V.estream_blocks}, {"p1_base", (int64_t)V.p1_base},
		{"p1_blocks", V.p1_blocks}, {"store_cells", V.store_cells}, {"plist_dwords", (int64_t)V.plist_dwords},
		{"parow_blocks", (int64_t)V.parow_blocks}, {"p1_prebuilt", V.p1_prebuilt}, {"spin_limit", p->s.spin_limit},
		{"pair_evals", p->s.pair_evals}, {"second_pass_pairs", p->s.second_pass_pairs}, {"cell_rows", p->s.cell_rows},
		{"bt_rows", p->s.bt_rows}, {"bt_rows_alloc", hibag_bt_rows_alloc(p->s.bt_rows)}, {"stream_bytes", (int64_t)p->s.stream_bytes},
		{"tile", HIBAG_TILE}, {"stored_per_visit", HIBAG_STORED_PER_VISIT}, {"use_mfma", m->use_mfma}, {"use_fp4", m->use_fp4}})
		iv.push_back({kv.first, kv.second});
	p->ints.reserve(iv.size());
	for (const auto &kv : iv) { p->ints.push_back(kv.second); p->entries.push_back({kv.first, &p->ints.back(), 8, 8}); }
	p->dbls = {L.split_heavy_ns, L.split_rest_ns};
	p->entries.push_back({"split_heavy_ns", &p->dbls[0], 8, 8});
	p->entries.push_back({"split_rest_ns", &p->dbls[1], 8, 8});
	return p;
}

int hibag_hip_test_layout_count(const hibag_hip_layout *p) { return p ? (int)p->entries.size() : 0; }

int hibag_hip_test_layout_get(const hibag_hip_layout *p, int index, const char **name, const void **data, uint64_t *bytes, int *elem_size)
{
	if (!p || index < 0 || index >= (int)p->entries.size()) return hibag_fail(HIBAG_HIP_EINVAL, "no such layout entry");
	const auto &e = p->entries[index];
	if (name) *name = e.name.c_str();
	if (data) *data = e.data;
	if (bytes) *bytes = e.bytes;
	if (elem_size) *elem_size = e.elem;
	return 0;
}

void hibag_hip_test_layout_free(hibag_hip_layout *p) { delete p; }

// ---- several devices ------------------------------------------------------------------------------------

hibag_hip_model *hibag_hip_model_replicate(const hibag_hip_model *src, int device)
{
	if (!src) { hibag_fail(HIBAG_HIP_EINVAL, "model is NULL"); return nullptr; }
	const int n = hibag_hip_device_count();
	if (device < 0 || device >= n) { hibag_fail(HIBAG_HIP_ENODEV, "HIP device %d not available (%d visible)", device, n); return nullptr; }
	hibag_hip_model *m = new (std::nothrow) hibag_hip_model;
	if (!m) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	m->device = device;
	m->n_hla = src->n_hla; m->n_snp = src->n_snp;
	m->have_snpidx = src->have_snpidx; m->use_mfma = src->use_mfma; m->use_fp4 = src->use_fp4;
	m->cls = src->cls;
	m->snp_weight_override = src->snp_weight_override;
	memcpy(m->tab, src->tab, sizeof(m->tab));
	if (src->finalized && hibag_hip_model_finalize(m)) { delete m; return nullptr; }
	return m;
}

// A shard of a model for classifier-sharded prediction (hibag_shard.hip): classifiers [first, first + count) of `src`, order
// kept, with the FULL model's per-SNP classifier counts (_GetSNPWeights, src/LibHLA.cpp:2484-2496), on `device`.
hibag_hip_model *hibag_hip_model_shard(const hibag_hip_model *src, int shard, int n_shards, int device)
{
	if (!src) { hibag_fail(HIBAG_HIP_EINVAL, "model is NULL"); return nullptr; }
	int first = 0, count = 0;
	if (hibag_hip_shard_bounds((int)src->cls.size(), n_shards, shard, &first, &count)) return nullptr;
	const int n = hibag_hip_device_count();
	if (device < 0 || device >= n) { hibag_fail(HIBAG_HIP_ENODEV, "HIP device %d not available (%d visible)", device, n); return nullptr; }
	hibag_hip_model *m = new (std::nothrow) hibag_hip_model;
	if (!m) { hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	try {
		m->device = device;
		m->n_hla = src->n_hla; m->n_snp = src->n_snp;
		m->have_snpidx = src->have_snpidx; m->use_mfma = src->use_mfma; m->use_fp4 = src->use_fp4;
		m->cls.assign(src->cls.begin() + first, src->cls.begin() + first + count);
		if (!src->snp_weight_override.empty()) m->snp_weight_override = src->snp_weight_override;     // (a shard of a shard keeps the full model's counts)
		else {
			m->snp_weight_override.assign(std::max(src->n_snp, 1), 0);
			for (const HostClassifier &k : src->cls)
				for (int v : k.snpidx) m->snp_weight_override[v]++;
		}
		memcpy(m->tab, src->tab, sizeof(m->tab));
	} catch (...) { delete m; hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); return nullptr; }
	if (src->finalized && hibag_hip_model_finalize(m)) { delete m; return nullptr; }
	return m;
}

int hibag_hip_model_engine(const hibag_hip_model *m, int classifier, int *engine, int *k_steps)
{
	if (!m || !m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model not finalized");
	if (classifier < 0 || classifier >= (int)m->cls.size()) return hibag_fail(HIBAG_HIP_EINVAL, "classifier %d out of range", classifier);
	if (engine) *engine = m->engine_of[classifier];
	if (k_steps) *k_steps = m->steps_of[classifier];
	return 0;
}

} // extern "C"
