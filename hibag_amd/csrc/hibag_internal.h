// hibag_internal.h -- what the host-side translation units of libhibag_hip.so share: the model container behind the opaque
// `hibag_hip_model` of include/hibag_hip.h, its device / pinned buffers, the per-kernel timers, the types that carry a
// prediction call through the drivers -- PredictOut (what to return), GenoSource / PackSource (where the genotypes come
// from), WorkspaceGuard, with_handover_repair (the repair of a failed hand-over) -- and the few functions that cross the files:
//   hibag_api.hip      error state, device selection, kernel target, the plugin table
//   hibag_model.hip    the model: classifiers in, the device layout out (hibag_hip_model_new ... _finalize, replicas, shards)
//   hibag_predict.hip  the batch driver that replaces CAttrBag_Model::PredictHLA: workspace, kernel sequence (enqueue_pack,
//                      run_core), the host-pointer pipeline (predict_staged_locked), the SNP map upload, BED input, partial
//                      sums, launch status, timing
//   hibag_whole.hip    the entries that take a small cohort through the device in ONE call: their frame (WholeCall), the
//                      batch knobs, the SNP-users index, the out-of-bag and masked drivers with their entries
//   hibag_finish.hip   what depends on the finish a call runs (ListOut::kind): its argument check, the call's state on the
//                      device, its workspace, its launch
//   hibag_prefix.hip   hibag_hip_predict_prefix: every sub-model "first k classifiers" from one pass 1
//   hibag_merge.hip    hibag_hip_predict_merge: k models' predictions and their merge on one stream
//   hibag_cohort.hip   a cohort's genotypes resident on a device in 2-bit form, and the prediction entries that read them
//   hibag_groups.hip   the plan of the group entries (hibag_hip_predict_groups*): the caller's partitions in list form
//   hibag_knock.hip    hibag_hip_oob_knock: the out-of-bag SNP knock-out tallies in one call on the model's workspace
#ifndef HIBAG_INTERNAL_H_
#define HIBAG_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hibag_hip.h"
#include "hibag_device.h"
#include "hibag_kernels.h"
#include "hibag_plugin.h"

// records the calling thread's last error (hibag_hip_last_error) and returns `code` (hibag_api.hip)
int hibag_fail(int code, const char *fmt, ...);
int hibag_selected_device();                 // the calling thread's hibag_hip_set_device() choice

#define HIP_TRY(expr)                                                                         \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if (e_ != hipSuccess)                                                                 \
			return hibag_fail(e_ == hipErrorOutOfMemory ? HIBAG_HIP_ENOMEM : HIBAG_HIP_ENODEV, \
				"%s failed: %s", #expr, hipGetErrorString(e_));                               \
	} while (0)

namespace hibag_detail {

// Grow-only pinned host buffer (staging of the pipelined host-pointer entries).
struct PinBuf {
	void *p = nullptr;
	size_t cap = 0;
	int reserve(size_t bytes);
	void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// Grow-only device buffer.
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	int reserve(size_t bytes)
	{
		if (bytes <= cap) return 0;
		if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
		HIP_TRY(hipMalloc(&p, bytes));
		cap = bytes;
		return 0;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
	template <class T> T *as() const { return (T *)p; }
};

inline int PinBuf::reserve(size_t bytes)
{
	if (bytes <= cap) return 0;
	release();
	HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
	cap = bytes;
	return 0;
}

struct HostClassifier {
	std::vector<int> snpidx;         // may be empty for plugin-built models
	int n_snp = 0;
	std::vector<uint64_t> bits;      // [H][2], bits >= n_snp cleared
	std::vector<double> freq;
	std::vector<int> hla;
};

struct KernelTimer {
	struct Pending { int k; hipEvent_t a, b; bool a_shared; };
	bool enabled = false;
	unsigned mask = 0xf;               // kernel classes that get events (bit k); the others run unobserved
	bool open = false;                 // begin() recorded something that end() has to close
	bool chainable = false;            // the last timer operation was an end() that recorded an event ...
	hipStream_t chain_stream = nullptr; // ... on this stream
	std::vector<Pending> pending;
	std::vector<hipEvent_t> pool;
	double ms[HIBAG_HIP_K_COUNT] = {0, 0, 0, 0};
	int64_t n[HIBAG_HIP_K_COUNT] = {0, 0, 0, 0};

	hipEvent_t get()
	{
		if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
		hipEvent_t e;
		(void)hipEventCreate(&e);
		return e;
	}
	// `chain`: the caller has enqueued nothing on `st` since the end() before -- that end's event is this begin's too
	// (an event record is a barrier packet of its own on the queue: five per batch instead of eight).
	void begin(int k, hipStream_t st, bool chain = false)
	{
		open = false;
		if (!enabled || !((mask >> k) & 1u)) { chainable = false; return; }
		Pending p;
		p.k = k;
		p.a_shared = chain && chainable && chain_stream == st && !pending.empty();
		p.a = p.a_shared ? pending.back().b : get();
		p.b = get();
		if (!p.a_shared) (void)hipEventRecord(p.a, st);
		pending.push_back(p);
		open = true;
		chainable = false;
	}
	void end(hipStream_t st)
	{
		if (!open) return;
		(void)hipEventRecord(pending.back().b, st);
		open = false;
		chainable = true;
		chain_stream = st;
	}
	void resolve()
	{
		for (auto &p : pending) {
			(void)hipEventSynchronize(p.b);
			float t = 0;
			if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) { ms[p.k] += t; n[p.k]++; }
		}
		for (auto &p : pending) {
			if (!p.a_shared) pool.push_back(p.a);
			pool.push_back(p.b);
		}
		pending.clear();
		chainable = false;
		open = false;
	}
	void reset()
	{
		resolve();
		for (int k = 0; k < HIBAG_HIP_K_COUNT; k++) { ms[k] = 0; n[k] = 0; }
	}
	void destroy()
	{
		resolve();
		for (auto e : pool) (void)hipEventDestroy(e);
		pool.clear();
	}
};

// streams and events of the host-pointer entries' slice pipeline (predict_staged_locked)
struct StagedStreams { hipStream_t run = nullptr, in = nullptr, out = nullptr; hipEvent_t up[2] = {}, ran[2] = {}, down[2] = {}; };


inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// rows of HibagBatchView::bt for a model of `bt_rows` operand rows: the model's and two spare (what pass 2 requests for a
// block of a classifier without rows of its own)
inline int hibag_bt_rows_alloc(int bt_rows) { return std::max(bt_rows, 1) + 2; }

} // namespace hibag_detail
using namespace hibag_detail;

struct hibag_hip_model {
	int device = 0;
	int n_hla = 0, n_snp = 0;
	bool finalized = false;
	bool have_snpidx = true;
	bool use_mfma = true;                  // matrix-core engine for classifiers with <= 112 SNPs (HIBAG_ENGINE=valu disables)
	bool use_fp4 = true;                   // its FP4 form for <= 30 SNPs (HIBAG_ENGINE=i8 keeps every classifier on the int8 form)
	std::vector<HostClassifier> cls;
	std::vector<int> snp_weight_override;   // classifier-sharded runs
	int64_t pair_evals = 0;
	double tab[HIBAG_TAB_N];

	// device model
	DevBuf d_int, d_stream, d_tile, d_tab, d_blk, d_pfac, d_phdr, d_parow;
	HibagModelView view{};
	int mask_rows = 0, bt_rows = 0, cell_rows = 0;
	size_t stream_bytes = 0;

	// per-batch workspace (grow-only)
	DevBuf ws_planes, ws_cw, ws_tot, ws_inv, ws_winv, ws_part, ws_best, ws_vrec, ws_geno, ws_out, ws_codes, ws_bt, ws_bias, ws_cells, ws_sync;
	// the whole-call entries (WholeCall below): a call's inputs beside the genotypes, and what only its own kernels read
	// and write; their outputs share ws_out
	DevBuf ws_in, ws_scratch;
	// the given entries (hibag_hip_predict_given*): a host-pointer call's constraint on the device, sample-major as the caller
	// gave it, and a batch's masks as k_finish_given reads them ([2 W][n_pad])
	DevBuf ws_allow, ws_masks;
	// the family entries (hibag_hip_predict_family*): the call's pedigree, depths and prior as uploaded (ws_fam_in), every
	// finished sample's joint dosage and support ([n_call][n_hla] then [n_call]: what the samples' children read, rebuilt by
	// every run), and a batch's ratio vectors as k_finish_family reads them ([2 n_hla][n_pad])
	DevBuf ws_fam_in, ws_family, ws_ratios;
	std::vector<int32_t> fam_depth;        // the call's depths on the host [n_call]: the rounds of every batch are read off them
	std::vector<int> engine_of, steps_of;  // per classifier: HIBAG_HIP_ENGINE_* and K steps, as finalized
	int store_mode = 0;                    // which cell sums pass 1 stores for pass 2 (HibagModelView::store_cells)
	int64_t second_pass_pairs = 0;         // haplotype pairs per sample pass 2 evaluates again
	HibagSideStream side;                  // second stream for pass 1 of the classifiers with several K steps (created at finalize if any)
	uint32_t epoch = 0;                    // batch counter for the hand-over flags (HibagBatchView::epoch)
	int *h_err = nullptr;                  // host-mapped error word of the hand-overs
	DevBuf ws_err;                         // its device twin: epoch of the last batch with a failed hand-over (HibagBatchView::err_dev)
	// A failed hand-over: `fault` is sticky until hibag_hip_model_clear_status(); from the first one on
	// the model launches without hand-overs (`no_chunks`: every work item undivided -- nothing left that could fail).
	int fault = 0;
	int64_t fault_count = 0;
	bool no_chunks = false;
	int drop_next = 0;                     // fault injection (hibag_hip_test_inject_handover_fault): pass whose first hand-over the next batch drops
	// The chunking hook of the tests (hibag_hip_test_set_chunking): the resident-workgroup figures as the device reported them
	// (view.slots_* hold min(queried, asked) while the hook is set), what the hook asked for (0 = nothing), and what the most
	// recent passes 1 and 2 of run_core launched (hibag_hip_test_last_launch)
	int slots_queried[5] = {0, 0, 0, 0, 0};  // slots_total[0..3], slots_accum
	int test_slots[2] = {0, 0}, test_tail_k = 0;
	HibagLaunchTotal last_total;
	HibagLaunchAccum last_accum;
	int n_launch_total = 0, n_launch_accum = 0;
	uint32_t spin_limit = 1u << 19;       // polls a waiting workgroup makes before it gives up (set at finalize from the longest item)
	// The workspace is one per model: calls on different streams are chained on the device through this event, each
	// waits for the one enqueued before it.
	hipEvent_t ws_done = nullptr;
	bool ws_pending = false;
	StagedStreams staged;                  // the host-pointer entries' slice pipeline (created on first use)
	PinBuf pin_geno, pin_out;              // its pinned staging buffers (two slices each)
	bool staged_ready = false;
	// PLINK BED payload + SNP map of hibag_hip_predict_bed
	DevBuf ws_bed, ws_bedidx;
	// hibag_hip_predict_oob: the plain haplotype table its rescan reads (built at the first call) -- bits, frequencies,
	// per-classifier offsets and allele starts, at the byte offsets below
	DevBuf oob_hap;
	size_t oob_freq_at = 0, oob_off_at = 0, oob_start_at = 0;
	bool oob_hap_ready = false;
	// hibag_hip_model_distance (hibag_dist.hip): its own stream, workspace and timing events; it reads oob_hap, which it
	// builds itself on a model that was never finalized (adding a classifier drops the table again)
	hipStream_t dist_st = nullptr;
	hipEvent_t dist_ev[2] = {nullptr, nullptr};
	DevBuf dist_cells, dist_tri, dist_acc, dist_num, dist_out;
	double dist_ms = 0;
	// hibag_hip_predict_prefix (hibag_prefix.hip): the second layout of this model, finalized with every cell sum stored
	// (built at the first call on a model whose own layout is not store mode 1, never touched by the other entries; the
	// call runs on that layout's workspace)
	hibag_hip_model *prefix_layout = nullptr;
	double pfx_accum_ms = 0;
	// hibag_hip_predict_masked, hibag_hip_oob_knock: the inverted index SNP -> (classifier, variant) (snp_users_index; CSR:
	// n_snp + 1 offsets, the classifiers, the variants; built at the first call, with the offsets' host twin)
	DevBuf snp_users;
	std::vector<int> snp_users_off;        // [n_snp + 1]
	bool snp_users_ready = false;

	KernelTimer timer;
	std::mutex lock;

	~hibag_hip_model()
	{
		(void)hipSetDevice(device);
		timer.destroy();
		if (h_err) (void)hipHostFree(h_err);
		if (ws_done) (void)hipEventDestroy(ws_done);
		pin_geno.release(); pin_out.release();
		for (hipStream_t st : {staged.run, staged.in, staged.out}) if (st) (void)hipStreamDestroy(st);
		for (int i = 0; i < 2; i++)
			for (hipEvent_t e : {staged.up[i], staged.ran[i], staged.down[i]}) if (e) (void)hipEventDestroy(e);
		if (side.fork) (void)hipEventDestroy(side.fork);
		if (side.join) (void)hipEventDestroy(side.join);
		if (side.stream) (void)hipStreamDestroy(side.stream);
		if (dist_st) (void)hipStreamDestroy(dist_st);
		for (hipEvent_t e : dist_ev) if (e) (void)hipEventDestroy(e);
		for (DevBuf *b : {&d_int, &d_stream, &d_tile, &d_tab, &d_blk, &d_pfac, &d_phdr, &d_parow, &ws_bt, &ws_bias, &ws_cells, &ws_sync, &ws_err, &ws_planes, &ws_cw, &ws_tot, &ws_inv, &ws_winv,
		                  &ws_part, &ws_best, &ws_vrec, &ws_geno, &ws_out, &ws_in, &ws_scratch, &ws_codes, &ws_allow, &ws_masks, &ws_fam_in, &ws_family, &ws_ratios, &ws_bed, &ws_bedidx, &oob_hap,
		                  &dist_cells, &dist_tri, &dist_acc, &dist_num, &dist_out, &snp_users})
			b->release();
		delete prefix_layout;
	}
};

// The plan of the group entries (include/hibag_hip.h "allele groups"): the caller's partitions of ONE model's alleles as the
// lists k_finish_groups walks, on that model's device (hibag_groups.hip).
struct hibag_hip_groups {
	const hibag_hip_model *model = nullptr;    // whose alleles are partitioned: the entries take the plan with this model only
	int device = 0;
	int n_hla = 0;
	std::vector<int32_t> levels;           // G_q per partition
	DevBuf d_call, d_dose, d_group, d_offset;
	HibagGroupsView view{};
};

namespace hibag_detail {

void build_table(double *tab);                               // hibag_model.hip: exp(d * log(1e-5)), the host libm's
int finalize_model(hibag_hip_model *m);                      // hibag_model.hip
int finalize_model_stream(hibag_hip_model *m);               // hibag_model.hip: the same with FinalizeOptions::STREAM (every cell sum stored), whatever the environment says
int batch_limit(const hibag_hip_model *m);                   // hibag_predict.hip: samples per batch (workspace bound)
int oob_hap_table(hibag_hip_model *m);                       // hibag_whole.hip: m->oob_hap from m->cls (once)

// ---- hibag_predict.hip's batch driver, as far as hibag_merge.hip drives it too ----
// Where a batch's genotypes come from: the int32 matrix, or a PLINK BED payload.
struct PackSource {
	const int32_t *d_geno = nullptr;       // [n_samp][row_len]
	int row_len = 0;                       // SNPs per sample in d_geno (0: the model's n_snp, model order)
	size_t ld = 0;                         // != 0: d_geno is SNP-MAJOR, [rows][ld] with one row of genotypes per SNP (k_codes_rows); d_col = row of each model SNP
	const int32_t *d_col = nullptr;        // [n_snp] column of each model SNP in d_geno (-1 = absent), nullptr = identity
	const uint8_t *d_bed = nullptr;        // payload rows (see k_bed_codes)
	int mode = 0;
	size_t stride = 0;
	int samp0 = 0;                         // BED sample index of the call's sample 0
	const int32_t *d_row = nullptr, *d_flip = nullptr;
};

// Which finish a call runs behind passes 1 and 2.  CALL is PredictHLA's own (the call, the dosage, the posterior matrix); the
// others are the list entries' (include/hibag_hip.h): per sample pairs() pairs and their probabilities, [n_samp][pairs()] each.
//   TOPK    k_finish_topk: the k best pairs
//   DRAW    k_finish_draw: k = n_draw pairs drawn from the posterior, keyed with `seed` and the sample's index
//   GROUPS  k_finish_groups: per partition of `plan` the best pair of groups, and optionally the group dosages
//   GIVEN   k_finish_given: the best pair among the cells consistent with the sample's two allele sets `allow`, a per-sample
//           INPUT that travels with the outputs; `support`, and optionally the restricted allele dosages
//   FAMILY  k_finish_family: the best pair under the posterior weighted by the parents' results; `support` and the dosage as
//           for GIVEN; the pedigree is an input in the CALL's numbering that does not travel with the outputs -- call0 says
//           where in the call the outputs stand
// What the drivers need to know of a kind they ask the methods below and hibag_finish.hip; only the fronts that build an
// output set name one.
enum class Finish { CALL, TOPK, DRAW, GROUPS, GIVEN, FAMILY };

struct ListOut {
	Finish kind = Finish::CALL;
	int k = 0;                             // TOPK, DRAW: the pairs per sample asked for
	int32_t *h1 = nullptr, *h2 = nullptr;  // (GROUPS: group indices)
	double *prob = nullptr;
	uint64_t seed = 0;                     // DRAW: the generator's key ...
	int64_t sample0 = 0;                   // ... and the index, in the caller's numbering, of sample 0 of h1 / h2 / prob
	const hibag_hip_groups *plan = nullptr; // GROUPS: the plan whose lists the finish walks
	double *dosage = nullptr;              // GROUPS, GIVEN, FAMILY: if asked for, [n_samp][levels()]
	int n_hla = 0;                         // GIVEN, FAMILY: the model's alleles
	double *support = nullptr;             // GIVEN, FAMILY: [n_samp]
	const uint32_t *allow = nullptr;       // GIVEN: the samples' sets [n_samp][2][W], where the outputs are (host / device)
	const int32_t *pedigree = nullptr;     // FAMILY: the call's pedigree [n_call][2] (HOST memory on every route) ...
	const double *prior = nullptr;         // ... and allele prior [n_hla] (host memory; null: all 1.0);
	int n_call = 0;                        // the call's samples (set with the call's state, finish_call_state) ...
	size_t call0 = 0;                      // ... of which sample call0 is sample 0 of the outputs

	bool is_list() const { return kind != Finish::CALL; }
	size_t pairs() const                   // per sample
	{
		switch (kind) {
		case Finish::CALL: return 0;
		case Finish::GROUPS: return plan ? (size_t)plan->view.n_part : 0;
		case Finish::GIVEN: case Finish::FAMILY: return 1;
		default: return (size_t)k;
		}
	}
	bool has_support() const { return kind == Finish::GIVEN || kind == Finish::FAMILY; }
	// dosage columns per sample: the plan's groups, the model's alleles
	size_t levels() const { return kind == Finish::GROUPS ? (plan ? (size_t)plan->view.n_level : 0) : has_support() ? (size_t)n_hla : 0; }
	size_t allow_words() const { return kind == Finish::GIVEN ? (size_t)2 * (((size_t)n_hla + 31) / 32) : 0; }      // of one sample
	// inputs in host memory on every route: a device-pointer entry uploads them itself, and so has nothing to do for no samples
	bool host_inputs() const { return kind == Finish::FAMILY; }
	// an unfinalized model is ESTATE to the older entries; the given and the family entries state every rejection as EINVAL
	int unfinalized_code() const { return has_support() ? HIBAG_HIP_EINVAL : HIBAG_HIP_ESTATE; }
};

// What a prediction call returns, the one "outputs" parameter of the drivers: the six per-sample outputs of PredictHLA (any
// may be null: not asked for) or, for the list entries, `list` and `matching` (the others stay null).  Device pointers for
// predict_device_locked, the caller's host arrays for the host-pointer drivers.  (The merge drivers of hibag_merge.hip carry
// their outputs in one too; their matrices are row-major with the samples along a row, so there advanced(s0, 1, 1) applies.)
struct PredictOut {
	int32_t *H1 = nullptr, *H2 = nullptr;
	double *max_prob = nullptr, *matching = nullptr;
	double *dosage = nullptr;              // [n_samp][n_hla]
	double *postprob = nullptr;            // [n_samp][n_cell]
	ListOut list;

	static PredictOut list_of(Finish kind, int k, int32_t *h1, int32_t *h2, double *prob, double *matching)
	{
		PredictOut o;
		o.matching = matching;
		o.list.kind = kind; o.list.k = k; o.list.h1 = h1; o.list.h2 = h2; o.list.prob = prob;
		return o;
	}
	static PredictOut topk(int k, int32_t *h1, int32_t *h2, double *prob, double *matching)
	{
		return list_of(Finish::TOPK, k, h1, h2, prob, matching);
	}
	static PredictOut draw(int n_draw, uint64_t seed, int64_t sample0, int32_t *h1, int32_t *h2, double *prob, double *matching)
	{
		PredictOut o = list_of(Finish::DRAW, n_draw, h1, h2, prob, matching);
		o.list.seed = seed; o.list.sample0 = sample0;
		return o;
	}
	static PredictOut groups(const hibag_hip_groups *plan, int32_t *g1, int32_t *g2, double *prob, double *matching, double *dosage)
	{
		PredictOut o = list_of(Finish::GROUPS, 0, g1, g2, prob, matching);
		o.list.plan = plan; o.list.dosage = dosage;
		return o;
	}
	static PredictOut given_sets(const hibag_hip_model *m, const uint32_t *allow, int32_t *h1, int32_t *h2, double *prob, double *support,
		double *matching, double *dosage)
	{
		PredictOut o = list_of(Finish::GIVEN, 0, h1, h2, prob, matching);
		o.list.n_hla = m ? m->n_hla : 0;
		o.list.allow = allow; o.list.support = support; o.list.dosage = dosage;
		return o;
	}
	// (the same outputs under a pedigree; the samples' depths are the call's state: finish_call_state computes them)
	static PredictOut family(const hibag_hip_model *m, const int32_t *pedigree, const double *prior, int32_t *h1, int32_t *h2, double *prob,
		double *support, double *matching, double *dosage)
	{
		PredictOut o = given_sets(m, nullptr, h1, h2, prob, support, matching, dosage);
		o.list.kind = Finish::FAMILY; o.list.pedigree = pedigree; o.list.prior = prior;
		return o;
	}
	// the set `s0` samples further on (null stays null; a draw is keyed with the sample's index in the caller's numbering)
	PredictOut advanced(size_t s0, size_t n_hla, size_t n_cell) const
	{
		PredictOut o = *this;
		auto adv = [](auto *&p, size_t by) { if (p) p += by; };
		adv(o.H1, s0); adv(o.H2, s0); adv(o.max_prob, s0); adv(o.matching, s0);
		adv(o.dosage, s0 * n_hla); adv(o.postprob, s0 * n_cell);
		adv(o.list.h1, s0 * list.pairs()); adv(o.list.h2, s0 * list.pairs()); adv(o.list.prob, s0 * list.pairs());
		adv(o.list.dosage, s0 * list.levels());
		adv(o.list.support, s0); adv(o.list.allow, s0 * list.allow_words());
		o.list.sample0 += (int64_t)s0; o.list.call0 += s0;
		return o;
	}
};

// A SNP-major host matrix (hibag_hip_predict_snp_major): geno[rows[r] * ld + s] is staged as row r of a slice's
// [rows.size()][n] device matrix -- only the rows the model uses travel.
struct HostRows {
	size_t ld = 0;
	std::vector<size_t> rows;
	bool consecutive = false;              // rows[r] = rows[0] + r: a slice is one strided block of the caller's matrix
};

// Where the genotypes of a host-pointer call come from, the one "source" parameter of predict_staged_locked:
//   a sample-major host matrix   `geno` [n_samp][pack.row_len] (row_len 0: the model's SNPs in model order), with
//                                pack.d_col / d_flip (on the device) if it is the cohort's own matrix
//   SNP-major host rows          `geno` with `rows` (rows.ld != 0), pack.d_col / d_flip as above
//   a payload on the device      `geno` null: `pack` as for hibag_launch_pack_bed (what the BED entries upload per call; the
//                                rows of a resident cohort, hibag_cohort.hip), samples pack.samp0 .. + n_samp
struct GenoSource {
	const int32_t *geno = nullptr;
	HostRows rows;
	PackSource pack;
	bool snp_major() const { return rows.ld != 0; }
};

// Host image of the part of a BED file a call needs.  SNP-major files keep only
// the rows of the wanted SNPs (a cohort file holds the whole genome, a model
// ~10^2-10^3 SNPs); individual-major files are kept whole.
struct BedImage {
	int mode = 0;
	size_t stride = 0;                 // bytes per row
	std::vector<uint8_t> rows;         // payload
	std::vector<int32_t> index;        // per wanted SNP: row (SNP-major) / column (individual-major) in `rows`, -1 = absent
};

int make_batch(hibag_hip_model *m, int n_samp, bool need_best, HibagBatchView &B);      // the model's workspace for one batch
// the pack of batch samples [s0, s0 + B.n_samp) of `src` into m->ws_codes, whichever of the three forms `src` has
void enqueue_pack(hibag_hip_model *m, HibagBatchView &B, const PackSource &src, int s0, hipStream_t st);
void run_core(hibag_hip_model *m, HibagBatchView &B, int vote_method, double *d_part, hipStream_t st);   // passes 1 and 2 behind a pack
// HIBAG_DEBUG_SYNC=1: wait for the stream behind a stage and name it on stderr (which kernel a device fault belongs to)
void debug_stage(const char *what, hipStream_t st);
// (`unfinalized`: the code an unfinalized model gets -- ListOut::unfinalized_code() where the call has an output set)
int check_predict_args(hibag_hip_model *m, const void *geno, int n_samp, int vote_method, const void *H1, const void *H2, int unfinalized = HIBAG_HIP_ESTATE);

// ---- hibag_finish.hip: what depends on the finish a call runs, one switch over ListOut::kind each ----
int check_list_args(const hibag_hip_model *m, int n_samp, const ListOut &list);       // the finish's own arguments, behind check_predict_args
// What a call needs on the device before its first batch, once per run by the call's owner (StagedRun::run,
// predict_device_entry) behind the argument checks: the constraint of a host route up on `up` (`list.allow` becomes the device
// copy), the family entries' depths, pedigree and prior up on `st` (waited for).  `host_route`: the arrays of `list` are the
// caller's host memory; else the call is a device-pointer entry's on the caller's stream `st`, and what goes up is chained
// behind whatever still uses the model's workspace.
int finish_call_state(hibag_hip_model *m, ListOut &list, int n_samp, bool host_route, hipStream_t st, hipStream_t up);
int finish_reserve_batch(hibag_hip_model *m, const ListOut &list, int n_pad);          // the finish's own workspace for batches of up to n_pad samples
// the finish of batch B on its partial sums B.part, with `out` already advanced to the batch's first sample
int finish_launch(hibag_hip_model *m, HibagBatchView &B, const PredictOut &out, hipStream_t st);

bool take_fault(hibag_hip_model *m);                         // a hand-over failed since the last look: counted, hand-overs off
int sticky_fault(hibag_hip_model *m);
int workspace_enter(hibag_hip_model *m, hipStream_t st);
int workspace_leave(hibag_hip_model *m, hipStream_t st);
int staged_streams(hibag_hip_model *m, StagedStreams **out);  // the model's streams of the host-pointer entries (created on first use)
// the SNP map of a call on the model's device (m->ws_bedidx): col[k] (null: k; negative: -1, absent) and flip[k] != 0 of every model SNP
int upload_snp_map(hibag_hip_model *m, const int32_t *col, const int32_t *flip, const int32_t **d_col, const int32_t **d_flip);
// the host-pointer driver: slices, the three-stream pipeline, repair of a failed hand-over
int predict_staged_locked(hibag_hip_model *m, const GenoSource &src, int n_samp, int vote_method, const PredictOut &out);
int load_bed(const char *fn, int n_samp, int n_snp, const int32_t *want, int n_want, BedImage &img);

// Records ws_done when a driver that enqueues on the model's shared workspace returns -- also on its error paths, once
// anything has been enqueued.
struct WorkspaceGuard {
	hibag_hip_model *m = nullptr;
	hipStream_t st = nullptr;
	bool enqueued = false, left = false;
	int leave() { left = true; return workspace_leave(m, st); }
	~WorkspaceGuard() { if (enqueued && !left && m->ws_done) { (void)hipEventRecord(m->ws_done, st); m->ws_pending = true; } }
};

// ---- hibag_whole.hip: a small (training-sized) cohort through the device in ONE call ----
// hibag_hip_predict_oob, hibag_hip_predict_masked, hibag_hip_oob_knock and hibag_hip_predict_prefix upload the genotypes and
// the call's inputs once, run batches on the model's workspace and download the results once.  WholeCall is the frame they
// share; the entries hold m->lock for the whole call, run it under with_handover_repair and end synchronised.

// The layout of one device buffer: take() hands out consecutive 8-byte-aligned blocks (0 bytes for what is not asked for),
// `bytes` is what they need in all, at() a block's address once the buffer is reserved.
struct Arena {
	size_t bytes = 0;
	char *base = nullptr;
	size_t take(size_t n) { const size_t at = bytes; bytes = at + (n + 7) / 8 * 8; return at; }
	template <class T> T *at(size_t off) const { return (T *)(base + off); }
};

// The frame of one whole call on the workspace of `m` (for the prefix entry the layout it runs on).  The driver lays out
// `in` (ws_in: the call's inputs), `out` (ws_out: what goes back to the caller) and `scratch` (ws_scratch: what only the
// call's kernels touch) with take(), then
//   open()            the model's run stream, every reserve, workspace_enter, the armed guard: from here on ws_done is
//                     recorded on every return
//   upload*()         the genotypes into ws_geno (`geno`: where the packs of the batches read them), the inputs into `in`
//   for_each_batch()  make_batch and the driver's launches for `count` samples from `first` on
//   close()           hipGetLastError, the downloads (a null destination: not asked for), the ws_done record, the synchronise
struct WholeCall {
	struct Download { void *dst; const void *src; size_t bytes; };
	hibag_hip_model *m;
	hipStream_t st = nullptr;
	Arena in, out, scratch;
	PackSource geno;                       // the call's genotypes on the device: [n_samp][n_snp] in ws_geno
	size_t geno_bytes = 0;
	WorkspaceGuard guard;

	explicit WholeCall(hibag_hip_model *model) : m(model) {}
	int open(int n_samp);
	int upload(void *dst, const void *src, size_t bytes) { HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); return 0; }
	int upload_geno(const int32_t *host) { return upload(m->ws_geno.p, host, geno_bytes); }
	int download(void *dst, const void *src, size_t bytes) { if (dst) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); return 0; }
	int close(std::initializer_list<Download> downloads);
	// (`lim`: the unit's batch cap -- samples, or for the knock-out the lanes of its 64-lane groups)
	template <class Body> int for_each_batch(size_t total, size_t lim, bool need_best, Body body)
	{
		for (size_t first = 0; first < total; first += lim) {
			const int count = (int)std::min(lim, total - first);
			HibagBatchView B;
			if (int rc = make_batch(m, count, need_best, B)) return rc;
			if (int rc = body(B, first, count)) return rc;
		}
		return 0;
	}
};

// `lim` lowered to the diagnostic knob `env_name` (smaller batches), in whole wavefronts: at least 64
int batch_cap(const char *env_name, int lim);
int oob_force_rescan();                                      // HIBAG_OOB_RESCAN (diagnostic): every pick by the full walk
void oob_hap_view(const hibag_hip_model *m, HibagOobOut &O); // the hap_* and hla_start fields of O from m->oob_hap
int snp_users_index(hibag_hip_model *m);                     // m->snp_users from m->cls (once)

// The repair of a failed hand-over, for every driver whose results go to the caller's host arrays.  A device-pointer launch
// still running on another stream may yet fail a hand-over: it is waited for first, so that its fault becomes the model's
// sticky status (its caller's to see) instead of being taken for this call's own and repaired away.  Then `body` runs -- the
// whole call, final synchronisation included.  If a hand-over failed in it the outputs are poisoned: the body runs once
// more, now without hand-overs (take_fault switched them off), before anything is returned to the caller.
template <class Body>
int with_handover_repair(hibag_hip_model *const *models, int n_models, Body body)
{
	for (int i = 0; i < n_models; i++) {
		hibag_hip_model *m = models[i];
		if (m->ws_pending && m->ws_done) HIP_TRY(hipEventSynchronize(m->ws_done));
		if (int rc = sticky_fault(m)) return rc;
	}
	for (int run = 0; run < 2; run++) {
		if (int rc = body()) return rc;
		bool fault = false;
		for (int i = 0; i < n_models; i++) fault = take_fault(models[i]) || fault;
		if (!fault) return 0;
	}
	return hibag_fail(HIBAG_HIP_EHANDOVER, "a hand-over between workgroups failed in a launch without hand-overs");
}

} // namespace hibag_detail

#endif
