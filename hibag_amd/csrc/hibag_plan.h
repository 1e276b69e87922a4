// hibag_plan.h -- the launch arithmetic of passes 1 and 2 as pure host functions: how many work items a launch has, which
// of them go undivided, which in K chunks ("hand-overs", hibag_k_pass1.h), and the grid that follows.  No HIP call, no
// model, no environment: the launchers (hibag_kernels.hip) call these with what they know, the test entries
// (hibag_hip_test_plan_total / _accum) with what a test gives them -- a test of these functions tests what is launched.
#ifndef HIBAG_PLAN_H_
#define HIBAG_PLAN_H_

// Pass 1 (k_total).  Workgroups [0, n_whole) take one item each; behind them the other `rest` items in K chunks, chunk k
// of item n_whole + j at workgroup n_whole + k * stride + j.
struct HibagPlanTotal {
	unsigned n;         // work items: group quads x items of the model
	int many;           // 1: two rounds or more of the denser build's resident workgroups -- the FP4-only build at six per CU
	unsigned slots;     // resident workgroups of the build chosen (0 = unknown: nothing is cut)
	unsigned K;         // chunks per cut item (1 = none is cut)
	unsigned n_whole;   // undivided items
	unsigned rest;      // cut items: the last, incomplete round and the full round before it (0 = none)
	unsigned stride;    // rest rounded up to a multiple of 8: the chunks of an item share an XCD
	unsigned grid;      // workgroups launched
};

// gx: group quads; n_item: the model's work items; slots_few / slots_many: resident workgroups of the five- and the
// six-per-CU build (of the storing pair or the plain one); k_req: chunks asked for (tail_chunks); vote: majority vote (its
// record log is not handed over: nothing is cut); all_fp4: every item a one-step FP4 classifier; split: the launch walks
// the split item list.
inline HibagPlanTotal hibag_plan_total(unsigned gx, unsigned n_item, int slots_few, int slots_many, int k_req, bool vote,
	bool all_fp4, bool split)
{
	HibagPlanTotal P;
	// more items than resident workgroups: the last, incomplete round and the full round before it go in K chunks each
	P.n = gx * n_item;
	// two rounds of the denser build's resident workgroups or more: six workgroups per CU, otherwise five
	// (the denser build holds the one-step FP4 loop only: models with other work items always take the general one)
	P.many = all_fp4 && !split && slots_many > 0 && P.n >= 2u * (unsigned)slots_many;
	const int slots = P.many ? slots_many : slots_few;
	P.slots = slots > 0 ? (unsigned)slots : 0u;
	P.n_whole = P.n; P.rest = 0; P.stride = 8; P.K = 1;
	if (!vote && k_req > 1 && slots > 0 && P.n > (unsigned)slots) {
		P.K = (unsigned)k_req;
		P.rest = P.n % (unsigned)slots + (unsigned)slots;
		P.n_whole = P.n - P.rest;
		P.stride = (P.rest + 7) / 8 * 8;
	}
	P.grid = P.n_whole + (P.rest ? P.K * P.stride : 0);
	return P;
}

// Pass 2 (k_accum).  Per XCD: workgroups [0, n_whole) take one item each, behind them the other nx - n_whole items in K
// chunks, chunk k of item n_whole + j at n_whole + k * (nx - n_whole) + j; workgroup 8 w + x is number w of XCD x.
struct HibagPlanAccum {
	unsigned nx;        // work items per XCD: group quads x tiles
	unsigned sx;        // resident workgroups per XCD (0 = unknown: nothing is cut)
	unsigned K;         // chunks per cut item (1 = none is cut)
	unsigned n_whole;   // undivided items per XCD
	unsigned grid;      // workgroups launched
};

inline HibagPlanAccum hibag_plan_accum(unsigned nx, int slots, int k_req)
{
	HibagPlanAccum P;
	P.nx = nx;
	P.sx = slots > 0 ? (unsigned)slots / 8 : 0u;
	P.n_whole = nx; P.K = 1;
	if (k_req > 1 && P.sx > 0 && nx > P.sx) {
		P.K = (unsigned)k_req;
		P.n_whole = nx - (nx % P.sx + P.sx);
	}
	P.grid = 8 * (P.n_whole + P.K * (nx - P.n_whole));
	return P;
}

// What a launcher reports of its most recent launch (hibag_hip_test_last_launch).
struct HibagLaunchTotal {
	HibagPlanTotal plan{};
	int launched = 0;   // 1: k_total was launched
	int walk = 0;       // the build's WALK: 0 = every engine, 1 / 2 = the FP4-only builds (generated / prebuilt rows)
	int store = 0;      // the build stores every cell sum
	int vote = 0;       // the majority vote's build
};
struct HibagLaunchAccum {
	HibagPlanAccum plan{};
	int kernel = 0;     // 0 = none (no classifier: the sums are zeroed), 1 = k_accum, 2 = k_accum_cells
};

#endif
