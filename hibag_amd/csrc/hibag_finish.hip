// hibag_finish.hip -- the one host module that knows the finishes (Finish, ListOut: hibag_internal.h).  Behind passes 1 and 2 a
// call runs one of six finish kernels; what differs between them on the host side is here, each function one switch over
// ListOut::kind: the finish's own argument check, the state a call needs on the device before its first batch, the
// finish's per-batch workspace, and its launch.  The drivers of hibag_predict.hip (predict_device_locked, StagedRun) and the
// entries call these and ListOut's methods and otherwise know nothing about any finish; a new finish is a value of the
// enumeration, a case in each switch here and its `extern "C"` fronts.

#include "hibag_internal.h"

namespace hibag_detail {

int check_list_args(const hibag_hip_model *m, int n_samp, const ListOut &list)
{
	static_assert(HIBAG_HIP_TOPK_MAX == HIBAG_TOPK_MAX && HIBAG_HIP_DRAW_MAX == HIBAG_DRAW_MAX, "the public bounds are the kernels' bounds");
	switch (list.kind) {
	case Finish::CALL: return 0;
	case Finish::FAMILY:
		if (n_samp > 0 && !list.pedigree) return hibag_fail(HIBAG_HIP_EINVAL, "pedigree is NULL");
		if (n_samp > 0 && (!list.h1 || !list.h2 || !list.prob || !list.support))
			return hibag_fail(HIBAG_HIP_EINVAL, "h1, h2, prob and support are all required");
		for (int s = 0; s < n_samp; s++)
			for (int k = 0; k < 2; k++) {
				const int32_t p = list.pedigree[2 * (size_t)s + k];
				if (p < -1 || p >= s)
					return hibag_fail(HIBAG_HIP_EINVAL, "pedigree[%d][%d] = %d: a parent index must lie in -1 .. %d (parents precede "
						"their children in the call)", s, k, (int)p, s - 1);
			}
		for (int h = 0; list.prior && n_samp > 0 && h < list.n_hla; h++)
			if (!(list.prior[h] > 0) || !(list.prior[h] <= 1.79769313486231570815e+308))
				return hibag_fail(HIBAG_HIP_EINVAL, "prior[%d] = %g: every entry of the prior must be finite and > 0", h, list.prior[h]);
		return 0;
	case Finish::GIVEN:
		if (n_samp > 0 && !list.allow) return hibag_fail(HIBAG_HIP_EINVAL, "allow is NULL");
		if (n_samp > 0 && (!list.h1 || !list.h2 || !list.prob || !list.support))
			return hibag_fail(HIBAG_HIP_EINVAL, "h1, h2, prob and support are all required");
		return 0;
	case Finish::GROUPS:
		if (!list.plan) return hibag_fail(HIBAG_HIP_EINVAL, "the group plan is NULL");
		if (list.plan->model != m) return hibag_fail(HIBAG_HIP_EINVAL, "the group plan was made for another model");
		break;
	case Finish::DRAW:
		if (list.k < 1 || list.k > HIBAG_HIP_DRAW_MAX)
			return hibag_fail(HIBAG_HIP_EINVAL, "n_draw = %d is outside 1 .. %d (HIBAG_HIP_DRAW_MAX)", list.k, HIBAG_HIP_DRAW_MAX);
		if (list.sample0 < 0) return hibag_fail(HIBAG_HIP_EINVAL, "sample0 = %lld is negative", (long long)list.sample0);
		break;
	case Finish::TOPK:
		if (list.k < 1 || list.k > HIBAG_HIP_TOPK_MAX)
			return hibag_fail(HIBAG_HIP_EINVAL, "k = %d is outside 1 .. %d (HIBAG_HIP_TOPK_MAX)", list.k, HIBAG_HIP_TOPK_MAX);
		break;
	}
	if (n_samp > 0 && (!list.h1 || !list.h2 || !list.prob)) return hibag_fail(HIBAG_HIP_EINVAL, "h1, h2 and prob are all required");
	return 0;
}

// ---- the family entries' call-wide state (include/hibag_hip.h "pedigrees") ----------------------------------------
// depth(s) = 0 without a parent in the call, else 1 + the larger depth of its parents: one pass, parents precede their
// children (check_list_args has seen to it).
static int family_depths(const ListOut &list, std::vector<int32_t> &depth)
{
	try { depth.assign((size_t)list.n_call, 0); } catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
	for (int s = 0; s < list.n_call; s++)
		for (int k = 0; k < 2; k++) {
			const int32_t p = list.pedigree[2 * (size_t)s + k];
			if (p >= 0) depth[s] = std::max(depth[s], depth[p] + 1);
		}
	return 0;
}

// where the call's inputs lie in m->ws_fam_in: the pedigree, the depths (int32), then the prior (double, 8-aligned)
static size_t family_prior_at(size_t n_call) { return (3 * n_call * sizeof(int32_t) + 7) / 8 * 8; }

// host -> device of the call's pedigree, depths and prior on `st`, once per run (so a run repeated after a failed hand-over
// sends them again; ws_family is rebuilt by the run itself, parents first).  Waits for the copy: the image is pageable host
// memory about to go out of scope.
static int family_upload(hibag_hip_model *m, const ListOut &list, hipStream_t st)
{
	const size_t n = (size_t)list.n_call, nh = (size_t)list.n_hla, at = family_prior_at(n);
	std::vector<char> image;
	try { image.assign(at + nh * sizeof(double), 0); } catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
	memcpy(image.data(), list.pedigree, 2 * n * sizeof(int32_t));
	memcpy(image.data() + 2 * n * sizeof(int32_t), m->fam_depth.data(), n * sizeof(int32_t));
	if (list.prior) memcpy(image.data() + at, list.prior, nh * sizeof(double));
	HIP_TRY(hipMemcpyAsync(m->ws_fam_in.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

static HibagFamilyView family_view(hibag_hip_model *m, const ListOut &list)
{
	const size_t n = (size_t)list.n_call;
	HibagFamilyView F;
	F.ped = m->ws_fam_in.as<int32_t>(); F.depth = F.ped + 2 * n;
	F.prior = list.prior ? (const double *)(m->ws_fam_in.as<char>() + family_prior_at(n)) : nullptr;
	F.fam_D = m->ws_family.as<double>(); F.fam_S = F.fam_D + n * (size_t)list.n_hla;
	F.ratios = m->ws_ratios.as<double>();
	F.call0 = list.call0;
	return F;
}

int finish_call_state(hibag_hip_model *m, ListOut &list, int n_samp, bool host_route, hipStream_t st, hipStream_t up)
{
	switch (list.kind) {
	case Finish::GIVEN: {
		// A host route's constraint goes up once per run -- so a run repeated after a failed hand-over sends it again --, ahead of
		// the first slice's genotypes on the stream they take (in order, so the first slice's `up` event stands for it too).  It
		// is a few words per sample; every slice reads its part of the one device copy.
		if (!host_route) return 0;                 // (a device-pointer entry's sets are on the device as they are)
		const size_t bytes = (size_t)n_samp * list.allow_words() * sizeof(uint32_t);
		if (int rc = m->ws_allow.reserve(bytes)) return rc;
		HIP_TRY(hipMemcpyAsync(m->ws_allow.p, list.allow, bytes, hipMemcpyHostToDevice, up));
		list.allow = m->ws_allow.as<uint32_t>();
		return 0;
	}
	case Finish::FAMILY:
		list.n_call = n_samp;
		if (int rc = family_depths(list, m->fam_depth)) return rc;
		if (!host_route) if (int rc = workspace_enter(m, st)) return rc;
		if (int rc = m->ws_fam_in.reserve(family_prior_at((size_t)n_samp) + std::max<size_t>(list.n_hla, 1) * sizeof(double))) return rc;
		if (int rc = m->ws_family.reserve(std::max<size_t>((size_t)n_samp * ((size_t)list.n_hla + 1), 1) * sizeof(double))) return rc;
		return family_upload(m, list, st);
	default: return 0;
	}
}

int finish_reserve_batch(hibag_hip_model *m, const ListOut &list, int n_pad)
{
	switch (list.kind) {
	case Finish::GIVEN:                            // a batch's masks, word-major ([2 W][n_pad]: hibag_k_given.h)
		return m->ws_masks.reserve(list.allow_words() * (size_t)n_pad * sizeof(uint32_t));
	case Finish::FAMILY:                           // a batch's ratio vectors, allele-major ([2 n_hla][n_pad]: hibag_k_family.h)
		return m->ws_ratios.reserve((size_t)2 * std::max(list.n_hla, 1) * (size_t)n_pad * sizeof(double));
	default: return 0;
	}
}

int finish_launch(hibag_hip_model *m, HibagBatchView &B, const PredictOut &o, hipStream_t st)
{
	const ListOut &l = o.list;
	switch (l.kind) {
	case Finish::CALL:
		hibag_launch_finish(m->view, B, B.part, o.H1, o.H2, o.max_prob, o.matching, o.dosage, o.postprob, st);
		break;
	case Finish::TOPK:
		hibag_launch_finish_topk(m->view, B, B.part, l.k, l.h1, l.h2, l.prob, o.matching, st);
		break;
	case Finish::DRAW:
		hibag_launch_finish_draw(m->view, B, B.part, l.k, l.seed, l.sample0, l.h1, l.h2, l.prob, o.matching, st);
		break;
	case Finish::GROUPS:
		hibag_launch_finish_groups(m->view, B, B.part, l.plan->view, l.h1, l.h2, l.prob, o.matching, l.dosage, st);
		break;
	case Finish::GIVEN:
		hibag_launch_finish_given(m->view, B, B.part, l.allow, m->ws_masks.as<uint32_t>(), l.h1, l.h2, l.prob, l.support, o.matching,
			l.dosage, st);
		break;
	case Finish::FAMILY: {
		// the rounds: the distinct depths of the batch's samples, ascending (one pass: a depth is at most the batch's
		// generations, a small number)
		const int32_t *depth = m->fam_depth.data() + l.call0;
		std::vector<int> rounds;
		try {
			const int deepest = *std::max_element(depth, depth + B.n_samp);
			std::vector<char> seen((size_t)deepest + 1, 0);
			for (int s = 0; s < B.n_samp; s++) seen[depth[s]] = 1;
			for (int d = 0; d <= deepest; d++) if (seen[d]) rounds.push_back(d);
		} catch (...) { return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory"); }
		hibag_launch_finish_family(m->view, B, B.part, family_view(m, l), rounds.data(), (int)rounds.size(), l.h1, l.h2, l.prob,
			l.support, o.matching, l.dosage, st);
		break;
	}
	}
	return 0;
}

} // namespace hibag_detail
