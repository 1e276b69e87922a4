// hibag_groups.hip -- the plan of the group entries (include/hibag_hip.h "allele groups"): the caller's
// partitions of a model's alleles turned, once, into the lists k_finish_groups walks (hibag_k_groups.h), on the model's
// device.  The entries themselves are fronts of the two drivers of hibag_predict.hip (and of hibag_cohort.hip's).

#include "hibag_internal.h"

namespace {

// the marks of a list entry (hibag_k_groups.h has the same values for the kernel)
constexpr uint32_t END = 0x80000000u, TWICE = 0x40000000u, ZERO = 0x20000000u, CELL = 0x1fffffffu;

// One partition's two lists.  `of`: the group of every allele; G groups.
//   call: the cells by (bin, cell), the last of every bin marked END -- n_cell entries;
//   dose: group by group the cells with an allele in it, in cell order, TWICE where both are, the group's last marked END;
//         a group without alleles: one entry ZERO | END.
void partition_lists(const int32_t *of, int n_hla, int G, std::vector<uint32_t> &call, std::vector<uint32_t> &dose)
{
	const size_t P = (size_t)n_hla * (n_hla + 1) / 2;
	std::vector<std::pair<uint32_t, uint32_t>> by_bin;      // (bin, cell): sorted, that is the order of the list
	by_bin.reserve(P);
	std::vector<std::vector<uint32_t>> of_group((size_t)G);
	uint32_t c = 0;
	for (int h1 = 0; h1 < n_hla; h1++)
		for (int h2 = h1; h2 < n_hla; h2++, c++) {            // cell order: c = h2 + h1 (2n - h1 - 1) / 2
			const int a = std::min(of[h1], of[h2]), b = std::max(of[h1], of[h2]);
			by_bin.emplace_back((uint32_t)(b + (long long)a * (2 * G - a - 1) / 2), c);
			if (a == b) of_group[a].push_back(c | TWICE);
			else { of_group[a].push_back(c); of_group[b].push_back(c); }
		}
	std::sort(by_bin.begin(), by_bin.end());
	call.resize(P);
	for (size_t i = 0; i < P; i++)
		call[i] = by_bin[i].second | ((i + 1 == P || by_bin[i + 1].first != by_bin[i].first) ? END : 0u);
	dose.clear();
	for (int g = 0; g < G; g++) {
		if (of_group[g].empty()) { dose.push_back(ZERO | END); continue; }
		dose.insert(dose.end(), of_group[g].begin(), of_group[g].end());
		dose.back() |= END;
	}
}

int groups_create(hibag_hip_model *m, int n_part, const int32_t *group_of, hibag_hip_groups **out)
{
	if (!out) return hibag_fail(HIBAG_HIP_EINVAL, "plan is NULL");
	*out = nullptr;
	if (!m) return hibag_fail(HIBAG_HIP_EINVAL, "model is NULL");
	if (!m->finalized) return hibag_fail(HIBAG_HIP_ESTATE, "model not finalized");
	if (n_part < 1 || n_part > HIBAG_HIP_GROUPS_MAX_PART)
		return hibag_fail(HIBAG_HIP_EINVAL, "n_part = %d is outside 1 .. %d (HIBAG_HIP_GROUPS_MAX_PART)", n_part, HIBAG_HIP_GROUPS_MAX_PART);
	if (!group_of) return hibag_fail(HIBAG_HIP_EINVAL, "group_of is NULL");
	const int nh = m->n_hla;
	if (nh < 1 || (size_t)nh * (nh + 1) / 2 > CELL) return hibag_fail(HIBAG_HIP_EINVAL, "the model has %d alleles", nh);
	hibag_hip_groups *p = nullptr;
	std::vector<uint32_t> call_all, dose_all;
	std::vector<int32_t> offset;
	try {
		p = new hibag_hip_groups;
		p->model = m; p->device = m->device; p->n_hla = nh;
		offset.assign((size_t)n_part + 1, 0);
		for (int q = 0; q < n_part; q++) {
			int G = 0;
			for (int h = 0; h < nh; h++) {
				const int32_t id = group_of[(size_t)q * nh + h];
				if (id < 0 || id >= nh) {
					delete p;
					return hibag_fail(HIBAG_HIP_EINVAL, "group_of[%d][%d] = %d is outside 0 .. %d", q, h, (int)id, nh - 1);
				}
				G = std::max(G, id + 1);
			}
			p->levels.push_back(G);
			offset[q + 1] = offset[q] + G;
			if (offset[q + 1] > HIBAG_HIP_GROUPS_MAX_LEVELS) {
				delete p;
				return hibag_fail(HIBAG_HIP_EINVAL, "the partitions have more than %d groups together (HIBAG_HIP_GROUPS_MAX_LEVELS)", HIBAG_HIP_GROUPS_MAX_LEVELS);
			}
		}
		// the lists, partition-minor: entry i of partition q at [i * n_part + q]; the dosage lists padded to the longest with
		// entries behind the last END (cell 0, no mark: added to a sum nobody stores)
		const size_t P = (size_t)nh * (nh + 1) / 2, Q = (size_t)n_part;
		std::vector<std::vector<uint32_t>> dose((size_t)n_part);
		std::vector<uint32_t> call;
		call_all.assign(P * Q, 0);
		size_t longest = 0;
		for (int q = 0; q < n_part; q++) {
			partition_lists(group_of + (size_t)q * nh, nh, p->levels[q], call, dose[q]);
			for (size_t i = 0; i < P; i++) call_all[i * Q + q] = call[i];
			longest = std::max(longest, dose[q].size());
		}
		dose_all.assign(longest * Q, 0);
		for (int q = 0; q < n_part; q++)
			for (size_t i = 0; i < dose[q].size(); i++) dose_all[i * Q + q] = dose[q][i];
		p->view.n_part = n_part; p->view.n_dose = (int)longest; p->view.n_level = offset[n_part];
	} catch (...) {
		delete p;
		return hibag_fail(HIBAG_HIP_ENOMEM, "out of host memory");
	}
	auto upload = [&]() -> int {
		HIP_TRY(hipSetDevice(p->device));
		const size_t b_call = call_all.size() * sizeof(uint32_t), b_dose = dose_all.size() * sizeof(uint32_t),
			b_group = (size_t)n_part * nh * sizeof(int32_t), b_off = offset.size() * sizeof(int32_t);
		if (int rc = p->d_call.reserve(b_call)) return rc;
		if (int rc = p->d_dose.reserve(b_dose)) return rc;
		if (int rc = p->d_group.reserve(b_group)) return rc;
		if (int rc = p->d_offset.reserve(b_off)) return rc;
		HIP_TRY(hipMemcpy(p->d_call.p, call_all.data(), b_call, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(p->d_dose.p, dose_all.data(), b_dose, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(p->d_group.p, group_of, b_group, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(p->d_offset.p, offset.data(), b_off, hipMemcpyHostToDevice));
		return 0;
	};
	if (int rc = upload()) { hibag_hip_groups_free(p); return rc; }
	p->view.call = p->d_call.as<uint32_t>(); p->view.dose = p->d_dose.as<uint32_t>();
	p->view.group_of = p->d_group.as<int32_t>(); p->view.offset = p->d_offset.as<int32_t>();
	*out = p;
	return 0;
}

} // namespace

extern "C" {

int hibag_hip_groups_create(hibag_hip_model *m, int n_part, const int32_t *group_of, hibag_hip_groups **plan)
{
	return groups_create(m, n_part, group_of, plan);
}

void hibag_hip_groups_free(hibag_hip_groups *plan)
{
	if (!plan) return;
	(void)hipSetDevice(plan->device);
	for (DevBuf *b : {&plan->d_call, &plan->d_dose, &plan->d_group, &plan->d_offset}) b->release();
	delete plan;
}

int hibag_hip_groups_levels(const hibag_hip_groups *plan, int32_t *counts)
{
	if (!plan || !counts) return hibag_fail(HIBAG_HIP_EINVAL, "plan and counts are both required");
	std::copy(plan->levels.begin(), plan->levels.end(), counts);
	return 0;
}

int hibag_hip_groups_tile(const hibag_hip_groups *plan, int *lds)
{
	if (!plan) return hibag_fail(HIBAG_HIP_EINVAL, "plan is NULL");
	return hibag_groups_tile(plan->n_hla * (plan->n_hla + 1) / 2, plan->view.n_part, lds);
}

} // extern "C"
