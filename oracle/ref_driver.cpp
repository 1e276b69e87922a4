// C front end of the HIBAG library sources for tests (oracle.build_ref() compiles it together with them into
// oracle/_ref/libhibag_ref.so).  TEST INFRASTRUCTURE ONLY.  It goes through the library's public classes and nothing else:
// CAttrBag_Model::InitTraining / NewClassifierAllSamp / BuildClassifiers / PredictHLA, CAttrBag_Classifier::Assign and its
// accessors, CAlg_Prediction::Init_Target_IFunc, HLA_LIB::GPUExtProcPtr.
//
// Every entry returns 0 (or a count) on success and -1 on failure.  The library throws std::exception (ErrHLA, and the
// stand-in Rf_error) as well as const char * (src/LibHLA.cpp:1020, :1071), and a plugin may throw const char * through it:
// all three are caught here, the message is kept for ref_last_error(), and GPUExtProcPtr is cleared so that a failed run
// never leaves a plugin installed.
#include "LibHLA.h"

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace HLA_LIB;

namespace {

std::string g_error;

double (*g_unif)(void *) = nullptr;
void *g_unif_state = nullptr;

struct Model {
	CAttrBag_Model m;
	std::vector<int> geno, h1, h2;      // InitTraining keeps the genotype pointer: owned here
	int n_samp = 0, n_hla = 0;
};

// the caller's table, copied (so that its memory may go away), and the build_haplomatch recorder
TypeGPUExtProc g_table;
UINT32 *(*g_real_haplomatch)(const THaplotype[], const size_t[], int, const TGenotype[], size_t &) = nullptr;
int g_rec_n_hla = 0, g_rec_n_samp = 0;      // lengths of build_haplomatch's nHaplo[] and geno[]: the model being trained

struct MatchCall {
	std::vector<THaplotype> haplo;
	std::vector<size_t> lens;
	int n_snp;
	std::vector<TGenotype> geno;
	size_t out_n;
	bool null_buf;
	std::vector<UINT32> buf;
};
std::vector<MatchCall> g_calls;

UINT32 *record_haplomatch(const THaplotype haplo[], const size_t n_haplo[], int n_snp, const TGenotype geno[], size_t &out_n)
{
	MatchCall c;
	c.lens.assign(n_haplo, n_haplo + g_rec_n_hla);
	size_t H = 0;
	for (size_t v : c.lens) H += v;
	c.haplo.assign(haplo, haplo + H);
	c.n_snp = n_snp;
	c.geno.assign(geno, geno + g_rec_n_samp);
	UINT32 *buf = (*g_real_haplomatch)(haplo, n_haplo, n_snp, geno, out_n);
	c.out_n = out_n;
	c.null_buf = buf == nullptr;
	if (buf) c.buf.assign(buf, buf + 1 + (size_t)buf[0]);      // buf[0] = 2 * pairs, then (sample, pair) words
	g_calls.push_back(std::move(c));
	return buf;
}

template <class F> int guarded(F f)
{
	try {
		return f();
	} catch (const std::exception &e) {
		g_error = e.what();
	} catch (const char *msg) {
		g_error = msg ? msg : "(null message)";
	} catch (...) {
		g_error = "unknown exception";
	}
	GPUExtProcPtr = nullptr;
	return -1;
}

const CAttrBag_Classifier &classifier(Model *M, int i)
{
	if (!M || i < 0 || (size_t)i >= M->m.ClassifierList().size()) throw std::runtime_error("classifier index out of range");
	return M->m.ClassifierList()[(size_t)i];
}

} // namespace

// R's uniform generator, for the bootstrap and the SNP sampling (src/LibHLA.cpp:120-126, :930-960)
extern "C" double unif_rand(void)
{
	if (!g_unif) throw std::runtime_error("unif_rand: no source set (ref_set_unif_rand)");
	return (*g_unif)(g_unif_state);
}

extern "C" {

const char *ref_last_error(void) { return g_error.c_str(); }

void ref_set_unif_rand(double (*fn)(void *), void *state) { g_unif = fn; g_unif_state = state; }

int ref_set_target(const char *name)
{
	return guarded([&] { CAlg_Prediction::Init_Target_IFunc(name); return 0; });
}

const char *ref_cpu_info(void) { return CPU_Info(); }

// GPUExtProcPtr = a copy of *table (NULL clears).  record != 0: build_haplomatch is wrapped, each call's inputs and
// returned buffer are kept for ref_match_*; the list of kept calls starts empty.
int ref_set_gpu_table(const void *table, int record)
{
	return guarded([&] {
		g_calls.clear();
		g_real_haplomatch = nullptr;
		if (!table) { GPUExtProcPtr = nullptr; return 0; }
		memcpy(&g_table, table, sizeof(g_table));
		if (record && g_table.build_haplomatch) {
			g_real_haplomatch = g_table.build_haplomatch;
			g_table.build_haplomatch = &record_haplomatch;
		}
		GPUExtProcPtr = &g_table;
		return 0;
	});
}

int ref_gpu_table_is_set(void) { return GPUExtProcPtr != nullptr; }

// a model to assign classifiers to and predict with
void *ref_model_new(int n_snp, int n_samp, int n_hla)
{
	Model *M = nullptr;
	if (guarded([&] { M = new Model; M->n_samp = n_samp; M->n_hla = n_hla; M->m.InitTraining(n_snp, n_samp, n_hla); return 0; }) != 0) {
		delete M;
		return nullptr;
	}
	return M;
}

// a model to train: geno int [n_samp][n_snp], H1 / H2 0-based allele indices [n_samp]
void *ref_model_new_training(int n_snp, int n_samp, const int *geno, int n_hla, const int *H1, const int *H2)
{
	Model *M = nullptr;
	if (guarded([&] {
			M = new Model;
			M->n_samp = n_samp; M->n_hla = n_hla;
			M->geno.assign(geno, geno + (size_t)n_snp * n_samp);
			M->h1.assign(H1, H1 + n_samp);
			M->h2.assign(H2, H2 + n_samp);
			M->m.InitTraining(n_snp, n_samp, M->geno.data(), n_hla, M->h1.data(), M->h2.data());
			return 0;
		}) != 0) {
		delete M;
		return nullptr;
	}
	return M;
}

void ref_model_free(void *h) { delete (Model *)h; }

// NewClassifierAllSamp + Assign; samp_num may be NULL; hla[] ascending
int ref_model_add_classifier(void *h, int n_snp, const int *snpidx, const int *samp_num, int n_haplo, const double *freq,
	const int *hla, const char *const *haplo, double acc)
{
	return guarded([&] {
		Model *M = (Model *)h;
		for (int i = 0; i < n_haplo; i++)
			if (hla[i] < 0 || hla[i] >= M->n_hla) throw std::runtime_error("add_classifier: allele index out of range");
		CAttrBag_Classifier *I = M->m.NewClassifierAllSamp();
		I->Assign(n_snp, snpidx, samp_num, n_haplo, freq, hla, (const char **)haplo, &acc);
		return 0;
	});
}

// PredictHLA; any output may be NULL (H1 and H2 only together)
int ref_model_predict(void *h, const int *geno, int n_samp, int vote_method, int *H1, int *H2, double *max_prob,
	double *matching, double *dosage, double *postprob)
{
	return guarded([&] {
		((Model *)h)->m.PredictHLA(geno, n_samp, vote_method, H1, H2, max_prob, matching, dosage, postprob, false);
		return 0;
	});
}

// BuildClassifiers; returns the model's number of classifiers
int ref_model_train(void *h, int nclassifier, int mtry, int prune)
{
	return guarded([&] {
		Model *M = (Model *)h;
		g_rec_n_hla = M->n_hla; g_rec_n_samp = M->n_samp;
		M->m.BuildClassifiers(nclassifier, mtry, prune != 0, false, false);
		return (int)M->m.ClassifierList().size();
	});
}

int ref_model_n_classifier(void *h) { return (int)((Model *)h)->m.ClassifierList().size(); }

int ref_classifier_info(void *h, int i, int *n_snp, int *n_haplo, double *acc)
{
	return guarded([&] {
		const CAttrBag_Classifier &c = classifier((Model *)h, i);
		*n_snp = c.nSNP(); *n_haplo = c.nHaplo(); *acc = c.OutOfBag_Accuracy();
		return 0;
	});
}

// snpidx[n_snp], samp_num[n_samp], freq / hla [n_haplo], bits[2 * n_haplo]: the packed words as stored -- bits at or above
// n_snp are whatever the library left there
int ref_classifier_get(void *h, int i, int *snpidx, int *samp_num, double *freq, int *hla, uint64_t *bits)
{
	return guarded([&] {
		const CAttrBag_Classifier &c = classifier((Model *)h, i);
		std::copy(c.SNPIndex().begin(), c.SNPIndex().end(), snpidx);
		std::copy(c.BootstrapCount().begin(), c.BootstrapCount().end(), samp_num);
		const CHaplotypeList &L = c.Haplotype();
		size_t k = 0;
		for (size_t a = 0; a < L.LenPerHLA.size(); a++)
			for (size_t j = 0; j < L.LenPerHLA[a]; j++, k++) {
				if (k >= L.Num_Haplo) throw std::runtime_error("classifier_get: LenPerHLA exceeds Num_Haplo");
				freq[k] = L.List[k].Freq;
				hla[k] = (int)a;
				bits[2 * k] = (uint64_t)L.List[k].PackedHaplo[0];
				bits[2 * k + 1] = (uint64_t)L.List[k].PackedHaplo[1];
			}
		if (k != L.Num_Haplo) throw std::runtime_error("classifier_get: LenPerHLA does not sum to Num_Haplo");
		return 0;
	});
}

// the recorded build_haplomatch calls of the last training run
int ref_match_count(void) { return (int)g_calls.size(); }

// n_hla = length of lens, n_geno = length of geno; buf_len = -1 where the plugin returned NULL
int ref_match_info(int i, int *n_haplo, int *n_hla, int *n_snp, int *n_geno, long long *out_n, long long *buf_len)
{
	return guarded([&] {
		const MatchCall &c = g_calls.at((size_t)i);
		*n_haplo = (int)c.haplo.size(); *n_hla = (int)c.lens.size(); *n_snp = c.n_snp; *n_geno = (int)c.geno.size();
		*out_n = (long long)c.out_n; *buf_len = c.null_buf ? -1 : (long long)c.buf.size();
		return 0;
	});
}

// haplo: 32-byte THaplotype records, geno: 48-byte TGenotype records (inst/include/LibHLA_ext.h:261-352)
int ref_match_get(int i, void *haplo, long long *lens, void *geno, uint32_t *buf)
{
	return guarded([&] {
		const MatchCall &c = g_calls.at((size_t)i);
		memcpy(haplo, c.haplo.data(), c.haplo.size() * sizeof(THaplotype));
		for (size_t a = 0; a < c.lens.size(); a++) lens[a] = (long long)c.lens[a];
		memcpy(geno, c.geno.data(), c.geno.size() * sizeof(TGenotype));
		if (!c.buf.empty()) memcpy(buf, c.buf.data(), c.buf.size() * sizeof(UINT32));
		return 0;
	});
}

} // extern "C"
