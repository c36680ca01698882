// gorse_host_capi.cpp -- flat C entry points over the C++ host mirror, so that the parity tests
// (pytest + ctypes) can drive gorse::cf::BPR / ALS / Evaluate / ann::Bruteforce / heap::* exactly as
// the reference's Go tests drive their Go twins.  Test/binding plumbing only.
#include <cstring>
#include <sstream>

#include "gorse_cf.hpp"
#include "gorse_ctr.hpp"
#include "gorse_vectors.hpp"
#include "../csrc/rank_keys.hpp"
#include "../csrc/sparse_host.hpp"
#include "../csrc/als_plan.hpp"
#include "../csrc/bpr_bins.hpp"
#include "../csrc/hot_rows.hpp"
#include "../csrc/topk_sym.hpp"

using namespace gorse;

namespace {
thread_local std::string g_err;
template <typename F>
int32_t guard(F &&f) {
    try {
        f();
        return 0;
    } catch (const HipError &e) {
        g_err = e.what();
        return e.code;
    } catch (const storage::ErrNotFound &e) {
        g_err = e.what();
        return -201;
    } catch (const storage::ErrAlreadyExists &e) {
        g_err = e.what();
        return -202;
    } catch (const storage::ErrNotSupported &e) {
        g_err = e.what();
        return -203;
    } catch (const std::out_of_range &e) {
        g_err = e.what();
        return GORSE_ERR_RANGE;
    } catch (const std::invalid_argument &e) {
        g_err = e.what();
        return GORSE_ERR_INVALID;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -100;
    }
}
struct FitLog {
    std::string text;
};
}  // namespace

extern "C" {
const char *gh_last_error() { return g_err.c_str(); }

// ---- dataset ---------------------------------------------------------------------------------
void *gh_dataset_new() { return new dataset::Dataset(); }
void *gh_dataset_new_shared(void *other) { return new dataset::Dataset(*(dataset::Dataset *)other, true); }
void gh_dataset_free(void *d) { delete (dataset::Dataset *)d; }
void gh_dataset_add_feedback(void *d, const int32_t *u, const int32_t *i, int64_t n) {
    auto *ds = (dataset::Dataset *)d;
    for (int64_t t = 0; t < n; t++) ds->AddFeedbackIndexed(u[t], i[t]);
}
void gh_dataset_add_feedback_str(void *d, const char *user, const char *item) {
    ((dataset::Dataset *)d)->AddFeedback(user, item);
}
void gh_dataset_add_user(void *d, const char *user) { ((dataset::Dataset *)d)->AddUser(user); }
void gh_dataset_add_item(void *d, const char *item) { ((dataset::Dataset *)d)->AddItem(item); }
void gh_dataset_set_negatives(void *d, int32_t user, const int32_t *neg, int32_t n) {
    ((dataset::Dataset *)d)->SetNegatives(user, std::vector<int32_t>(neg, neg + n));
}
int32_t gh_dataset_count_users(void *d) { return ((dataset::Dataset *)d)->CountUsers(); }
int32_t gh_dataset_count_items(void *d) { return ((dataset::Dataset *)d)->CountItems(); }
int32_t gh_dataset_count_feedback(void *d) { return ((dataset::Dataset *)d)->CountFeedback(); }
// SplitCF(numTestUsers, seed): two new datasets (free both)
int32_t gh_dataset_split_cf(void *d, int32_t num_test_users, int64_t seed, void **train, void **test) {
    return guard([&] {
        auto pr = ((dataset::Dataset *)d)->SplitCF(num_test_users, seed);
        *train = new dataset::Dataset(std::move(pr.first));
        *test = new dataset::Dataset(std::move(pr.second));
    });
}
// LoadDataFromBuiltIn's two files, given as text
int32_t gh_dataset_load_ncf(const char *train_txt, const char *test_txt, void **train, void **test) {
    return guard([&] {
        std::istringstream a(train_txt), b(test_txt);
        auto pr = dataset::Dataset::LoadNCF(a, b);
        *train = new dataset::Dataset(std::move(pr.first));
        *test = new dataset::Dataset(std::move(pr.second));
    });
}
// row `row` of GetUserFeedback (side 0) / GetItemFeedback (side 1) / the stored negatives (side 2); returns its length
int32_t gh_dataset_row(void *d, int32_t side, int32_t row, int32_t *out, int32_t cap) {
    auto *ds = (dataset::Dataset *)d;
    const auto &m = side == 0 ? ds->GetUserFeedback() : (side == 1 ? ds->GetItemFeedback() : ds->Negatives());
    if (row < 0 || (size_t)row >= m.size()) return 0;
    const auto &r = m[(size_t)row];
    for (size_t t = 0; t < r.size() && (int32_t)t < cap; t++) out[t] = r[t];
    return (int32_t)r.size();
}
// GetUserIDF (side 0) / GetItemIDF (side 1) into out[CountUsers() / CountItems() of the dictionary]
int32_t gh_dataset_idf(void *d, int32_t side, float *out, int32_t cap) {
    auto v = side == 0 ? ((dataset::Dataset *)d)->GetUserIDF() : ((dataset::Dataset *)d)->GetItemIDF();
    for (size_t t = 0; t < v.size() && (int32_t)t < cap; t++) out[t] = v[t];
    return (int32_t)v.size();
}

// ---- FreqDict / RandomGenerator (test hooks over dataset/dict.go, common/util/random.go) --------------------------------------
void *gh_freqdict_new() { return new dataset::FreqDict(); }
void gh_freqdict_free(void *d) { delete (dataset::FreqDict *)d; }
int32_t gh_freqdict_add(void *d, const char *s) { return ((dataset::FreqDict *)d)->Add(s); }
int32_t gh_freqdict_add_no_count(void *d, const char *s) { return ((dataset::FreqDict *)d)->AddNoCount(s); }
int32_t gh_freqdict_count(void *d) { return ((dataset::FreqDict *)d)->Count(); }
int32_t gh_freqdict_freq(void *d, int32_t id) { return ((dataset::FreqDict *)d)->Freq(id); }
int32_t gh_freqdict_id(void *d, const char *s) { return ((dataset::FreqDict *)d)->Id(s); }
void gh_rng_normal_matrix(int64_t seed, int64_t rows, int64_t cols, float mean, float stddev, float *out) {
    util::RandomGenerator rng(seed);
    std::vector<float> m;
    rng.NormalMatrix(rows, cols, mean, stddev, m);
    std::copy(m.begin(), m.end(), out);
}
// successive SampleInt32(low, high, n[i], exclude) calls on ONE generator, like random_test.go:51-59; out = concatenation
int32_t gh_rng_sample_int32(int64_t seed, int32_t low, int32_t high, const int32_t *ns, int32_t n_calls, const int32_t *exclude,
                            int32_t n_exclude, int32_t *out, int32_t *out_lens) {
    util::RandomGenerator rng(seed);
    const std::set<int32_t> ex(exclude, exclude + n_exclude);
    int32_t at = 0;
    for (int32_t c = 0; c < n_calls; c++) {
        auto v = rng.SampleInt32(low, high, ns[c], ex);
        out_lens[c] = (int32_t)v.size();
        for (int32_t x : v) out[at++] = x;
    }
    return at;
}

// ---- models ------------------------------------------------------------------------------------
static model::Params make_params(const char **names, const double *vals, int32_t n) {
    model::Params p;
    for (int32_t k = 0; k < n; k++) p[names[k]] = vals[k];
    return p;
}
void *gh_bpr_new(const char **names, const double *vals, int32_t n) { return new cf::BPR(make_params(names, vals, n)); }
void *gh_als_new(const char **names, const double *vals, int32_t n) { return new cf::ALS(make_params(names, vals, n)); }
void gh_model_free(void *m) { delete (cf::MatrixFactorization *)m; }
const char *gh_model_name(void *m) { return ((cf::MatrixFactorization *)m)->Name(); }

// Fit(ctx, trainSet, valSet, config) -> Score.  log_out receives the zap-style log lines.
int32_t gh_model_fit(void *m, void *train, void *val, int32_t jobs, int32_t verbose, int32_t candidates, int32_t topk,
                     int32_t patience, const volatile int32_t *cancel, float *score3, int32_t *epochs_done, char *log_out,
                     int64_t log_cap) {
    return guard([&] {
        cf::FitConfig c;
        c.Jobs = jobs, c.Verbose = verbose, c.Candidates = candidates, c.TopK = topk, c.Patience = patience, c.Cancel = cancel;
        std::string logs;
        // (the count of epochs comes from the model: EpochsDone)
        c.Log = [&](const std::string &s) { logs += s + "\n"; };
        cf::Score s = ((cf::MatrixFactorization *)m)->Fit(*(dataset::Dataset *)train, *(dataset::Dataset *)val, c);
        score3[0] = s.NDCG, score3[1] = s.Precision, score3[2] = s.Recall;
        if (epochs_done) *epochs_done = ((cf::MatrixFactorization *)m)->EpochsDone();
        if (log_out && log_cap > 0) {
            size_t n = std::min<size_t>((size_t)log_cap - 1, logs.size());
            memcpy(log_out, logs.data(), n);
            log_out[n] = 0;
        }
    });
}
int32_t gh_model_predict(void *m, const char *user, const char *item, float *out) {
    return guard([&] { *out = ((cf::MatrixFactorization *)m)->Predict(user, item); });
}
int32_t gh_model_internal_predict(void *m, int32_t u, int32_t i, float *out) {
    return guard([&] { *out = ((cf::MatrixFactorization *)m)->internalPredict(u, i); });
}
int32_t gh_model_n_factors(void *m) { return ((cf::MatrixFactorization *)m)->NFactors(); }
int32_t gh_model_count_users(void *m) {
    auto *mf = (cf::MatrixFactorization *)m;
    return mf->UserIndex ? mf->UserIndex->Count() : -1;
}
int32_t gh_model_count_items(void *m) {
    auto *mf = (cf::MatrixFactorization *)m;
    return mf->ItemIndex ? mf->ItemIndex->Count() : -1;
}
int32_t gh_model_user_index(void *m, const char *id) {
    auto *mf = (cf::MatrixFactorization *)m;
    return mf->UserIndex ? mf->UserIndex->Id(id) : -1;
}
int32_t gh_model_item_index(void *m, const char *id) {
    auto *mf = (cf::MatrixFactorization *)m;
    return mf->ItemIndex ? mf->ItemIndex->Id(id) : -1;
}
void gh_model_get_user_factor(void *m, int32_t u, float *out) {
    auto *mf = (cf::MatrixFactorization *)m;
    memcpy(out, mf->GetUserFactor(u), (size_t)mf->NFactors() * 4);
}
void gh_model_get_item_factor(void *m, int32_t i, float *out) {
    auto *mf = (cf::MatrixFactorization *)m;
    memcpy(out, mf->GetItemFactor(i), (size_t)mf->NFactors() * 4);
}
int32_t gh_model_is_user_predictable(void *m, int32_t u) { return ((cf::MatrixFactorization *)m)->IsUserPredictable(u); }
int32_t gh_model_is_item_predictable(void *m, int32_t i) { return ((cf::MatrixFactorization *)m)->IsItemPredictable(i); }
void gh_model_clear(void *m) { ((cf::MatrixFactorization *)m)->Clear(); }
int32_t gh_model_invalid(void *m) { return ((cf::MatrixFactorization *)m)->Invalid(); }
// MarshalModel into a caller buffer; returns bytes needed
int64_t gh_model_marshal(void *m, char *buf, int64_t cap) {
    std::ostringstream o;
    cf::MarshalModel(o, *(cf::MatrixFactorization *)m);
    const std::string &s = o.str();
    if (buf && cap >= (int64_t)s.size()) memcpy(buf, s.data(), s.size());
    return (int64_t)s.size();
}
void *gh_model_unmarshal(const char *buf, int64_t n) {
    void *r = nullptr;
    guard([&] {
        std::istringstream i(std::string(buf, (size_t)n));
        r = cf::UnmarshalModel(i).release();
    });
    return r;
}
// test helper: a model whose factors are given (ids "0".."n-1"), the equivalent of Unmarshal
int32_t gh_model_load_factors(void *m, int32_t U, int32_t I, const float *P, const float *Q) {
    return guard([&] {
        auto *mf = (cf::MatrixFactorization *)m;
        mf->Clear();
        const int d = mf->NFactors();
        mf->UserIndex = std::make_shared<dataset::FreqDict>();
        mf->ItemIndex = std::make_shared<dataset::FreqDict>();
        for (int32_t u = 0; u < U; u++) mf->UserIndex->Add(std::to_string(u));
        for (int32_t i = 0; i < I; i++) mf->ItemIndex->Add(std::to_string(i));
        mf->UserPredictable.assign((size_t)U, true);
        mf->ItemPredictable.assign((size_t)I, true);
        mf->UserFactor.assign(P, P + (size_t)U * (size_t)d);
        mf->ItemFactor.assign(Q, Q + (size_t)I * (size_t)d);
    });
}
// Evaluate(estimator, testSet, trainSet, topK, numCandidates, nJobs, metrics...); metric ids 0..5
int32_t gh_evaluate(void *m, void *test, void *train, int32_t topk, int32_t candidates, int32_t jobs, const int32_t *metric_ids,
                    int32_t n_metrics, float *out) {
    return guard([&] {
        static const cf::Metric table[] = {cf::NDCG, cf::Precision, cf::Recall, cf::HR, cf::MAP, cf::MRR};
        std::vector<cf::Metric> ms;
        for (int32_t k = 0; k < n_metrics; k++) ms.push_back(table[metric_ids[k]]);
        auto r = cf::Evaluate(*(cf::MatrixFactorization *)m, *(dataset::Dataset *)test, *(dataset::Dataset *)train, topk,
                              candidates, jobs, ms);
        for (int32_t k = 0; k < n_metrics; k++) out[k] = r[(size_t)k];
    });
}
// MatrixFactorization::SetHostEvaluate: Evaluate (Fit's included) ranks on the device and walks the metrics on the host
void gh_model_set_host_evaluate(void *m, int32_t on) { ((cf::MatrixFactorization *)m)->SetHostEvaluate(on != 0); }
float gh_metric(int32_t id, const int32_t *target, int32_t nt, const int32_t *rank, int32_t nr) {
    static const cf::Metric table[] = {cf::NDCG, cf::Precision, cf::Recall, cf::HR, cf::MAP, cf::MRR};
    return table[id](cf::TargetSet(target, target + nt), std::vector<int32_t>(rank, rank + nr));
}

// ---- ModelSearch (optimize.go) ---------------------------------------------------------------------------------------
namespace {
// optimize_test.go:29-99: a model whose Fit returns NDCG = NFactors + InitMean + InitStdDev over a 4 x 4 x 1 grid
struct MockForSearch : cf::MatrixFactorization {
    const char *Name() const override { return "mock"; }
    cf::Score Fit(dataset::Dataset &, dataset::Dataset &, const cf::FitConfig &) override {
        cf::Score s;
        s.NDCG = Params.GetFloat32(model::NFactors, 0) + Params.GetFloat32(model::InitMean, 0) + Params.GetFloat32(model::InitStdDev, 0);
        return s;
    }
    model::Params SuggestParams(cf::Trial &trial) override {
        model::Params p;
        p[model::NFactors] = trial.SuggestDiscreteFloat(model::NFactors, 1, 4, 1);
        p[model::InitMean] = trial.SuggestDiscreteFloat(model::InitMean, 1, 4, 1);
        p[model::InitStdDev] = trial.SuggestDiscreteFloat(model::InitStdDev, 4, 4, 1);
        return p;
    }
};
void report(const cf::SearchResult &r, char *type_out, int64_t type_cap, char *params_out, int64_t params_cap, float *score3) {
    if (type_out && type_cap > (int64_t)r.Type.size()) std::memcpy(type_out, r.Type.c_str(), r.Type.size() + 1);
    std::string text;
    for (auto &kv : r.Params) {
        char num[64];
        snprintf(num, sizeof(num), "%.17g", kv.second);
        text += kv.first + "=" + num + "\n";
    }
    if (params_out && params_cap > (int64_t)text.size()) std::memcpy(params_out, text.c_str(), text.size() + 1);
    score3[0] = r.Score_.NDCG, score3[1] = r.Score_.Precision, score3[2] = r.Score_.Recall;
}
}  // namespace
// TestTPE's search (optimize_test.go:101-126); sampler: 0 = TPE (what the reference's test and master use), 1 = random;
// best_value = study.GetBestValue()
int32_t gh_search_mock(int32_t n_trials, int64_t seed, int32_t sampler, double *best_value, char *type_out, int64_t type_cap,
                       char *params_out, int64_t params_cap, float *score3) {
    return guard([&] {
        cf::ModelSearch search({{"mock", [] { return std::unique_ptr<cf::MatrixFactorization>(new MockForSearch()); }}}, nullptr,
                               nullptr, cf::FitConfig(), false);
        cf::Study study(seed, sampler ? cf::Study::Sampler::Random : cf::Study::Sampler::TPE);
        study.Optimize([&](cf::Trial &t) { return search.Objective(t); }, n_trials);
        *best_value = study.GetBestValue();
        report(search.Result(), type_out, type_cap, params_out, params_cap, score3);
    });
}
// optimizeCollaborativeFiltering (master/tasks.go:1268-1316): BPR and ALS with their default parameters (+ the overrides
// given, e.g. NEpochs), FitConfig{Jobs, Patience}, n_trials trials; counters = {dataset uploads, resident reuses, trials run}
int32_t gh_model_search(void *train, void *val, int32_t n_trials, int64_t seed, int32_t jobs, int32_t patience,
                        const char **names, const double *vals, int32_t n_over, int32_t keep_resident, const volatile int32_t *cancel,
                        char *type_out, int64_t type_cap, char *params_out, int64_t params_cap, float *score3, int32_t *counters) {
    return guard([&] {
        // the overrides are re-applied after SuggestParams (which replaces the whole parameter set, optimize.go:69)
        const model::Params over = make_params(names, vals, n_over);
        struct BPRo : cf::BPR {
            model::Params over;
            model::Params SuggestParams(cf::Trial &t) override {
                model::Params p = cf::BPR::SuggestParams(t);
                for (auto &kv : over) p[kv.first] = kv.second;
                return p;
            }
        };
        struct ALSo : cf::ALS {
            model::Params over;
            model::Params SuggestParams(cf::Trial &t) override {
                model::Params p = cf::ALS::SuggestParams(t);
                for (auto &kv : over) p[kv.first] = kv.second;
                return p;
            }
        };
        cf::FitConfig c;
        c.SetJobs(jobs).SetPatience(patience);
        c.Cancel = cancel;
        cf::ModelSearch search({{"BPR", [&] { auto m = new BPRo(); m->over = over; return std::unique_ptr<cf::MatrixFactorization>(m); }},
                                {"ALS", [&] { auto m = new ALSo(); m->over = over; return std::unique_ptr<cf::MatrixFactorization>(m); }}},
                               (dataset::Dataset *)train, (dataset::Dataset *)val, c, keep_resident != 0);
        int trials = 0;
        search.OnTrial = [&] { trials++; };
        cf::Study study(seed);
        study.Optimize([&](cf::Trial &t) { return search.Objective(t); }, n_trials, cancel);
        report(search.Result(), type_out, type_cap, params_out, params_cap, score3);
        if (counters) counters[0] = search.Resident().uploads, counters[1] = search.Resident().reuses, counters[2] = trials;
    });
}

// ---- the TPE sampler's pieces (tpe.hpp), for the CPU tests ---------------------------------------------------------------
// the Parzen estimator of `n` observations on [low, high]: returns the number of components (n + 1), fills weights / mus / sigmas
int32_t gh_tpe_parzen(const double *obs, int32_t n, double low, double high, double *weights, double *mus, double *sigmas, int32_t cap) {
    const cf::tpe::ParzenEstimator pe(std::vector<double>(obs, obs + n), low, high);
    const int32_t m = (int32_t)pe.mus.size();
    for (int32_t i = 0; i < m && i < cap; i++) weights[i] = pe.weights[(size_t)i], mus[i] = pe.mus[(size_t)i], sigmas[i] = pe.sigmas[(size_t)i];
    return m;
}
int32_t gh_tpe_gamma(int32_t n) { return cf::tpe::default_gamma(n); }
void gh_tpe_weights(int32_t n, double *out) {
    const std::vector<double> w = cf::tpe::default_weights(n);
    for (size_t i = 0; i < w.size(); i++) out[i] = w[i];
}
void gh_tpe_log_pdf(const double *samples, int32_t ns, const double *obs, int32_t n, double low, double high, double q, double *out) {
    const cf::tpe::ParzenEstimator pe(std::vector<double>(obs, obs + n), low, high);
    const std::vector<double> r = cf::tpe::gmm_log_pdf(std::vector<double>(samples, samples + ns), pe, low, high, q);
    for (size_t i = 0; i < r.size(); i++) out[i] = r[i];
}
// a study over one log-uniform parameter x in [low, high] with the objective -(log x - log target)^2: the values suggested
void gh_tpe_study_1d(int32_t n_trials, int64_t seed, int32_t sampler, double low, double high, double target, double *suggested) {
    cf::Study study(seed, sampler ? cf::Study::Sampler::Random : cf::Study::Sampler::TPE);
    int t = 0;
    study.Optimize([&](cf::Trial &trial) {
        const double x = trial.SuggestLogFloat("x", low, high);
        suggested[t++] = x;
        const double e = std::log(x) - std::log(target);
        return -e * e;
    }, n_trials);
}

// ---- gob (test hooks of gob.hpp) and the MatrixFactorizationUsers blob --------------------------------------------------
static int64_t copy_out(const std::string &s, char *buf, int64_t cap) {
    if (buf && cap >= (int64_t)s.size()) memcpy(buf, s.data(), s.size());
    return (int64_t)s.size();
}
int64_t gh_gob_encode_int(int64_t v, char *buf, int64_t cap) { return copy_out(gob::encode_int(v), buf, cap); }
int64_t gh_gob_encode_string(const char *s, char *buf, int64_t cap) { return copy_out(gob::encode_string(s), buf, cap); }
int32_t gh_gob_decode_int(const char *buf, int64_t n, int64_t *out) {
    return guard([&] { *out = gob::decode_int(std::string(buf, (size_t)n)); });
}
// kinds: 0 int, 1 float64, 2 bool
int64_t gh_gob_encode_params(const char **names, const double *vals, const int32_t *kinds, int32_t n, char *buf, int64_t cap) {
    gob::Entries e;
    for (int32_t k = 0; k < n; k++) {
        gob::Value v = kinds[k] == 0 ? gob::Value::of_int((int64_t)vals[k]) : gob::Value::of_float(vals[k]);
        if (kinds[k] == 2) v.kind = gob::Value::Bool, v.b = vals[k] != 0;
        e.emplace_back(names[k], v);
    }
    return copy_out(gob::encode_map("Params", e), buf, cap);
}
// decoded entries as "name\tkind\tvalue" lines
int64_t gh_gob_decode_params(const char *buf, int64_t n, char *out, int64_t cap) {
    std::string text;
    int32_t rc = guard([&] {
        for (auto &kv : gob::decode_map(std::string(buf, (size_t)n))) {
            char num[64];
            snprintf(num, sizeof(num), "%.17g", kv.second.number());
            text += kv.first + "\t" + std::to_string((int)kv.second.kind) + "\t" +
                    (kv.second.kind == gob::Value::String ? kv.second.s : std::string(num)) + "\n";
        }
    });
    return rc != 0 ? rc : copy_out(text, out, cap);
}
// the worked example of the encoding/gob documentation, type Point struct{ X, Y int } holding {22, 33}, rebuilt from the
// primitives: the definition of type 65 (a structType with two int fields), then the value
int64_t gh_gob_doc_example(char *buf, int64_t cap) {
    std::string def;
    gob::put_int(def, -65);
    gob::put_uint(def, 3);  // wireType.StructT
    gob::put_uint(def, 1);  // CommonType
    gob::put_uint(def, 1);
    gob::put_string(def, "Point");
    gob::put_uint(def, 1);
    gob::put_int(def, 65);
    gob::put_uint(def, 0);
    gob::put_uint(def, 1);  // Field
    gob::put_uint(def, 2);  // two fieldTypes
    for (const char *f : {"X", "Y"}) {
        gob::put_uint(def, 1);
        gob::put_string(def, f);
        gob::put_uint(def, 1);
        gob::put_int(def, gob::tInt);
        gob::put_uint(def, 0);
    }
    gob::put_uint(def, 0);
    gob::put_uint(def, 0);
    std::string val;
    gob::put_int(val, 65);
    gob::put_uint(val, 1);
    gob::put_int(val, 22);
    gob::put_uint(val, 1);
    gob::put_int(val, 33);
    gob::put_uint(val, 0);
    return copy_out(gob::message(def) + gob::message(val), buf, cap);
}
void *gh_mfusers_new() { return new logics::MatrixFactorizationUsers(); }
void gh_mfusers_free(void *u) { delete (logics::MatrixFactorizationUsers *)u; }
void gh_mfusers_add(void *u, const char *id, const float *v, int32_t d) {
    ((logics::MatrixFactorizationUsers *)u)->Add(id, std::vector<float>(v, v + d));
}
int32_t gh_mfusers_get(void *u, const char *id, float *out, int32_t cap) {
    std::vector<float> v;
    if (!((logics::MatrixFactorizationUsers *)u)->Get(id, v)) return -1;
    for (size_t t = 0; t < v.size() && (int32_t)t < cap; t++) out[t] = v[t];
    return (int32_t)v.size();
}
int64_t gh_mfusers_marshal(void *u, char *buf, int64_t cap) {
    return copy_out(((logics::MatrixFactorizationUsers *)u)->Marshal(), buf, cap);
}
int32_t gh_mfusers_unmarshal(void *u, const char *buf, int64_t n) {
    return guard([&] { ((logics::MatrixFactorizationUsers *)u)->Unmarshal(std::string(buf, (size_t)n)); });
}

// ---- heap ----------------------------------------------------------------------------------------
int32_t gh_topk_filter(int32_t k, const int32_t *items, const float *weights, int32_t n, int32_t *out_items, float *out_w) {
    heap::TopKFilter f(k);
    for (int32_t t = 0; t < n; t++) f.Push(items[t], weights[t]);
    auto r = f.PopAll();
    for (size_t t = 0; t < r.size(); t++) out_items[t] = r[t].Value, out_w[t] = r[t].Weight;
    return (int32_t)r.size();
}
int32_t gh_pq_drain(int32_t desc, int32_t reverse, const int32_t *items, const float *weights, int32_t n, int32_t *out_items,
                    float *out_w) {
    int32_t cnt = 0;
    int32_t rc = guard([&] {
        heap::PriorityQueue pq(desc != 0);
        for (int32_t t = 0; t < n; t++) pq.Push(items[t], weights[t]);
        heap::PriorityQueue q = reverse ? pq.Reverse() : pq.Clone();
        while (q.Len() > 0) {
            auto e = q.Pop();
            out_items[cnt] = e.first, out_w[cnt] = e.second, cnt++;
        }
    });
    return rc < 0 ? rc : cnt;
}

// ---- ann.Bruteforce ---------------------------------------------------------------------------------
void *gh_bruteforce_new(int32_t metric) { return new ann::Bruteforce(metric); }
void gh_bruteforce_free(void *b) { delete (ann::Bruteforce *)b; }
int32_t gh_bruteforce_add(void *b, const float *v, int32_t d, int32_t *ret) {
    return guard([&] { *ret = ((ann::Bruteforce *)b)->Add(std::vector<float>(v, v + d)); });
}
int32_t gh_bruteforce_search_index(void *b, int32_t q, int32_t k, int32_t prune0, int32_t *idx, float *dist, int32_t *cnt) {
    return guard([&] {
        auto r = ((ann::Bruteforce *)b)->SearchIndex(q, k, prune0 != 0);
        *cnt = (int32_t)r.size();
        for (size_t t = 0; t < r.size(); t++) idx[t] = r[t].first, dist[t] = r[t].second;
    });
}
int32_t gh_bruteforce_search_vector(void *b, const float *q, int32_t d, int32_t k, int32_t prune0, int32_t *idx, float *dist,
                                    int32_t *cnt) {
    return guard([&] {
        auto r = ((ann::Bruteforce *)b)->SearchVector(std::vector<float>(q, q + d), k, prune0 != 0);
        *cnt = (int32_t)r.size();
        for (size_t t = 0; t < r.size(); t++) idx[t] = r[t].first, dist[t] = r[t].second;
    });
}

// ---- vectors.Database ("hip://") ----------------------------------------------------------------------
// Vectors cross the boundary one field at a time through a thread-local staging list: *_stage_* fill it before
// AddVectors, GetVectors / QueryVectors leave their results in it for the gh_vdb_result_* readers.
namespace {
typedef int32_t (*gh_search_cb)(const float *X, int64_t n, int32_t d, int32_t metric, const float *Q, int64_t nq, int32_t k,
                                int32_t *idx, float *dist, int32_t *cnt);
struct CallbackSearcher : vectors::Searcher {  // the CPU test-suite's checker (an exact search built on the oracle)
    gh_search_cb cb;
    explicit CallbackSearcher(gh_search_cb c) : cb(c) {}
    void invalidate(const std::string &) override {}
    void search(const std::string &, const float *X, int64_t n, int d, int metric, const float *Q, int64_t nq, int k,
                int32_t *idx, float *dist, int32_t *cnt) override {
        if (cb(X, n, d, metric, Q, nq, k, idx, dist, cnt) != 0) throw std::runtime_error("search callback failed");
    }
};
typedef int32_t (*gh_sparse_search_cb)(int64_t n, const int64_t *indptr, const uint32_t *indices, const float *values,
                                       const uint8_t *admissible, int64_t nq, const int64_t *q_indptr, const uint32_t *q_indices,
                                       const float *q_values, int32_t k, int32_t *idx, float *score, int32_t *cnt);
struct CallbackSparseSearcher : vectors::SparseSearcher {  // the CPU test-suite's checker for sparse collections
    gh_sparse_search_cb cb;
    explicit CallbackSparseSearcher(gh_sparse_search_cb c) : cb(c) {}
    void invalidate(const std::string &) override {}
    void search(const std::string &, int64_t n, const int64_t *indptr, const uint32_t *indices, const float *values,
                const uint8_t *admissible, int64_t nq, const int64_t *q_indptr, const uint32_t *q_indices, const float *q_values,
                int k, int32_t *idx, float *score, int32_t *cnt) override {
        if (cb(n, indptr, indices, values, admissible, nq, q_indptr, q_indices, q_values, k, idx, score, cnt) != 0)
            throw std::runtime_error("sparse search callback failed");
    }
};
struct VdbHandle {
    std::shared_ptr<vectors::HipDatabase> db;
};
thread_local std::vector<vectors::ScoredVector> g_stage;
thread_local std::vector<int64_t> g_stage_split;  // batch queries: result t is g_stage[split[t] .. split[t+1])
std::vector<std::string> split_lines(const char *s) {
    std::vector<std::string> out;
    if (!s || !*s) return out;
    std::string cur;
    for (const char *p = s;; p++) {
        if (*p == '\n' || *p == 0) {
            out.push_back(cur);
            cur.clear();
            if (*p == 0) break;
        } else {
            cur.push_back(*p);
        }
    }
    return out;
}
vectors::HipDatabase &vdb(void *h) { return *((VdbHandle *)h)->db; }
}  // namespace

// MatrixFactorizationItems (logics/cf.go:36-128); cb = a search callback (the CPU test-suite's checker) or NULL for the GPU
void *gh_mfitems_new(int64_t timestamp_unix_nanos, gh_search_cb cb) {
    std::shared_ptr<vectors::Searcher> s;
    if (cb) s = std::make_shared<CallbackSearcher>(cb);
    return new logics::MatrixFactorizationItems(timestamp_unix_nanos, s);
}
void gh_mfitems_free(void *m) { delete (logics::MatrixFactorizationItems *)m; }
void gh_mfitems_add(void *m, const char *id, const float *v, int32_t d) {
    ((logics::MatrixFactorizationItems *)m)->Add(id, std::vector<float>(v, v + d));
}
int64_t gh_mfitems_count(void *m) { return (int64_t)((logics::MatrixFactorizationItems *)m)->Count(); }
int32_t gh_mfitems_dimension(void *m) { return ((logics::MatrixFactorizationItems *)m)->Dimension(); }
int64_t gh_mfitems_timestamp(void *m) { return ((logics::MatrixFactorizationItems *)m)->Timestamp(); }
int64_t gh_mfitems_id(void *m, int64_t i, char *buf, int64_t cap) {
    return copy_out(((logics::MatrixFactorizationItems *)m)->Id((size_t)i), buf, cap);
}
void gh_mfitems_row(void *m, int64_t i, float *out) {
    auto *x = (logics::MatrixFactorizationItems *)m;
    std::memcpy(out, x->Row((size_t)i), (size_t)x->Dimension() * sizeof(float));
}
int64_t gh_mfitems_marshal(void *m, char *buf, int64_t cap) {
    return copy_out(((logics::MatrixFactorizationItems *)m)->Marshal(), buf, cap);
}
// the blob with the reference's own index section and a device-built graph (MarshalReference); called twice by the ctypes wrapper
// (size, then content): the bytes of the first call are kept until the second has copied them
int64_t gh_mfitems_marshal_reference(void *m, char *buf, int64_t cap) {
    // kept for: the object AND the state it was marshalled from (items added between the two calls make a fresh blob)
    static thread_local std::string kept;
    static thread_local void *kept_for = nullptr;
    static thread_local size_t kept_count = 0;
    static thread_local int64_t kept_stamp = 0;
    int64_t out = -1;
    guard([&] {
        auto *items = (logics::MatrixFactorizationItems *)m;
        if (!(buf && kept_for == m && kept_count == items->Count() && kept_stamp == items->Timestamp() && (int64_t)kept.size() <= cap)) {
            kept = items->MarshalReference();
            kept_for = m;
            kept_count = items->Count();
            kept_stamp = items->Timestamp();
        }
        out = copy_out(kept, buf, cap);
        if (buf) {
            kept.clear();
            kept_for = nullptr;
        }
    });
    return out;
}
int32_t gh_mfitems_unmarshal(void *m, const char *buf, int64_t n) {
    return guard([&] { ((logics::MatrixFactorizationItems *)m)->Unmarshal(std::string(buf, (size_t)n)); });
}
// Search: ids joined by '\n' into ids_buf (returns the byte count), scores into scores[0..cap_scores); *n_out = results
int64_t gh_mfitems_search(void *m, const float *v, int32_t d, int32_t n, char *ids_buf, int64_t cap, double *scores,
                          int32_t cap_scores, int32_t *n_out) {
    int64_t bytes = -1;
    const int32_t rc = guard([&] {
        auto res = ((logics::MatrixFactorizationItems *)m)->Search(std::vector<float>(v, v + d), n);
        std::string joined;
        for (size_t t = 0; t < res.size(); t++) {
            if (t) joined.push_back('\n');
            joined += res[t].Id;
            if ((int32_t)t < cap_scores) scores[t] = res[t].Value;
        }
        *n_out = (int32_t)res.size();
        bytes = copy_out(joined, ids_buf, cap);
    });
    return rc == 0 ? bytes : -1;
}
int64_t gh_gob_f32_slice(const float *v, int32_t n, char *buf, int64_t cap) { return copy_out(gob::encode_f32_slice(v, (size_t)n), buf, cap); }

void *gh_vdb_open(const char *url) {
    void *out = nullptr;
    guard([&] { out = new VdbHandle{vectors::Open(url)}; });
    return out;
}
void *gh_vdb_open_with_searcher(gh_search_cb cb) {
    return new VdbHandle{std::make_shared<vectors::HipDatabase>(std::make_shared<CallbackSearcher>(cb))};
}
void *gh_vdb_open_with_searchers(gh_search_cb cb, gh_sparse_search_cb scb) {
    std::shared_ptr<vectors::Searcher> dense;
    std::shared_ptr<vectors::SparseSearcher> sparse;
    if (cb) dense = std::make_shared<CallbackSearcher>(cb);
    if (scb) sparse = std::make_shared<CallbackSparseSearcher>(scb);
    return new VdbHandle{std::make_shared<vectors::HipDatabase>(dense, sparse)};
}
void gh_vdb_free(void *h) { delete (VdbHandle *)h; }
int32_t gh_vdb_close(void *h) { return guard([&] { vdb(h).Close(); }); }
int32_t gh_vdb_add_collection(void *h, const char *name, int32_t dim, int32_t distance, const char *qtype, int32_t bits) {
    return guard([&] {
        vectors::VectorConfig cfg;
        cfg.Type = qtype ? qtype : "";
        cfg.Bits = bits;
        vdb(h).AddCollection(name, dim, (vectors::Distance)distance, cfg);
    });
}
int32_t gh_vdb_delete_collection(void *h, const char *name) { return guard([&] { vdb(h).DeleteCollection(name); }); }
int32_t gh_vdb_describe(void *h, const char *name, int32_t *dim, int32_t *distance, int32_t *bits) {
    return guard([&] {
        auto info = vdb(h).DescribeCollection(name);
        *dim = info.Dimension;
        *distance = (int32_t)info.Dist;
        *bits = info.Config.Bits;
    });
}
// '\n'-joined names into buf (NUL-terminated); returns the length needed or a negative error
int64_t gh_vdb_list(void *h, char *buf, int64_t cap) {
    std::string joined;
    int32_t rc = guard([&] {
        for (auto &n : vdb(h).ListCollections()) joined += (joined.empty() ? "" : "\n") + n;
    });
    if (rc != 0) return rc;
    if ((int64_t)joined.size() + 1 <= cap) std::memcpy(buf, joined.c_str(), joined.size() + 1);
    return (int64_t)joined.size() + 1;
}
int64_t gh_vdb_count(void *h, const char *name) {
    int64_t n = 0;
    int32_t rc = guard([&] { n = vdb(h).CountVectors(name); });
    return rc != 0 ? rc : n;
}
void gh_vdb_stage_clear() {
    g_stage.clear();
    g_stage_split.clear();
}
void gh_vdb_stage_vector(const char *id, const float *values, int32_t n_values, const uint32_t *indices, int32_t n_indices,
                         int32_t hidden, const char *categories, int64_t timestamp_ms) {
    vectors::ScoredVector v;
    v.Id = id;
    v.Values.assign(values, values + n_values);
    if (n_indices > 0) v.Indices.assign(indices, indices + n_indices);
    v.IsHidden = hidden != 0;
    v.Categories = split_lines(categories);
    v.TimestampMs = timestamp_ms;
    g_stage.push_back(std::move(v));
}
int32_t gh_vdb_add_staged(void *h, const char *name) {
    return guard([&] {
        std::vector<vectors::Vector> vs(g_stage.begin(), g_stage.end());
        g_stage.clear();
        vdb(h).AddVectors(name, vs);
    });
}
int32_t gh_vdb_get(void *h, const char *name, const char *ids) {
    return guard([&] {
        gh_vdb_stage_clear();
        for (auto &v : vdb(h).GetVectors(name, split_lines(ids))) {
            vectors::ScoredVector s;
            static_cast<vectors::Vector &>(s) = v;
            g_stage.push_back(std::move(s));
        }
    });
}
int32_t gh_vdb_delete_vectors(void *h, const char *name, int64_t timestamp_ms) {
    return guard([&] { vdb(h).DeleteVectors(name, timestamp_ms); });
}
// the query is the LAST staged vector (dense Values, or Indices + Values for a sparse collection); results replace the staging list
int32_t gh_vdb_query_staged(void *h, const char *name, const char *categories, int32_t topk) {
    return guard([&] {
        if (g_stage.empty()) throw std::invalid_argument("no staged query vector");
        vectors::Vector q = g_stage.back();
        gh_vdb_stage_clear();
        g_stage = vdb(h).QueryVectors(name, q, split_lines(categories), topk);
    });
}
int32_t gh_vdb_query_batch(void *h, const char *name, const float *Q, int64_t nq, int32_t d, const char *categories,
                           int32_t topk) {
    return guard([&] {
        gh_vdb_stage_clear();
        auto res = vdb(h).QueryVectorsBatch(name, std::vector<float>(Q, Q + nq * d), nq, split_lines(categories), topk);
        g_stage_split.push_back(0);
        for (auto &r : res) {
            for (auto &v : r) g_stage.push_back(std::move(v));
            g_stage_split.push_back((int64_t)g_stage.size());
        }
    });
}
// every staged vector is one sparse query; results replace the staging list, split per query
int32_t gh_vdb_query_sparse_staged(void *h, const char *name, const char *categories, int32_t topk) {
    return guard([&] {
        std::vector<vectors::Vector> qs(g_stage.begin(), g_stage.end());
        gh_vdb_stage_clear();
        auto res = vdb(h).QuerySparseBatch(name, qs, split_lines(categories), topk);
        g_stage_split.push_back(0);
        for (auto &r : res) {
            for (auto &v : r) g_stage.push_back(std::move(v));
            g_stage_split.push_back((int64_t)g_stage.size());
        }
    });
}
int32_t gh_vdb_result_nnz(int64_t r) { return (int32_t)g_stage[(size_t)r].Indices.size(); }
void gh_vdb_result_indices(int64_t r, uint32_t *out) {
    std::copy(g_stage[(size_t)r].Indices.begin(), g_stage[(size_t)r].Indices.end(), out);
}
int64_t gh_vdb_result_count() { return (int64_t)g_stage.size(); }
int64_t gh_vdb_result_split(int64_t t) { return t >= 0 && t < (int64_t)g_stage_split.size() ? g_stage_split[(size_t)t] : -1; }
const char *gh_vdb_result_id(int64_t r) { return g_stage[(size_t)r].Id.c_str(); }
float gh_vdb_result_score(int64_t r) { return g_stage[(size_t)r].Score; }
int32_t gh_vdb_result_hidden(int64_t r) { return g_stage[(size_t)r].IsHidden ? 1 : 0; }
int64_t gh_vdb_result_timestamp(int64_t r) { return g_stage[(size_t)r].TimestampMs; }
int32_t gh_vdb_result_dim(int64_t r) { return (int32_t)g_stage[(size_t)r].Values.size(); }
void gh_vdb_result_values(int64_t r, float *out) {
    std::copy(g_stage[(size_t)r].Values.begin(), g_stage[(size_t)r].Values.end(), out);
}
int64_t gh_vdb_result_categories(int64_t r, char *buf, int64_t cap) {
    std::string joined;
    for (auto &c : g_stage[(size_t)r].Categories) joined += (joined.empty() ? "" : "\n") + c;
    if ((int64_t)joined.size() + 1 <= cap) std::memcpy(buf, joined.c_str(), joined.size() + 1);
    return (int64_t)joined.size() + 1;
}

// ---- logics: embedding item-to-item / user-to-user over a vectors.Database ----------------------------------
void *gh_vwriter_new(void *h, const char *collection, int32_t distance, int64_t timestamp_ms, int32_t batch) {
    return new logics::VectorWriter(((VdbHandle *)h)->db, collection, (vectors::Distance)distance, timestamp_ms, batch);
}
void *gh_vwriter_new_sparse(void *h, const char *collection, int64_t timestamp_ms, int32_t batch) {  // distance Dot
    return new logics::VectorWriter(((VdbHandle *)h)->db, collection, vectors::Dot, timestamp_ms, batch, true);
}
void gh_vwriter_free(void *w) { delete (logics::VectorWriter *)w; }
// stage the vector a sparse kind writes for one item / user: kind 0 = tags, 1 = feedback (users / items), 2 = auto
void gh_logics_stage_kind_vector(int32_t kind, const char *id, int32_t hidden, const char *categories, int64_t timestamp_ms,
                                 const int32_t *tags, int32_t n_tags, const float *tags_idf, int32_t n_tags_idf,
                                 const int32_t *feedback, int32_t n_feedback, const float *fb_idf, int32_t n_fb_idf) {
    vectors::Vector meta;
    meta.Id = id;
    meta.IsHidden = hidden != 0;
    meta.Categories = split_lines(categories);
    meta.TimestampMs = timestamp_ms;
    std::vector<int32_t> t(tags, tags + n_tags), f(feedback, feedback + n_feedback);
    std::vector<float> ti(tags_idf, tags_idf + n_tags_idf), fi(fb_idf, fb_idf + n_fb_idf);
    vectors::ScoredVector v;
    static_cast<vectors::Vector &>(v) = kind == 0   ? logics::tagsVector(meta, t, ti)
                                        : kind == 1 ? logics::feedbackVector(meta, f, fi)
                                                    : logics::autoVector(meta, t, ti, f, fi);
    g_stage.push_back(std::move(v));
}
// the vector to add is the LAST staged one
int32_t gh_vwriter_add_staged(void *w) {
    return guard([&] {
        if (g_stage.empty()) throw std::invalid_argument("no staged vector");
        vectors::Vector v = g_stage.back();
        gh_vdb_stage_clear();
        ((logics::VectorWriter *)w)->Add(v);
    });
}
int32_t gh_vwriter_clean(void *w) { return guard([&] { ((logics::VectorWriter *)w)->Clean(); }); }
// results: staged as ScoredVector with Score = the cache.Score value (double narrowed for transport is NOT wanted: see
// gh_logics_result_score)
namespace {
thread_local std::vector<double> g_scores;
void stage_scores(const std::vector<std::vector<logics::Score>> &res) {
    gh_vdb_stage_clear();
    g_scores.clear();
    g_stage_split.push_back(0);
    for (auto &r : res) {
        for (auto &sc : r) {
            vectors::ScoredVector v;
            v.Id = sc.Id;
            v.Categories = sc.Categories;
            g_stage.push_back(std::move(v));
            g_scores.push_back(sc.Value);
        }
        g_stage_split.push_back((int64_t)g_stage.size());
    }
}
}  // namespace
int32_t gh_logics_query_similar(void *h, const char *collection, const char *id, const char *categories, int32_t n) {
    return guard([&] { stage_scores({logics::QuerySimilar(vdb(h), collection, id, split_lines(categories), n)}); });
}
int32_t gh_logics_query_similar_bulk(void *h, const char *collection, const char *ids, const char *categories, int32_t n) {
    return guard([&] { stage_scores(logics::QuerySimilarBulk(vdb(h), collection, split_lines(ids), split_lines(categories), n)); });
}
int32_t gh_logics_query_similar_typed(void *h, const char *collection, const char *type, const char *id, const char *categories,
                                      int32_t n) {
    return guard([&] { stage_scores({logics::QuerySimilarTyped(vdb(h), collection, type, id, split_lines(categories), n)}); });
}
int32_t gh_logics_query_similar_typed_bulk(void *h, const char *collection, const char *type, const char *ids,
                                           const char *categories, int32_t n) {
    return guard([&] {
        stage_scores(logics::QuerySimilarTypedBulk(vdb(h), collection, type, split_lines(ids), split_lines(categories), n));
    });
}
double gh_logics_result_score(int64_t r) { return g_scores[(size_t)r]; }

// MatrixFactorization::RecommendUnseen: user ids '\n'-joined; seen = NULL (no lists given) or CSR over ITEM INDICES (seen_ptr n_users + 1);
// item_ok: one byte per item index or NULL.  items_out (item indices, padded with -1) and scores_out are n_users x n, count_out n_users.
int32_t gh_model_recommend_unseen(void *m, const char *user_ids, int64_t n_users, int32_t n, const int64_t *seen_ptr,
                                  const int32_t *seen_items, const uint8_t *item_ok, int32_t n_item_ok, int32_t *items_out,
                                  float *scores_out, int32_t *count_out) {
    return guard([&] {
        auto *mf = (cf::MatrixFactorization *)m;
        if (mf->Invalid()) throw std::runtime_error("model is not fitted");
        std::vector<std::string> ids = split_lines(user_ids);
        ids.resize((size_t)n_users);
        std::vector<int32_t> users((size_t)n_users);
        for (int64_t t = 0; t < n_users; t++) users[(size_t)t] = mf->UserIndex->Id(ids[(size_t)t]);
        std::vector<int64_t> ptr;
        std::vector<int32_t> flat;
        if (seen_ptr) {
            ptr.assign(seen_ptr, seen_ptr + n_users + 1);
            flat.assign(seen_items, seen_items + ptr.back());
        }
        std::vector<bool> ok(item_ok, item_ok + (item_ok ? n_item_ok : 0));
        std::vector<int32_t> items, count;
        std::vector<float> scores;
        mf->RecommendUnseenIndexed(users, n, ptr, flat, ok, items, scores, count);
        std::copy(items.begin(), items.end(), items_out);
        std::copy(scores.begin(), scores.end(), scores_out);
        std::copy(count.begin(), count.end(), count_out);
    });
}
int32_t gh_model_holds_training_rows(void *m) { return ((cf::MatrixFactorization *)m)->HandleHoldsTrainingRows(); }

// users: Q is n_users x d; excludes: one '\n'-joined id list per user, users separated by '\x1e' (record separator)
namespace {
std::vector<logics::UserQuery> parse_user_queries(const float *Q, int64_t n_users, int32_t d, const char *excludes) {
    std::vector<logics::UserQuery> users((size_t)n_users);
    std::vector<std::string> per_user;
    std::string cur;
    for (const char *p = excludes ? excludes : "";; p++) {
        if (*p == '\x1e' || *p == 0) {
            per_user.push_back(cur);
            cur.clear();
            if (*p == 0) break;
        } else {
            cur.push_back(*p);
        }
    }
    for (int64_t t = 0; t < n_users; t++) {
        users[(size_t)t].Embedding.assign(Q + t * d, Q + (t + 1) * d);
        if ((size_t)t < per_user.size()) users[(size_t)t].Exclude = split_lines(per_user[(size_t)t].c_str());
    }
    return users;
}
}  // namespace
int32_t gh_logics_cf_recommend_bulk(void *h, const char *collection, const float *Q, int64_t n_users, int32_t d,
                                    const char *excludes, int32_t cache_size) {
    return guard([&] { stage_scores(logics::CollaborativeRecommendBulk(vdb(h), collection, parse_user_queries(Q, n_users, d, excludes), cache_size)); });
}
int32_t gh_logics_cf_recommend_unseen(void *h, const char *collection, const float *Q, int64_t n_users, int32_t d,
                                      const char *excludes, int32_t cache_size) {
    return guard([&] { stage_scores(logics::CollaborativeRecommendUnseen(vdb(h), collection, parse_user_queries(Q, n_users, d, excludes), cache_size)); });
}
// The neighbourhood recommenders (logics::ItemToItemRecommend / UserToUserRecommend and their Bulk forms).  Lists of lists travel as
// '\n'-joined ids per record, records separated by '\x1e'.  user_to_user = 0: positives = one record per user; user_to_user = 1:
// user_ids = one id per user, feedback_users / feedback_items = the data store's positive feedback (one record per feedback user).
namespace {
std::vector<std::vector<std::string>> split_records(const char *s) {
    std::vector<std::vector<std::string>> out;
    std::string cur;
    for (const char *p = s ? s : "";; p++) {
        if (*p == '\x1e' || *p == 0) {
            out.push_back(split_lines(cur.c_str()));
            cur.clear();
            if (*p == 0) break;
        } else {
            cur.push_back(*p);
        }
    }
    return out;
}
}  // namespace
int32_t gh_logics_nbr_recommend(void *h, int32_t user_to_user, int32_t bulk, const char *collection, const char *type, int64_t n_users,
                                const char *user_ids, const char *positives, const char *excludes, const char *feedback_users,
                                const char *feedback_items, const char *categories, int32_t cache_size) {
    return guard([&] {
        std::vector<logics::NbrUser> users((size_t)n_users);
        const auto ids = split_lines(user_ids);
        const auto pos = split_records(positives), exc = split_records(excludes), fbi = split_records(feedback_items);
        for (size_t t = 0; t < users.size(); t++) {
            if (t < ids.size()) users[t].Id = ids[t];
            if (t < pos.size()) users[t].Positives = pos[t];
            if (t < exc.size()) users[t].Exclude = exc[t];
        }
        logics::FeedbackMap feedback;
        const auto fbu = split_lines(feedback_users);
        for (size_t r = 0; r < fbu.size(); r++) feedback[fbu[r]] = r < fbi.size() ? fbi[r] : std::vector<std::string>();
        const auto cats = split_lines(categories);
        if (bulk) {
            stage_scores(user_to_user ? logics::UserToUserRecommendBulk(vdb(h), collection, type, users, feedback, cache_size)
                                      : logics::ItemToItemRecommendBulk(vdb(h), collection, type, users, cats, cache_size));
            return;
        }
        std::vector<std::vector<logics::Score>> res;
        for (const auto &u : users)
            res.push_back(user_to_user ? logics::UserToUserRecommend(vdb(h), collection, type, u, feedback, cache_size)
                                       : logics::ItemToItemRecommend(vdb(h), collection, type, u, cats, cache_size));
        stage_scores(res);
    });
}
// logics::RecommendSequential / RecommendSequentialBulk.  The stages are staged one call each, in the recommenders' order, then run:
//   gh_logics_seq_add_lists  shared = 0: one record of ids per user (recommendCollaborative / recommendExternal), shared = 1: one record for
//                            everybody (recommendLatest / recommendNonPersonalized); scores = one double per id, in record order
//   gh_logics_seq_add_nbr    recommendItemToItem (user_to_user = 0) / recommendUserToUser over a collection; feedback as in gh_logics_nbr_recommend
//   gh_logics_seq_run        bulk = 0: the per-user loop, bulk = 1: one candidate chain for all users; results staged like every logics call
namespace {
thread_local std::vector<logics::SeqStage> g_seq;
}
void gh_logics_seq_clear() { g_seq.clear(); }
int32_t gh_logics_seq_add_lists(int32_t shared, int32_t cache_size, const char *ids, const double *scores, int64_t n_scores) {
    return guard([&] {
        logics::SeqStage st;
        st.kind = shared ? logics::SeqStage::Shared : logics::SeqStage::Lists;
        st.CacheSize = cache_size;
        int64_t e = 0;
        for (const auto &rec : split_records(ids)) {
            std::vector<logics::Score> l;
            for (const std::string &id : rec) {
                if (e >= n_scores) throw std::invalid_argument("fewer scores than ids");
                logics::Score sc;
                sc.Id = id;
                sc.Value = scores[e++];
                l.push_back(std::move(sc));
            }
            if (shared) {
                st.shared = std::move(l);
                break;
            }
            st.lists.push_back(std::move(l));
        }
        g_seq.push_back(std::move(st));
    });
}
int32_t gh_logics_seq_add_nbr(int32_t user_to_user, int32_t cache_size, const char *collection, const char *type, const char *categories,
                              const char *feedback_users, const char *feedback_items) {
    return guard([&] {
        logics::SeqStage st;
        st.kind = user_to_user ? logics::SeqStage::UserToUser : logics::SeqStage::ItemToItem;
        st.CacheSize = cache_size;
        st.collection = collection;
        st.type = type;
        st.categories = split_lines(categories);
        const auto fbu = split_lines(feedback_users);
        const auto fbi = split_records(feedback_items);
        for (size_t r = 0; r < fbu.size(); r++) st.feedback[fbu[r]] = r < fbi.size() ? fbi[r] : std::vector<std::string>();
        g_seq.push_back(std::move(st));
    });
}
int32_t gh_logics_seq_run(void *h, int32_t bulk, int64_t n_users, const char *user_ids, const char *positives, const char *excludes) {
    return guard([&] {
        std::vector<logics::NbrUser> users((size_t)n_users);
        const auto ids = split_lines(user_ids);
        const auto pos = split_records(positives), exc = split_records(excludes);
        for (size_t t = 0; t < users.size(); t++) {
            if (t < ids.size()) users[t].Id = ids[t];
            if (t < pos.size()) users[t].Positives = pos[t];
            if (t < exc.size()) users[t].Exclude = exc[t];
        }
        for (auto &st : g_seq)
            if (st.kind == logics::SeqStage::Lists) st.lists.resize(users.size());
        if (bulk) {
            stage_scores(logics::RecommendSequentialBulk(vdb(h), users, g_seq));
            return;
        }
        std::vector<std::vector<logics::Score>> res;
        for (size_t t = 0; t < users.size(); t++) res.push_back(logics::RecommendSequential(vdb(h), users[t], g_seq, t));
        stage_scores(res);
    });
}
// logics::AddReplacementCandidates / ApplyReplacementDecay / RecommendWithReplacement for one user.  Ids travel '\n'-joined, the
// scores and the feedback kinds (1 positive, 2 read) as arrays in id order.
//   gh_logics_replacement_add     stages three lists: the grown candidates, positiveExisting and negativeItems (scores 0)
//   gh_logics_replacement_decay   stages the decayed, re-sorted results
//   gh_logics_replacement_run     the whole body; scorer(item id) = the ranker's float32 score of that candidate
namespace {
std::vector<logics::Score> scored_ids(const char *ids, const double *scores, int64_t n) {
    std::vector<logics::Score> out;
    for (const std::string &id : split_lines(ids)) {
        logics::Score sc;
        sc.Id = id;
        if ((int64_t)out.size() < n && scores) sc.Value = scores[out.size()];
        out.push_back(std::move(sc));
    }
    return out;
}
std::vector<logics::ReplacementFeedback> feedback_of(const char *items, const uint8_t *kinds, int64_t n) {
    std::vector<logics::ReplacementFeedback> out;
    for (const std::string &id : split_lines(items)) {
        if ((int64_t)out.size() >= n) throw std::invalid_argument("fewer kinds than feedback items");
        out.push_back({id, (int)kinds[out.size()]});
    }
    return out;
}
std::set<std::string> id_set(const char *ids) {
    const auto v = split_lines(ids);
    return std::set<std::string>(v.begin(), v.end());
}
std::vector<logics::Score> as_scores(const std::set<std::string> &ids) {
    std::vector<logics::Score> out;
    for (const std::string &id : ids) {
        logics::Score sc;
        sc.Id = id;
        out.push_back(std::move(sc));
    }
    return out;
}
}  // namespace
int32_t gh_logics_replacement_add(const char *cand_ids, const double *cand_scores, int64_t n_cand, const char *fb_items, const uint8_t *fb_kinds,
                                  int64_t n_fb, const char *existing) {
    return guard([&] {
        const auto r = logics::AddReplacementCandidates(scored_ids(cand_ids, cand_scores, n_cand), feedback_of(fb_items, fb_kinds, n_fb), id_set(existing));
        stage_scores({r.Candidates, as_scores(r.Positive), as_scores(r.Negative)});
    });
}
int32_t gh_logics_replacement_decay(const char *ids, const double *scores, int64_t n, const char *positive, const char *negative,
                                    double positive_decay, double read_decay) {
    return guard([&] {
        stage_scores({logics::ApplyReplacementDecay(scored_ids(ids, scores, n), id_set(positive), id_set(negative), positive_decay, read_decay)});
    });
}
int32_t gh_logics_replacement_run(const char *cand_ids, const double *cand_scores, int64_t n_cand, const char *fb_items, const uint8_t *fb_kinds,
                                  int64_t n_fb, const char *existing, float (*scorer)(const char *), double positive_decay, double read_decay) {
    return guard([&] {
        auto ranker = [&](const std::vector<logics::Score> &c) {
            std::vector<float> out;
            for (const logics::Score &sc : c) out.push_back(scorer(sc.Id.c_str()));
            return out;
        };
        stage_scores({logics::RecommendWithReplacement(scored_ids(cand_ids, cand_scores, n_cand), feedback_of(fb_items, fb_kinds, n_fb),
                                                       id_set(existing), ranker, positive_decay, read_decay)});
    });
}
// HipDatabase::SetNbrTableFromIndex: slot `which` of the gorse_nbr handle `nbr` from the collection's resident index; the row
// numbering (ids in row order) is staged like a query's results
int32_t gh_vdb_set_nbr_table_from_index(void *h, const char *collection, void *nbr, int32_t which, const char *type, const char *categories,
                                        int32_t n) {
    return guard([&] {
        const auto ids = vdb(h).SetNbrTableFromIndex(collection, (gorse_nbr *)nbr, which, type, split_lines(categories), n);
        g_stage.clear();
        g_stage_split.clear();
        for (const std::string &id : ids) {
            vectors::ScoredVector v;
            v.Id = id;
            g_stage.push_back(std::move(v));
        }
    });
}
// master/tasks.go:925-969: items of model `m` into collaborative_filtering_<model_id> of database `h`, users into a new
// MatrixFactorizationUsers (returned; free with gh_mfusers_free).  hidden: one byte per item or NULL; categories: one
// '\n'-joined list per item, items separated by '\x1e', or NULL
void *gh_publish_cf(void *m, void *h, int64_t model_id, const uint8_t *hidden, int32_t n_hidden, const char *categories,
                    int32_t batch) {
    void *out = nullptr;
    guard([&] {
        std::vector<bool> hid(hidden, hidden + (hidden ? n_hidden : 0));
        std::vector<std::vector<std::string>> cats;
        if (categories) {
            std::string cur;
            for (const char *p = categories;; p++) {
                if (*p == '\x1e' || *p == 0) {
                    cats.push_back(split_lines(cur.c_str()));
                    cur.clear();
                    if (*p == 0) break;
                } else {
                    cur.push_back(*p);
                }
            }
        }
        auto users = logics::PublishCollaborativeFiltering(*(cf::MatrixFactorization *)m, vdb(h), model_id, hid, cats, batch > 0 ? batch : 1024);
        out = new logics::MatrixFactorizationUsers(std::move(users));
    });
    return out;
}
int32_t gh_mfusers_count(void *u) { return (int32_t)((logics::MatrixFactorizationUsers *)u)->Count(); }

// CPU test hook for the ranking kernels' integer encodings (csrc/rank_keys.hpp, the very header the kernels include):
// what = 0 fkey, 1 fkey_inv(fkey), 2 dist_key, 3 dist_from_key(dist_key, -0 flag), 4 score_ord, 5 key_score(make_key(score_ord, row))
// -> out_u32[i]; 6 key_row(make_key(.., row)) with row = i.  Float results come back as their bits.
void gh_test_rank_key(int32_t what, const float *x, int64_t n, uint32_t *out_u32) {
    namespace rk = gorse::rank;
    for (int64_t i = 0; i < n; i++) {
        switch (what) {
        case 0: out_u32[i] = rk::fkey(x[i]); break;
        case 1: out_u32[i] = rk::f2u(rk::fkey_inv(rk::fkey(x[i]))); break;
        case 2: out_u32[i] = rk::dist_key(x[i]); break;
        case 3: out_u32[i] = rk::f2u(rk::dist_from_key(rk::dist_key(x[i]), rk::dist_is_negative_zero(x[i]))); break;
        case 4: out_u32[i] = rk::score_ord(x[i]); break;
        case 5: out_u32[i] = rk::f2u(rk::key_score(rk::make_key(rk::score_ord(x[i]), (int32_t)i))); break;
        default: out_u32[i] = (uint32_t)rk::key_row(rk::make_key(rk::score_ord(x[i]), (int32_t)i)); break;
        }
    }
}
// CPU test hook for the symmetric all-pairs sweep's tile schedule (csrc/topk_sym.hpp, the very header the kernel includes):
// cover[q * n + r] += 1 for every (query q, row r) pair the workgroups of an all-pairs sweep over n rows (queries = the rows
// q0 .. q0 + nq) score -- by a workgroup's own columns (every tile it multiplies) or along the rows of a transposed tile, for the
// columns that emit.  Returns the number of row tiles all workgroups multiplied.
int64_t gh_test_topk_sym_cover(int64_t n, int64_t q0, int64_t nq, int32_t tile_rows, int32_t bq, int32_t *cover) {
    const int64_t all_tiles = (n + tile_rows - 1) / tile_rows;
    const int64_t blocks = (nq + bq - 1) / bq;
    int64_t multiplied = 0;
    for (int64_t blk = 0; blk < blocks; blk++) {
        const gorse::SymSchedule s(q0, nq, tile_rows, bq, blk);
        const int64_t nt = s.tiles(all_tiles);
        multiplied += nt;
        for (int64_t tl = 0; tl < nt; tl++) {
            const int64_t tile = s.tile_index(tl);
            for (int64_t r = tile * tile_rows; r < (tile + 1) * tile_rows && r < n; r++)
                for (int64_t c = blk * bq; c < (blk + 1) * bq; c++) {
                    if (c < nq) cover[c * n + r] += 1;  // the column's own list
                    if (s.transposed(tile) && gorse::SymSchedule::column_emits(q0, nq, tile_rows, c))
                        cover[(r - q0) * n + (q0 + c)] += 1;  // the row's query, candidate = the column's row
                }
        }
    }
    return multiplied;
}
// CPU test hooks for the BPR chunk preparation by user bins (csrc/bpr_bins.hpp, the very header the launch code includes):
// the geometry of a chunk -> out[0..4] = shift, bins, tile, tiles, ok; the words of the tile x bin matrix a handle allocates;
// and the four passes restated on the CPU over given user keys -> run offsets bucket[U + 2] and the (sample id, user) pairs in run order.
void gh_test_bpr_bins_geometry(int64_t U, int64_t n, int64_t *out5) {
    const gorse::PrepBins pb = gorse::prep_bins(U, n);
    out5[0] = pb.shift, out5[1] = pb.nbins, out5[2] = pb.tile, out5[3] = (n + pb.tile - 1) / pb.tile, out5[4] = pb.ok ? 1 : 0;
}
int64_t gh_test_bpr_bins_matrix_words(int64_t U, int64_t cap) { return (int64_t)gorse::prep_matrix_words(U, cap); }
int32_t gh_test_bpr_bins_emulate(int64_t U, const int32_t *key, int64_t n, int32_t *bucket, int32_t *pair_s, int32_t *pair_u) {
    std::vector<int32_t> b, ps, pu;
    if (!gorse::prep_bins_emulate(U, key, n, b, ps, pu)) return 0;
    std::copy(b.begin(), b.end(), bucket);
    std::copy(ps.begin(), ps.end(), pair_s);
    std::copy(pu.begin(), pu.end(), pair_u);
    return 1;
}
// the hot items of a BPR handle and their replica rows (csrc/hot_rows.hpp, the header gorse_mf_create includes) for a user CSR, with
// replica unit `unit` and at most `max_r` rows per item: items[s], meta[s] = hot_code(first row, log2 R) for the returned number of
// slots (at most min(1024, I / 4)); out1[0] = the rows in all
int32_t gh_test_bpr_hot_layout(int64_t U, int64_t I, const int64_t *uptr, const int32_t *uidx, double unit, int32_t max_r, int32_t *items,
                               int32_t *meta, int64_t *out1) {
    std::vector<int64_t> cnt((size_t)I, 0);
    for (int64_t t = 0; t < uptr[U]; t++) cnt[(size_t)uidx[t]]++;
    const std::vector<int32_t> hot = gorse::hot_items_select(cnt, uptr[U]);
    std::vector<int32_t> slot((size_t)I, -1);
    for (size_t k = 0; k < hot.size(); k++) slot[(size_t)hot[k]] = (int32_t)k;
    std::vector<uint64_t> acc(hot.size(), 0);
    gorse::hot_shares_rows(uptr, uidx, slot.data(), 0, U, acc.data());
    int64_t users = 0;
    for (int64_t r = 0; r < U; r++) users += uptr[r + 1] > uptr[r];
    std::vector<int32_t> m;
    out1[0] = gorse::hot_replica_layout(acc, users, I, gorse::hot_neg_replicas((int64_t)hot.size(), I), unit, max_r, m);
    std::copy(hot.begin(), hot.end(), items);
    std::copy(m.begin(), m.end(), meta);
    return (int32_t)hot.size();
}
// the accumulated tier of a BPR handle (csrc/hot_rows.hpp acc_rows_layout) on top of the hot layout above, for nFactors d and cold window
// `window`: slot[I] = the class of every item as gorse_mf_create uploads it, acc_items[k] = the item of the tier's k-th row (at most I);
// out3 = {replica rows of the hot tier, hot items, cold items}; returns the tier's rows
int32_t gh_test_bpr_acc_layout(int64_t U, int64_t I, int32_t d, const int64_t *uptr, const int32_t *uidx, double unit, int32_t max_r,
                               int64_t window, int32_t *slot_out, int32_t *acc_items, int64_t *out3) {
    std::vector<int64_t> cnt((size_t)I, 0);
    for (int64_t t = 0; t < uptr[U]; t++) cnt[(size_t)uidx[t]]++;
    const std::vector<int32_t> hot = gorse::hot_items_select(cnt, uptr[U]);
    std::vector<int32_t> slot((size_t)I, -1);
    int64_t n_cold = 0;
    for (int64_t i = 0; i < I; i++)
        if (gorse::item_is_cold(cnt[(size_t)i], uptr[U], I, window)) slot[(size_t)i] = -2, n_cold++;
    for (size_t k = 0; k < hot.size(); k++) slot[(size_t)hot[k]] = (int32_t)k;
    std::vector<uint64_t> acc(hot.size(), 0);
    gorse::hot_shares_rows(uptr, uidx, slot.data(), 0, U, acc.data());
    int64_t users = 0;
    for (int64_t r = 0; r < U; r++) users += uptr[r + 1] > uptr[r];
    std::vector<int32_t> m, ai, am;
    const int64_t rows = gorse::hot_replica_layout(acc, users, I, gorse::hot_neg_replicas((int64_t)hot.size(), I), unit, max_r, m);
    for (size_t k = 0; k < hot.size(); k++) slot[(size_t)hot[k]] = m[k];
    const int64_t n_acc = gorse::acc_rows_layout(slot, rows, U, d, n_cold, ai, am);
    std::copy(slot.begin(), slot.end(), slot_out);
    std::copy(ai.begin(), ai.end(), acc_items);
    out3[0] = rows, out3[1] = (int64_t)hot.size(), out3[2] = n_cold;
    return (int32_t)n_acc;
}
// The owner mapping of the BPR sole-writer fold (csrc/hot_rows.hpp fold_share: csrc/bpr_fold.hpp run_folders takes a thread's share from it
// once per launch, and the periodic passes and the last pass all walk that share): for `folders` folder workgroups, the first
// min(folders, hot_blocks) of them the hot tier's, every thread walks the groups of its share as a pass does.  owner[(slot, element)] =
// block x threads + thread of the element's owner, -1 where nobody owns it; claims[(slot, element)] = how many threads claimed it.
// Returns the floats of a group (what one access moves), 0 where d is no multiple of it.
int32_t gh_test_bpr_fold_owner(int32_t n_hot, int32_t n_acc, int32_t d, int32_t folders, int32_t hot_blocks, int32_t *owner, int32_t *claims) {
    if (d % gorse::kFoldGroup != 0) return 0;
    const int64_t n = (int64_t)(n_hot + n_acc) * d;
    std::fill(owner, owner + n, -1);
    std::fill(claims, claims + n, 0);
    for (int b = 0; b < folders; b++)
        for (int t = 0; t < gorse::kFolderThreads; t++) {
            const gorse::FoldShare sh = gorse::fold_share(b, t, n_hot, n_acc, folders, hot_blocks);
            const int groups = gorse::fold_groups(sh, d);
            for (int g = sh.tid; g < groups; g += sh.nthreads) {
                const int slot = gorse::fold_group_slot(sh, g, d), e = gorse::fold_group_elem(g, d);
                for (int k = 0; k < gorse::kFoldGroup; k++) {
                    owner[(int64_t)slot * d + e + k] = b * gorse::kFolderThreads + t;
                    claims[(int64_t)slot * d + e + k]++;
                }
            }
        }
    return gorse::kFoldGroup;
}
// the ALS row plan's long-row threshold for a side of `side_entries` feedbacks (csrc/als_plan.hpp, the header als_build_plan includes)
int64_t gh_test_als_long_row(int64_t side_entries, int32_t d) { return gorse::als_long_row_threshold(side_entries, d); }
// the 64-bit sparse ranking key itself, and the number of results the reference returns (xvec.go:379-446)
uint64_t gh_test_sparse_key(float score, int32_t row) { return gorse::rank::make_key(gorse::rank::score_ord(score), row); }
int32_t gh_test_sparse_written(int64_t pos, int64_t neg, int64_t adm, int32_t k) { return gorse::rank::written(pos, neg, adm, k); }
// the scratch numbering of a sparse index's rows (csrc/sparse_host.hpp, the header gorse_sparse_create includes): longest first, the
// rows longer than front_cut in a row group of their own with phantom ids behind them.  new_of: n, orig_of: n + group entries at most;
// out3 = {scratch ids, front rows, phantom ids}
void gh_test_sparse_row_order(int64_t n, const int64_t *indptr, int64_t front_cut, int64_t group, int32_t *new_of, int32_t *orig_of,
                              int64_t *out3) {
    const gorse::sparse::RowOrder o = gorse::sparse::order_rows(n, indptr, front_cut, group);
    for (int64_t r = 0; r < n; r++) new_of[r] = o.new_of[(size_t)r];
    for (int64_t s = 0; s < o.Np; s++) orig_of[s] = o.orig_of[(size_t)s];
    out3[0] = o.Np, out3[1] = o.n_front, out3[2] = o.pad;
}
// the HNSW levels MarshalReference gives the n vectors of a model (gorse_vectors.hpp ReferenceLevels: the arithmetic both twins share)
// and the levelFactor it writes, as its bits
uint32_t gh_test_hnsw_levels(int64_t n, int32_t *level) {
    const std::vector<int> lv = logics::MatrixFactorizationItems::ReferenceLevels(n);
    for (int64_t i = 0; i < n; i++) level[i] = lv[(size_t)i];
    const float f = logics::MatrixFactorizationItems::ReferenceLevelFactor();
    uint32_t bits;
    memcpy(&bits, &f, 4);
    return bits;
}
// ---- model/ctr: the factorization machine's Fit loop and EvaluateClassification ---------------------------------------
// metric: 0 Precision, 1 Recall, 2 Accuracy, 3 AUC (evaluator.go:85-153)
float gh_ctr_metric(int32_t id, const float *pos, int32_t npos, const float *neg, int32_t nneg) {
    const std::vector<float> p(pos, pos + npos), n(neg, neg + nneg);
    switch (id) {
        case 0: return ctr::Precision(p, n);
        case 1: return ctr::Recall(p, n);
        case 2: return ctr::Accuracy(p, n);
        default: return ctr::AUC(p, n);
    }
}
void *gh_ctr_dataset_new(int64_t n_features) {
    auto *d = new ctr::Dataset();
    d->n_features = n_features;
    return d;
}
void gh_ctr_dataset_free(void *d) { delete (ctr::Dataset *)d; }
// n rows at once: row i = idx / val [indptr[i], indptr[i+1])
void gh_ctr_dataset_add(void *d, int64_t n, const int64_t *indptr, const int32_t *idx, const float *val, const float *target) {
    for (int64_t i = 0; i < n; i++)
        ((ctr::Dataset *)d)->Add(idx + indptr[i], val + indptr[i], (int)(indptr[i + 1] - indptr[i]), target[i]);
}
// item embeddings of the rows added so far: per field its dimension and a Count() x D matrix of bf16 bit patterns (zero
// rows where a sample has none); n_fields = 0 removes them.  Returns 0, or 1 when called before the rows are complete.
int32_t gh_ctr_dataset_set_embeddings(void *d, int32_t n_fields, const int32_t *dims, const uint16_t *const *emb) {
    auto *ds = (ctr::Dataset *)d;
    ds->emb_dims.assign(dims, dims + n_fields);
    ds->emb.assign((size_t)n_fields, {});
    for (int32_t k = 0; k < n_fields; k++) ds->emb[(size_t)k].assign(emb[k], emb[k] + (size_t)ds->Count() * (size_t)dims[k]);
    return 0;
}
// one embedding field's tensors after Fit: H (d x D), Wa (D x d), ba (d), We (D x d), be (d); returns the field count
int32_t gh_fm_field_params(void *m, int32_t field, float *H, float *Wa, float *ba, float *We, float *be) {
    const auto *f = (ctr::FM *)m;
    if (field >= 0 && field < (int32_t)f->fields.size()) {
        const auto &x = f->fields[(size_t)field];
        std::copy(x.H.begin(), x.H.end(), H);
        std::copy(x.Wa.begin(), x.Wa.end(), Wa);
        std::copy(x.ba.begin(), x.ba.end(), ba);
        std::copy(x.We.begin(), x.We.end(), We);
        std::copy(x.be.begin(), x.be.end(), be);
    }
    return (int32_t)f->fields.size();
}
// optimizer: 0 SGD, 1 Adam (model.SGD / model.Adam)
void *gh_fm_new(int32_t n_factors, int32_t n_epochs, int32_t batch_size, float lr, float reg, int32_t optimizer, int64_t seed) {
    return new ctr::FM(n_factors, n_epochs, batch_size, lr, reg, optimizer, seed);
}
void gh_fm_free(void *m) { delete (ctr::FM *)m; }
// score4 = Precision, Recall, Accuracy, AUC of the returned Score
int32_t gh_fm_fit(void *m, void *train, void *test, int32_t verbose, int32_t patience, const int32_t *cancel, float *score4) {
    return guard([&] {
        ctr::FitConfig cfg;
        cfg.Verbose = verbose;
        cfg.Patience = patience;
        cfg.cancel = cancel;
        const ctr::Score s = ((ctr::FM *)m)->Fit(*(ctr::Dataset *)train, *(ctr::Dataset *)test, cfg);
        score4[0] = s.Precision, score4[1] = s.Recall, score4[2] = s.Accuracy, score4[3] = s.AUC;
    });
}
int32_t gh_fm_evaluate(void *m, void *test, float *score4) {
    return guard([&] {
        const ctr::Score s = ctr::EvaluateClassification(*(ctr::FM *)m, *(ctr::Dataset *)test);
        score4[0] = s.Precision, score4[1] = s.Recall, score4[2] = s.Accuracy, score4[3] = s.AUC;
    });
}
// ctr::FM::SetTest / EvaluateResident / SetHostEvaluate: the test split resident on the device
int32_t gh_fm_set_test(void *m, void *test) {
    return guard([&] { ((ctr::FM *)m)->SetTest(*(ctr::Dataset *)test); });
}
int32_t gh_fm_evaluate_resident(void *m, float *score4) {
    return guard([&] {
        const ctr::Score s = ((ctr::FM *)m)->EvaluateResident();
        score4[0] = s.Precision, score4[1] = s.Recall, score4[2] = s.Accuracy, score4[3] = s.AUC;
    });
}
void gh_fm_set_host_evaluate(void *m, int32_t on) { ((ctr::FM *)m)->SetHostEvaluate(on != 0); }
// the evaluations of the last Fit: epoch, cost, AUC; returns how many there are (at most cap are written)
int32_t gh_fm_log(void *m, int32_t *epochs, float *costs, float *aucs, int32_t cap) {
    const auto &lg = ((ctr::FM *)m)->log;
    for (int32_t i = 0; i < cap && i < (int32_t)lg.size(); i++) epochs[i] = lg[i].epoch, costs[i] = lg[i].cost, aucs[i] = lg[i].score.AUC;
    return (int32_t)lg.size();
}
// B, W (n_features), V (n_features x d) after Fit
void gh_fm_params(void *m, float *B, float *W, float *V) {
    const auto *f = (ctr::FM *)m;
    *B = f->B;
    std::copy(f->W.begin(), f->W.end(), W);
    std::copy(f->V.begin(), f->V.end(), V);
}
static ctr::LabelRows label_rows(int64_t n, const int32_t *id, const int64_t *indptr, const int32_t *label, const float *value) {
    ctr::LabelRows r;
    r.id.assign(id, id + n);
    r.indptr.assign(indptr, indptr + n + 1);
    r.label.assign(label, label + indptr[n]);
    r.value.assign(value, value + indptr[n]);
    return r;
}
// ctr::FM::SetItems: n label rows (id[i] < 0 / label < 0: unknown to the index) and one n x D bf16 table per field of the model
int32_t gh_ctr_fm_set_items(void *m, int64_t n, const int32_t *id, const int64_t *indptr, const int32_t *label, const float *value,
                            int32_t n_fields, const uint16_t *const *emb) {
    return guard([&] {
        ((ctr::FM *)m)->SetItems(label_rows(n, id, indptr, label, value), std::vector<const uint16_t *>(emb, emb + n_fields));
    });
}
// ctr::FM::RankUsers: items_out / scores_out in cand's layout, every user's list sorted
int32_t gh_ctr_fm_rank_users(void *m, int64_t n, const int32_t *id, const int64_t *indptr, const int32_t *label, const float *value,
                             const int64_t *cand_indptr, const int32_t *cand, int32_t *items_out, float *scores_out) {
    return guard([&] {
        std::vector<std::vector<int32_t>> cands((size_t)n);
        for (int64_t t = 0; t < n; t++) cands[(size_t)t].assign(cand + cand_indptr[t], cand + cand_indptr[t + 1]);
        const auto ranked = ((ctr::FM *)m)->RankUsers(label_rows(n, id, indptr, label, value), cands);
        for (int64_t t = 0; t < n; t++)
            for (size_t r = 0; r < ranked[(size_t)t].size(); r++) {
                items_out[cand_indptr[t] + (int64_t)r] = ranked[(size_t)t][r].item;
                scores_out[cand_indptr[t] + (int64_t)r] = ranked[(size_t)t][r].score;
            }
    });
}
// ---- model/ctr in sample form: ctr::SampleDataset, Materialise and the Fit that trains from it ---------------------------------
void *gh_ctr_samples_new(int64_t n_features) {
    auto *d = new ctr::SampleDataset();
    d->n_features = n_features;
    return d;
}
void gh_ctr_samples_free(void *d) { delete (ctr::SampleDataset *)d; }
// one side as label rows (side 0: users, 1: items), replacing it
void gh_ctr_samples_set_side(void *d, int32_t side, int64_t n, const int32_t *id, const int64_t *indptr, const int32_t *label,
                             const float *value) {
    auto *s = (ctr::SampleDataset *)d;
    (side == 0 ? s->users : s->items) = label_rows(n, id, indptr, label, value);
}
// the items' embeddings: per field its dimension and an items.Count() x D matrix of bf16 bit patterns (after the item side)
void gh_ctr_samples_set_embeddings(void *d, int32_t n_fields, const int32_t *dims, const uint16_t *const *emb) {
    auto *s = (ctr::SampleDataset *)d;
    s->emb_dims.assign(dims, dims + n_fields);
    s->emb.assign((size_t)n_fields, {});
    for (int32_t k = 0; k < n_fields; k++) s->emb[(size_t)k].assign(emb[k], emb[k] + (size_t)s->items.Count() * (size_t)dims[k]);
}
void gh_ctr_samples_add(void *d, int64_t n, const int32_t *user, const int32_t *item, const float *target) {
    auto *s = (ctr::SampleDataset *)d;
    s->user.insert(s->user.end(), user, user + n);
    s->item.insert(s->item.end(), item, item + n);
    s->target.insert(s->target.end(), target, target + n);
}
// ctr::Materialise: a new ctr::Dataset (gh_ctr_dataset_free), or NULL where the samples are malformed
void *gh_ctr_samples_materialise(void *d) {
    ctr::Dataset *out = nullptr;
    guard([&] { out = new ctr::Dataset(ctr::Materialise(*(ctr::SampleDataset *)d)); });
    return out;
}
// a ctr::Dataset's contents: out3 = rows, entries, embedding fields; then the rows; then one field's matrix (returns its D)
void gh_ctr_dataset_shape(void *d, int64_t *out3) {
    const auto *ds = (ctr::Dataset *)d;
    out3[0] = ds->Count(), out3[1] = (int64_t)ds->indices.size(), out3[2] = (int64_t)ds->emb_dims.size();
}
void gh_ctr_dataset_read(void *d, int64_t *indptr, int32_t *idx, float *val, float *target) {
    const auto *ds = (ctr::Dataset *)d;
    std::copy(ds->indptr.begin(), ds->indptr.end(), indptr);
    std::copy(ds->indices.begin(), ds->indices.end(), idx);
    std::copy(ds->values.begin(), ds->values.end(), val);
    std::copy(ds->target.begin(), ds->target.end(), target);
}
int32_t gh_ctr_dataset_read_embeddings(void *d, int32_t field, uint16_t *out) {
    const auto *ds = (ctr::Dataset *)d;
    if (field < 0 || field >= (int32_t)ds->emb_dims.size()) return 0;
    if (out) std::copy(ds->emb[(size_t)field].begin(), ds->emb[(size_t)field].end(), out);
    return ds->emb_dims[(size_t)field];
}
int32_t gh_fm_fit_samples(void *m, void *train, void *test, int32_t verbose, int32_t patience, const int32_t *cancel, float *score4) {
    return guard([&] {
        ctr::FitConfig cfg;
        cfg.Verbose = verbose;
        cfg.Patience = patience;
        cfg.cancel = cancel;
        const ctr::Score s = ((ctr::FM *)m)->Fit(*(ctr::SampleDataset *)train, *(ctr::SampleDataset *)test, cfg);
        score4[0] = s.Precision, score4[1] = s.Recall, score4[2] = s.Accuracy, score4[3] = s.AUC;
    });
}
}  // extern "C"
