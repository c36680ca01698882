// gorse_ctr.cpp -- see gorse_ctr.hpp.
#include "gorse_ctr.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "gorse_cf.hpp"

namespace gorse {
namespace ctr {

int Dataset::MaxLen() const {
    int m = 0;
    for (size_t i = 0; i + 1 < indptr.size(); i++) m = std::max(m, (int)(indptr[i + 1] - indptr[i]));
    return m;
}

void Dataset::Add(const int32_t *idx, const float *val, int len, float t) {
    indices.insert(indices.end(), idx, idx + len);
    values.insert(values.end(), val, val + len);
    indptr.push_back((int64_t)indices.size());
    target.push_back(t);
}

float Precision(const std::vector<float> &pos, const std::vector<float> &neg) {
    float tp = 0, fp = 0;
    for (float p : pos)
        if (p > 0) tp++;
    for (float p : neg)
        if (p > 0) fp++;
    if (tp + fp == 0) return 0;
    return tp / (tp + fp);
}

float Recall(const std::vector<float> &pos, const std::vector<float> &) {
    float tp = 0, fn = 0;
    for (float p : pos) {
        if (p > 0)
            tp++;
        else
            fn++;
    }
    if (tp + fn == 0) return 0;
    return tp / (tp + fn);
}

float Accuracy(const std::vector<float> &pos, const std::vector<float> &neg) {
    float correct = 0;
    for (float p : pos)
        if (p > 0) correct++;
    for (float p : neg)
        if (p < 0) correct++;
    if (pos.size() + neg.size() == 0) return 0;
    return correct / (float)(pos.size() + neg.size());
}

float AUC(std::vector<float> pos, std::vector<float> neg) {
    std::sort(pos.begin(), pos.end());
    std::sort(neg.begin(), neg.end());
    float sum = 0;
    size_t nPos = 0;
    for (float p : pos) {
        while (nPos < neg.size() && neg[nPos] < p) nPos++;
        sum += (float)nPos;
    }
    if (pos.size() * neg.size() == 0) return 0;
    return sum / (float)(pos.size() * neg.size());
}

FM::~FM() {
    if (h_) gorse_fm_destroy(h_);
}

// convertToTensors (fm.go:527-577): rows padded with index 0 / value 0 to the wider of the training width and the longest row
static void pad_rows(const Dataset &ds, const std::vector<int64_t> &rows, int width, std::vector<int32_t> &idx,
                     std::vector<float> &val) {
    idx.assign(rows.size() * (size_t)width, 0);
    val.assign(rows.size() * (size_t)width, 0.0f);
    for (size_t r = 0; r < rows.size(); r++) {
        const int64_t b = ds.indptr[(size_t)rows[r]], e = ds.indptr[(size_t)rows[r] + 1];
        for (int64_t j = b; j < e; j++) {
            idx[r * width + (size_t)(j - b)] = ds.indices[(size_t)j];
            val[r * width + (size_t)(j - b)] = ds.values[(size_t)j];
        }
    }
}

std::vector<float> FM::BatchInternalPredict(const Dataset &ds, const std::vector<int64_t> &rows) {
    std::vector<float> out(rows.size());
    if (rows.empty()) return out;
    if (!h_) throw std::invalid_argument("model is not fitted");
    int width = std::max(1, numDimension_);
    for (int64_t r : rows) width = std::max(width, (int)(ds.indptr[(size_t)r + 1] - ds.indptr[(size_t)r]));
    std::vector<int32_t> idx;
    std::vector<float> val;
    pad_rows(ds, rows, width, idx, val);
    if (fields.empty()) {
        check(gorse_fm_predict(h_, (int64_t)rows.size(), width, idx.data(), val.data(), out.data()));
        return out;
    }
    // the rows' embeddings gathered per field (convertToTensors); a set without them scores with absent (zero) embeddings
    if (!ds.emb_dims.empty() && ds.emb_dims.size() != fields.size()) throw std::invalid_argument("embedding fields differ from the fitted model's");
    std::vector<std::vector<uint16_t>> emb(fields.size());
    std::vector<const uint16_t *> ptrs(fields.size());
    for (size_t k = 0; k < fields.size(); k++) {
        const size_t D = (size_t)fields[k].D;
        if (!ds.emb_dims.empty() && ds.emb_dims[k] != fields[k].D) throw std::invalid_argument("embedding dimension differs from the fitted model's");
        emb[k].assign(rows.size() * D, 0);
        if (!ds.emb_dims.empty())
            for (size_t r = 0; r < rows.size(); r++)
                std::copy(ds.emb[k].begin() + (size_t)rows[r] * D, ds.emb[k].begin() + ((size_t)rows[r] + 1) * D, emb[k].begin() + r * D);
        ptrs[k] = emb[k].data();
    }
    check(gorse_fm_predict_embeddings(h_, (int64_t)rows.size(), width, idx.data(), val.data(), ptrs.data(), batchSize_, out.data()));
    return out;
}

// BatchPredict's encoding of one side (fm.go:183-206): the id entry with value 1 when the index knows the entity, then the
// labels it knows, in order; lead = 1 exactly when the id entry is there
static void encode_rows(const LabelRows &rows, std::vector<int64_t> &ptr, std::vector<int32_t> &idx, std::vector<float> &val,
                        std::vector<int32_t> &lead) {
    const int64_t n = rows.Count();
    if ((int64_t)rows.indptr.size() != n + 1) throw std::invalid_argument("label rows: indptr must hold Count() + 1 entries");
    ptr.assign(1, 0);
    idx.clear(), val.clear(), lead.clear();
    for (int64_t i = 0; i < n; i++) {
        const bool known = rows.id[(size_t)i] >= 0;
        if (known) idx.push_back(rows.id[(size_t)i]), val.push_back(1.0f);
        lead.push_back(known ? 1 : 0);
        for (int64_t j = rows.indptr[(size_t)i]; j < rows.indptr[(size_t)i + 1]; j++)
            if (rows.label[(size_t)j] >= 0) idx.push_back(rows.label[(size_t)j]), val.push_back(rows.value[(size_t)j]);
        ptr.push_back((int64_t)idx.size());
    }
}

void FM::SetItems(const LabelRows &items, const std::vector<const uint16_t *> &emb) {
    if (!h_) throw std::invalid_argument("model is not fitted");
    if (emb.size() != fields.size()) throw std::invalid_argument("one embedding table per field of the fitted model");
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx, lead;
    std::vector<float> val;
    encode_rows(items, ptr, idx, val, lead);
    check(gorse_fm_set_items(h_, items.Count(), ptr.data(), idx.data(), val.data(), lead.data(), emb.empty() ? nullptr : emb.data()));
}

std::vector<std::vector<Ranked>> FM::RankUsers(const LabelRows &users, const std::vector<std::vector<int32_t>> &cands) {
    if (!h_) throw std::invalid_argument("model is not fitted");
    if ((int64_t)cands.size() != users.Count()) throw std::invalid_argument("one candidate list per user");
    std::vector<int64_t> ptr, cptr(1, 0);
    std::vector<int32_t> idx, lead, flat;
    std::vector<float> val;
    encode_rows(users, ptr, idx, val, lead);
    for (const auto &c : cands) {
        flat.insert(flat.end(), c.begin(), c.end());
        cptr.push_back((int64_t)flat.size());
    }
    std::vector<float> scores(flat.size());
    std::vector<int32_t> order(flat.size());
    check(gorse_fm_rank_users(h_, users.Count(), ptr.data(), idx.data(), val.data(), lead.data(), cptr.data(), flat.data(), batchSize_,
                              nullptr, scores.data(), order.data()));
    std::vector<std::vector<Ranked>> out(cands.size());
    for (size_t t = 0; t < cands.size(); t++) {
        const size_t c0 = (size_t)cptr[t];
        for (size_t r = 0; r < cands[t].size(); r++) {
            const size_t p = c0 + (size_t)order[c0 + r];
            out[t].push_back({flat[p], scores[p]});
        }
    }
    return out;
}

void FM::SetTest(const Dataset &test) {
    if (!h_) throw std::invalid_argument("model is not fitted");
    const int64_t n = test.Count();
    testCount_ = -1;
    testPositive_.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; i++) testPositive_[(size_t)i] = test.target[(size_t)i] > 0;
    if (n == 0) {
        check(gorse_fm_set_test(h_, 0, 1, nullptr, nullptr, nullptr, nullptr));
        testCount_ = 0;
        return;
    }
    const int width = std::max({1, numDimension_, test.MaxLen()});
    std::vector<int64_t> all((size_t)n);
    for (int64_t i = 0; i < n; i++) all[(size_t)i] = i;
    std::vector<int32_t> idx;
    std::vector<float> val;
    pad_rows(test, all, width, idx, val);
    // a set without embeddings scores with absent (zero) ones, as BatchInternalPredict has it
    if (!test.emb_dims.empty() && test.emb_dims.size() != fields.size()) throw std::invalid_argument("embedding fields differ from the fitted model's");
    std::vector<std::vector<uint16_t>> zeros(fields.size());
    std::vector<const uint16_t *> ptrs(fields.size());
    for (size_t k = 0; k < fields.size(); k++) {
        if (!test.emb_dims.empty()) {
            if (test.emb_dims[k] != fields[k].D) throw std::invalid_argument("embedding dimension differs from the fitted model's");
            ptrs[k] = test.emb[k].data();
        } else {
            zeros[k].assign((size_t)n * (size_t)fields[k].D, 0);
            ptrs[k] = zeros[k].data();
        }
    }
    check(gorse_fm_set_test(h_, n, width, idx.data(), val.data(), test.target.data(), fields.empty() ? nullptr : ptrs.data()));
    testCount_ = n;
}

// the float32 counter `x++` run `count` times from 0: past 2^24 the increment rounds away
static float counter(int64_t count) { return (float)std::min<int64_t>(count, (int64_t)1 << 24); }

Score FM::EvaluateResident() {
    if (!h_ || testCount_ < 0) throw std::invalid_argument("no resident test split (SetTest)");
    if (testCount_ == 0) return Score{};
    int64_t c[GORSE_FM_EVAL_COUNTS];
    float aucSum = 0;
    check(gorse_fm_evaluate(h_, batchSize_, nullptr, c, &aucSum, nullptr));
    Score s;
    if (c[5] > 0) {  // a NaN logit: the metrics' own loops decide, on the same logits
        std::vector<float> logits((size_t)testCount_), pp, np_;
        check(gorse_fm_evaluate(h_, batchSize_, nullptr, c, &aucSum, logits.data()));
        for (int64_t i = 0; i < testCount_; i++) (testPositive_[(size_t)i] ? pp : np_).push_back(logits[(size_t)i]);
        s.Precision = Precision(pp, np_);
        s.Recall = Recall(pp, np_);
        s.Accuracy = Accuracy(pp, np_);
        s.AUC = AUC(pp, np_);
        return s;
    }
    const int64_t nPos = c[0], nNeg = c[1];
    const float tp = counter(c[2]), fp = counter(c[3]), fn = counter(nPos - c[2]);
    s.Precision = tp + fp == 0 ? 0 : tp / (tp + fp);
    s.Recall = tp + fn == 0 ? 0 : tp / (tp + fn);
    s.Accuracy = counter(c[2] + c[4]) / (float)(size_t)(nPos + nNeg);
    s.AUC = nPos * nNeg == 0 ? 0 : aucSum / (float)((size_t)nPos * (size_t)nNeg);
    return s;
}

void FM::ReadBack() {
    check(gorse_fm_get_params(h_, &B, W.data(), V.data()));
    for (size_t k = 0; k < fields.size(); k++) {
        Field &f = fields[k];
        check(gorse_fm_get_embedding_params(h_, (int32_t)k, f.H.data(), f.Wa.data(), f.ba.data(), f.We.data(), f.be.data()));
    }
}

Score EvaluateClassification(FM &m, const Dataset &test) {
    std::vector<int64_t> pos, neg;
    for (int64_t i = 0; i < test.Count(); i++) (test.target[(size_t)i] > 0 ? pos : neg).push_back(i);
    const std::vector<float> pp = m.BatchInternalPredict(test, pos), np_ = m.BatchInternalPredict(test, neg);
    if (test.Count() == 0) return Score{};
    Score s;
    s.Precision = Precision(pp, np_);
    s.Recall = Recall(pp, np_);
    s.Accuracy = Accuracy(pp, np_);
    s.AUC = AUC(pp, np_);
    return s;
}

void FM::Init(int64_t nFeatures, const std::vector<int32_t> &embDims) {
    // Init (fm.go:247-270): B = 0, W and V from N(0, 0.01) (layers.go:82-87), W drawn first
    nf_ = nFeatures;
    if (h_) gorse_fm_destroy(h_), h_ = nullptr;
    check(gorse_fm_create(&h_, device_, nf_, nFactors_));
    util::RandomGenerator rng(seed_);
    B = 0;
    rng.NormalMatrix(nf_, 1, 0, 0.01f, W);
    rng.NormalMatrix(nf_, nFactors_, 0, 0.01f, V);
    // the embedding fields (fm.go:257-264): nn.NewAttention draws its Linear (Wa ~ Uniform(+-1/sqrt(D)), ba = 0), then
    // H ~ Normal(0, 0.01); nn.NewLinear draws We the same way, be = 0 (layers.go:42-48, 166-171)
    fields.assign(embDims.size(), Field{});
    check(gorse_fm_set_embedding_dims(h_, (int32_t)embDims.size(), embDims.data()));
    auto uniform = [&](size_t n, float bound, std::vector<float> &out) {
        out.resize(n);
        for (auto &x : out) x = (float)rng.Float64() * (2 * bound) - bound;
    };
    for (size_t k = 0; k < fields.size(); k++) {
        Field &f = fields[k];
        f.D = embDims[k];
        const float bound = 1.0f / std::sqrt((float)f.D);
        uniform((size_t)f.D * nFactors_, bound, f.Wa);
        f.ba.assign((size_t)nFactors_, 0.0f);
        rng.NormalMatrix(nFactors_, f.D, 0, 0.01f, f.H);
        uniform((size_t)f.D * nFactors_, bound, f.We);
        f.be.assign((size_t)nFactors_, 0.0f);
    }
    check(gorse_fm_set_params(h_, B, W.data(), V.data()));
    for (size_t k = 0; k < fields.size(); k++) {
        const Field &f = fields[k];
        check(gorse_fm_set_embedding_params(h_, (int32_t)k, f.H.data(), f.Wa.data(), f.ba.data(), f.We.data(), f.be.data()));
    }
    log.clear();
    testCount_ = -1;  // the handle is new
}

template <class Evaluate>
Score FM::Train(const FitConfig &cfg, Evaluate evaluate) {
    Score score = evaluate();
    std::vector<std::pair<int, float>> scores{{0, score.AUC}};
    log.push_back({0, 0.0f, score});
    const int32_t opt = optimizer_ == 0 ? GORSE_OPT_SGD : GORSE_OPT_ADAM;
    for (int epoch = 1; epoch <= nEpochs_; epoch++) {
        float cost = 0;
        const int32_t rc = (cfg.cancel && *cfg.cancel) ? GORSE_ERR_CANCELLED
                                                       : gorse_fm_epoch(h_, batchSize_, opt, lr_, reg_, cfg.cancel, &cost);
        if (rc == GORSE_ERR_CANCELLED) {  // "fit AFM canceled": Score{}, the tensors keep the steps taken
            ReadBack();
            return Score{};
        }
        check(rc);
        if (epoch % cfg.Verbose == 0 || epoch == nEpochs_) {
            score = evaluate();
            scores.push_back({epoch, score.AUC});
            log.push_back({epoch, cost, score});
            if (std::isnan(cost) || std::isnan(score.GetValue())) break;  // model diverged
            if (cfg.Patience > 0 && epoch > cfg.Patience) {
                // lo.MaxBy: the first maximum
                auto best = scores[0];
                for (const auto &s : scores)
                    if (s.second > best.second) best = s;
                if (best.first <= epoch - cfg.Patience) break;  // early stopping
            }
        }
    }
    ReadBack();  // in Parameters() order: B, V, W, then per field H, Wa, ba, We, be
    return score;
}

Score FM::Fit(const Dataset &train, const Dataset &test, const FitConfig &cfg) {
    numDimension_ = train.MaxLen();
    if (!train.emb_dims.empty()) {
        if (train.emb.size() != train.emb_dims.size()) throw std::invalid_argument("one embedding matrix per field");
        for (size_t k = 0; k < train.emb_dims.size(); k++)
            if (train.emb[k].size() != (size_t)train.Count() * (size_t)train.emb_dims[k])
                throw std::invalid_argument("an embedding matrix must hold Count() x D values");
    }
    Init(train.n_features, train.emb_dims);
    if (!hostEvaluate_) SetTest(test);
    const int width = std::max(1, numDimension_);
    std::vector<int64_t> all((size_t)train.Count());
    for (int64_t i = 0; i < train.Count(); i++) all[(size_t)i] = i;
    {
        std::vector<int32_t> idx;
        std::vector<float> val;
        pad_rows(train, all, width, idx, val);
        check(gorse_fm_set_train(h_, train.Count(), width, idx.data(), val.data(), train.target.data()));
    }
    for (size_t k = 0; k < fields.size(); k++) check(gorse_fm_set_train_embeddings(h_, (int32_t)k, train.emb[k].data()));
    return Train(cfg, [&] { return hostEvaluate_ ? EvaluateClassification(*this, test) : EvaluateResident(); });
}

// sample i's row (Dataset.Get, data.go:221-267): user id | item id | user labels | item labels, from the sides as encode_rows
// leaves them
template <class F>
static void sample_row(const std::vector<int64_t> &uptr, const std::vector<int32_t> &uidx, const std::vector<float> &uval,
                       const std::vector<int32_t> &ulead, const std::vector<int64_t> &iptr, const std::vector<int32_t> &iidx,
                       const std::vector<float> &ival, const std::vector<int32_t> &ilead, int32_t u, int32_t c, F fn) {
    const int64_t u0 = uptr[(size_t)u], u1 = uptr[(size_t)u + 1], um = u0 + ulead[(size_t)u];
    const int64_t i0 = iptr[(size_t)c], i1 = iptr[(size_t)c + 1], im = i0 + ilead[(size_t)c];
    for (int64_t j = u0; j < um; j++) fn(uidx[(size_t)j], uval[(size_t)j]);
    for (int64_t j = i0; j < im; j++) fn(iidx[(size_t)j], ival[(size_t)j]);
    for (int64_t j = um; j < u1; j++) fn(uidx[(size_t)j], uval[(size_t)j]);
    for (int64_t j = im; j < i1; j++) fn(iidx[(size_t)j], ival[(size_t)j]);
}

static void check_samples(const SampleDataset &s) {
    if (s.user.size() != s.target.size() || s.item.size() != s.target.size())
        throw std::invalid_argument("one user, one item and one target per sample");
    for (size_t i = 0; i < s.target.size(); i++)
        if (s.user[i] < 0 || s.user[i] >= s.users.Count() || s.item[i] < 0 || s.item[i] >= s.items.Count())
            throw std::invalid_argument("a sample names a user or an item outside its side");
    if (s.emb.size() != s.emb_dims.size()) throw std::invalid_argument("one embedding table per field");
    for (size_t k = 0; k < s.emb_dims.size(); k++)
        if (s.emb[k].size() != (size_t)s.items.Count() * (size_t)s.emb_dims[k])
            throw std::invalid_argument("an embedding table must hold items.Count() x D values");
}

Dataset Materialise(const SampleDataset &s) {
    check_samples(s);
    std::vector<int64_t> uptr, iptr;
    std::vector<int32_t> uidx, ulead, iidx, ilead;
    std::vector<float> uval, ival;
    encode_rows(s.users, uptr, uidx, uval, ulead);
    encode_rows(s.items, iptr, iidx, ival, ilead);
    Dataset d;
    d.n_features = s.n_features;
    for (int64_t i = 0; i < s.Count(); i++) {
        sample_row(uptr, uidx, uval, ulead, iptr, iidx, ival, ilead, s.user[(size_t)i], s.item[(size_t)i], [&](int32_t f, float x) {
            d.indices.push_back(f);
            d.values.push_back(x);
        });
        d.indptr.push_back((int64_t)d.indices.size());
        d.target.push_back(s.target[(size_t)i]);
    }
    d.emb_dims = s.emb_dims;
    d.emb.assign(s.emb_dims.size(), {});
    for (size_t k = 0; k < s.emb_dims.size(); k++) {
        const size_t D = (size_t)s.emb_dims[k];
        d.emb[k].resize((size_t)s.Count() * D);
        for (int64_t i = 0; i < s.Count(); i++)
            std::copy(s.emb[k].begin() + (size_t)s.item[(size_t)i] * D, s.emb[k].begin() + ((size_t)s.item[(size_t)i] + 1) * D,
                      d.emb[k].begin() + (size_t)i * D);
    }
    return d;
}

Score FM::Fit(const SampleDataset &train, const SampleDataset &test, const FitConfig &cfg) {
    check_samples(train);
    check_samples(test);
    if (test.emb_dims != train.emb_dims || test.items.Count() != train.items.Count())
        throw std::invalid_argument("the test set must share the training set's item side");
    std::vector<int64_t> uptr, iptr;
    std::vector<int32_t> uidx, ulead, iidx, ilead;
    std::vector<float> uval, ival;
    encode_rows(train.users, uptr, uidx, uval, ulead);
    encode_rows(train.items, iptr, iidx, ival, ilead);
    numDimension_ = 0;  // the longest composed row
    for (int64_t i = 0; i < train.Count(); i++) {
        const int32_t u = train.user[(size_t)i], c = train.item[(size_t)i];
        numDimension_ = std::max(numDimension_, (int)(uptr[(size_t)u + 1] - uptr[(size_t)u] + iptr[(size_t)c + 1] - iptr[(size_t)c]));
    }
    Init(train.n_features, train.emb_dims);
    std::vector<const uint16_t *> tables;
    for (const auto &e : train.emb) tables.push_back(e.data());
    SetItems(train.items, tables);  // once: training, evaluation and ranking all read it in place
    check(gorse_fm_set_train_samples(h_, train.users.Count(), uptr.data(), uidx.data(), uval.data(), ulead.data(), train.Count(),
                                     train.user.data(), train.item.data(), train.target.data()));
    Dataset hostTest;
    if (hostEvaluate_) {
        hostTest = Materialise(test);
    } else {
        const int64_t n = test.Count();
        testPositive_.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) testPositive_[(size_t)i] = test.target[(size_t)i] > 0;
        encode_rows(test.users, uptr, uidx, uval, ulead);
        check(gorse_fm_set_test_samples(h_, test.users.Count(), uptr.data(), uidx.data(), uval.data(), ulead.data(), n,
                                        test.user.data(), test.item.data(), test.target.data()));
        testCount_ = n;
    }
    return Train(cfg, [&] { return hostEvaluate_ ? EvaluateClassification(*this, hostTest) : EvaluateResident(); });
}

}  // namespace ctr
}  // namespace gorse
