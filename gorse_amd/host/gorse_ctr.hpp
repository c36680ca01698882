// gorse_ctr.hpp -- host mirror of the reference's model/ctr factorization machine (ctr.AFM with its item-embedding branch,
// model/ctr/fm.go) and of its classification metrics (model/ctr/evaluator.go).  The numerics run on the device through the
// gorse_fm_* entry points of the C ABI; this file holds AFM.Fit's loop (evaluation schedule, NaN stop, patience, cancel) and
// EvaluateClassification as written.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/gorse_hip.h"

namespace gorse {
namespace ctr {

struct Score {  // model/ctr/model.go Score (the classification fields)
    float Precision = 0, Recall = 0, Accuracy = 0, AUC = 0;
    float GetValue() const { return AUC; }
};

// dataset.CTRSplit flattened: row i = indices / values [indptr[i], indptr[i+1]), target +-1
struct Dataset {
    int64_t n_features = 0;
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices;
    std::vector<float> values;
    std::vector<float> target;
    // item embeddings (GetItemEmbeddingDim, fm.go:555-561): per field its dimension and a Count() x D matrix of bf16 bit
    // patterns, an all-zero row where a sample has none; empty for a set without embeddings
    std::vector<int32_t> emb_dims;
    std::vector<std::vector<uint16_t>> emb;
    int64_t Count() const { return (int64_t)target.size(); }
    int MaxLen() const;
    void Add(const int32_t *idx, const float *val, int len, float t);
};

// evaluator.go:85-153, all fp32 (AUC sorts its arguments)
float Precision(const std::vector<float> &pos, const std::vector<float> &neg);
float Recall(const std::vector<float> &pos, const std::vector<float> &neg);
float Accuracy(const std::vector<float> &pos, const std::vector<float> &neg);
float AUC(std::vector<float> pos, std::vector<float> neg);

// One side of a ranking call as label rows, the form BatchPredict receives it in (fm.go:180-206): row i is the entity's own
// feature index (negative: the index does not know it, dataset.NotId) and its labels as (feature index, value), a negative
// index again meaning a label the index does not know.  Values reach this struct scaled.
struct LabelRows {
    std::vector<int32_t> id;
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> label;
    std::vector<float> value;
    int64_t Count() const { return (int64_t)id.size(); }
};

// The reference's own form of a CTR data set (model/ctr/data.go:152-267) without context labels: one label row per user and
// per item, one embedding per item and field, and per sample only (Users[i], Items[i], Target[i]).  Row ids and labels are
// feature indices, as in LabelRows; emb[k] is an items.Count() x emb_dims[k] matrix of bf16 bit patterns (an all-zero row for
// an item without one).  A training set and its test set share one item side, as Dataset.Split leaves them.
struct SampleDataset {
    int64_t n_features = 0;
    LabelRows users, items;
    std::vector<int32_t> emb_dims;
    std::vector<std::vector<uint16_t>> emb;
    std::vector<int32_t> user, item;
    std::vector<float> target;
    int64_t Count() const { return (int64_t)target.size(); }
};

// Dataset.Get (data.go:221-267) for every sample: the user-id entry, the item-id entry, the user's labels, the item's labels
// (entries the index does not know are left out, as BatchPredict leaves them out), and the item's embedding per field
Dataset Materialise(const SampleDataset &s);

struct Ranked {
    int32_t item;  // catalogue row
    float score;
};

struct FitConfig {
    int Verbose = 10, Patience = 0;
    const volatile int32_t *cancel = nullptr;  // ctx.Err() != nil
};

struct EvalRecord {
    int epoch;
    float cost;  // 0 at epoch 0
    Score score;
};

class FM {
   public:
    FM(int nFactors, int nEpochs, int batchSize, float lr, float reg, int optimizer, int64_t seed, int device = 0)
        : nFactors_(nFactors), nEpochs_(nEpochs), batchSize_(batchSize), lr_(lr), reg_(reg), optimizer_(optimizer), seed_(seed),
          device_(device) {}
    ~FM();
    FM(const FM &) = delete;
    FM &operator=(const FM &) = delete;
    // AFM.Fit (fm.go:307-417); a training set with item embeddings trains the attention branch as well
    Score Fit(const Dataset &train, const Dataset &test, const FitConfig &cfg);
    // The same Fit from samples: the item side goes to the device once (SetItems: it stays resident, so RankUsers works
    // afterwards without another SetItems), per sample three numbers (gorse_fm_set_train_samples, gorse_fm_set_test_samples).
    // Initial parameters, evaluation schedule, NaN stop, patience and cancel are Fit's, and so is every bit of the result
    // Fit(Materialise(train), Materialise(test)) gives.  With SetHostEvaluate(true) the test set is materialised once and
    // evaluated through EvaluateClassification.
    Score Fit(const SampleDataset &train, const SampleDataset &test, const FitConfig &cfg);
    // BatchInternalPredict (fm.go:156-178) of rows [0, ds.Count()) that satisfy keep (or all rows)
    std::vector<float> BatchInternalPredict(const Dataset &ds, const std::vector<int64_t> &rows);
    // The bulk form of the worker's rankByClickTroughRate (worker/pipeline.go:451-499).  SetItems encodes the catalogue as
    // BatchPredict would (the id entry when known, then the known labels) and makes it resident on the device with one
    // n_items x D bf16 table per field (emb; empty for a model without fields); RankUsers encodes the users the same way and
    // returns, per user, its candidates (catalogue rows) sorted as gorse_fm_rank_users orders them, with their scores.
    void SetItems(const LabelRows &items, const std::vector<const uint16_t *> &emb);
    std::vector<std::vector<Ranked>> RankUsers(const LabelRows &users, const std::vector<std::vector<int32_t>> &cands);
    // EvaluateClassification from a test split that stays on the device.  SetTest partitions, pads and uploads the set once
    // (gorse_fm_set_test); EvaluateResident scores it there and forms the Score from the counts that come back exactly as
    // evaluator.go:85-153 forms it from the logits (its float32 counters stop at 2^24, as tp++ does).  Should a logit be NaN,
    // the logits are fetched and the metrics' own loops run on them, as the host route's do.  Fit evaluates this way unless
    // SetHostEvaluate(true) asks for the free function below.
    void SetTest(const Dataset &test);
    Score EvaluateResident();
    void SetHostEvaluate(bool on) { hostEvaluate_ = on; }
    float B = 0;
    std::vector<float> W, V;          // the parameters after Fit (copied back, as into the nn tensors)
    struct Field {                    // one embedding field's tensors in Parameters() order (fm.go:136-146)
        int32_t D = 0;
        std::vector<float> H, Wa, ba, We, be;
    };
    std::vector<Field> fields;
    std::vector<EvalRecord> log;      // every evaluation of the last Fit, epoch 0 first

   private:
    int nFactors_, nEpochs_, batchSize_;
    float lr_, reg_;
    int optimizer_;
    int64_t seed_;
    int device_;
    int numDimension_ = 0;
    bool hostEvaluate_ = false;
    int64_t testCount_ = -1;           // rows of the resident split; -1: none
    std::vector<uint8_t> testPositive_;  // per row of it: target > 0
    void ReadBack();
    // Init (fm.go:247-270) on a new handle; Train: the epoch-0 evaluation, the epochs and what stops them, the read-back
    void Init(int64_t nFeatures, const std::vector<int32_t> &embDims);
    template <class Evaluate>
    Score Train(const FitConfig &cfg, Evaluate evaluate);
    int64_t nf_ = 0;
    gorse_fm *h_ = nullptr;
};

Score EvaluateClassification(FM &m, const Dataset &test);  // evaluator.go:46-83

}  // namespace ctr
}  // namespace gorse
