//go:build cgo && hip

// worker/pipeline.go:403-448 for many users at once: with database.vector = "hip://" the collaborative recommendations of a
// batch of users are ONE QueryVectorsBatch on the device (exact -dot top-k with the hidden-item mask applied inside the
// search) instead of one QueryVectors round trip per user.  The master needs no change at all: its publishing step
// (master/tasks.go:930-962) talks to vectors.Database, and "hip://" is one (storage/vectors/hip.go registers the prefix).
// Not compiled here: no Go toolchain in the build image.
package worker

import (
	"context"
	"time"

	mapset "github.com/deckarep/golang-set/v2"
	"github.com/gorse-io/gorse/common/log"
	"github.com/gorse-io/gorse/model/ctr"
	"github.com/gorse-io/gorse/storage/data"
	"github.com/gorse-io/gorse/storage/cache"
	"github.com/gorse-io/gorse/storage/vectors"
	"github.com/pkg/errors"
	"go.uber.org/zap"
)

// bulkQuerier is what storage/vectors/hip.go offers beyond vectors.Database.
type bulkQuerier interface {
	QueryVectorsBatch(ctx context.Context, collection string, queries [][]float32, categories []string, topK int) ([][]vectors.ScoredVector, error)
}

// updateCollaborativeRecommendBulk is updateCollaborativeRecommend for a batch of users.  topK is the largest
// CacheSize + |excludeSet| of the batch: every user gets at least what the per-user call would have fetched.
func (p *Pipeline) updateCollaborativeRecommendBulk(ctx context.Context, matrixFactorizationID int64, userIDs []string,
	userEmbeddings [][]float32, excludeSets []mapset.Set[string]) error {
	bulk, ok := p.VectorClient.(bulkQuerier)
	if !ok { // not the hip:// backend: the reference's loop
		for t := range userIDs {
			if err := p.updateCollaborativeRecommend(ctx, matrixFactorizationID, userIDs[t], userEmbeddings[t], excludeSets[t]); err != nil {
				return err
			}
		}
		return nil
	}
	topK := 0
	for _, s := range excludeSets {
		topK = max(topK, p.Config.Recommend.CacheSize+s.Cardinality())
	}
	localStartTime := time.Now()
	results, err := bulk.QueryVectorsBatch(ctx, vectors.CollaborativeFilteringCollection(matrixFactorizationID), userEmbeddings, nil, topK)
	if err != nil {
		return errors.WithStack(err)
	}
	for t, scoredVectors := range results {
		want := p.Config.Recommend.CacheSize + excludeSets[t].Cardinality()
		recommend := make([]cache.Score, 0, len(scoredVectors))
		for e, vector := range scoredVectors {
			if e >= want {
				break
			}
			if !excludeSets[t].Contains(vector.Id) {
				recommend = append(recommend, cache.Score{Id: vector.Id, Score: float64(vector.Score), Categories: vector.Categories, Timestamp: localStartTime})
			}
		}
		if err := p.CacheClient.AddScores(ctx, cache.CollaborativeFiltering, userIDs[t], recommend); err != nil {
			log.Logger().Error("failed to cache collaborative filtering recommendation result", zap.String("user_id", userIDs[t]), zap.Error(err))
			return errors.WithStack(err)
		}
		if err := p.CacheClient.Set(ctx,
			cache.Time(cache.Key(cache.CollaborativeFilteringUpdateTime, userIDs[t]), localStartTime),
			cache.String(cache.Key(cache.CollaborativeFilteringDigest, userIDs[t]), p.Config.Recommend.Collaborative.Hash(&p.Config.Recommend)),
		); err != nil {
			return errors.WithStack(err)
		}
		if err := p.CacheClient.DeleteScores(ctx, []string{cache.CollaborativeFiltering}, cache.ScoreCondition{Before: &localStartTime, Subset: new(userIDs[t])}); err != nil {
			return errors.WithStack(err)
		}
	}
	return nil
}

// unseenRecommender is the second thing storage/vectors/hip.go offers beyond vectors.Database: every query's topK best vectors that
// are not hidden and not among the query's excluded ids, with the exclusion applied on the device (gorse_mf_recommend over a
// throw-away gorse_mf: item factors = the collection's rows, user factors = the queries, "training rows" = the exclude sets; the C++
// twin is vectors::HipDatabase::RecommendUnseenBatch / logics::CollaborativeRecommendUnseen in gorse_amd/host/gorse_vectors.hpp).
type unseenRecommender interface {
	RecommendUnseenBatch(ctx context.Context, collection string, queries [][]float32, exclude [][]string, topK int) ([][]vectors.ScoredVector, error)
}

// updateCollaborativeRecommendUnseen is what a worker calls INSTEAD of the per-user loop and instead of
// updateCollaborativeRecommendBulk: topK stays CacheSize however long the longest exclude set is, and nothing is filtered on the
// host.  Each user's list is the first CacheSize entries of the list updateCollaborativeRecommend builds; the reference keeps up to
// |excludeSet| further items, an artefact of its over-fetch.
func (p *Pipeline) updateCollaborativeRecommendUnseen(ctx context.Context, matrixFactorizationID int64, userIDs []string,
	userEmbeddings [][]float32, excludeSets []mapset.Set[string]) error {
	rec, ok := p.VectorClient.(unseenRecommender)
	if !ok { // not the hip:// backend
		return p.updateCollaborativeRecommendBulk(ctx, matrixFactorizationID, userIDs, userEmbeddings, excludeSets)
	}
	exclude := make([][]string, len(excludeSets))
	for t, s := range excludeSets {
		exclude[t] = s.ToSlice()
	}
	localStartTime := time.Now()
	results, err := rec.RecommendUnseenBatch(ctx, vectors.CollaborativeFilteringCollection(matrixFactorizationID), userEmbeddings, exclude,
		p.Config.Recommend.CacheSize)
	if err != nil {
		return errors.WithStack(err)
	}
	for t, scoredVectors := range results {
		recommend := make([]cache.Score, 0, len(scoredVectors))
		for _, vector := range scoredVectors {
			recommend = append(recommend, cache.Score{Id: vector.Id, Score: float64(vector.Score), Categories: vector.Categories, Timestamp: localStartTime})
		}
		if err := p.CacheClient.AddScores(ctx, cache.CollaborativeFiltering, userIDs[t], recommend); err != nil {
			log.Logger().Error("failed to cache collaborative filtering recommendation result", zap.String("user_id", userIDs[t]), zap.Error(err))
			return errors.WithStack(err)
		}
		if err := p.CacheClient.Set(ctx,
			cache.Time(cache.Key(cache.CollaborativeFilteringUpdateTime, userIDs[t]), localStartTime),
			cache.String(cache.Key(cache.CollaborativeFilteringDigest, userIDs[t]), p.Config.Recommend.Collaborative.Hash(&p.Config.Recommend)),
		); err != nil {
			return errors.WithStack(err)
		}
		if err := p.CacheClient.DeleteScores(ctx, []string{cache.CollaborativeFiltering}, cache.ScoreCondition{Before: &localStartTime, Subset: new(userIDs[t])}); err != nil {
			return errors.WithStack(err)
		}
	}
	return nil
}

// ctrRanker is what model/ctr/fm_hip.go offers beyond ctr.FactorizationMachines: a resident item catalogue and one ranking call
// for a block of users (gorse_fm_set_items / gorse_fm_rank_users).
type ctrRanker interface {
	EncodeRankItem(itemId string, labels []ctr.Label, embeddings []ctr.Embedding) ctr.RankItem
	EncodeRankUser(userId string, labels []ctr.Label) ([]int32, []float32, int32)
	SetRankItems(items []ctr.RankItem) bool
	RankUsers(ctx context.Context, users []ctr.RankUser) ([][]float32, [][]int32, bool)
}

// rankCatalogue is the item cache encoded once per model and item-cache generation: the rows of the resident catalogue and
// each item's row number.
type rankCatalogue struct {
	row   map[string]int32
	items []data.Item
}

// encodeRankCatalogue encodes every item of the cache the way BatchPredict would and makes the result resident.  Label
// encoding and the scalers run here, in Go; the library sees indices and scaled values only.
func (p *Pipeline) encodeRankCatalogue(ranker ctrRanker, items []data.Item) (*rankCatalogue, bool) {
	catalogue := &rankCatalogue{row: make(map[string]int32, len(items)), items: items}
	encoded := make([]ctr.RankItem, len(items))
	for i := range items {
		catalogue.row[items[i].ItemId] = int32(i)
		encoded[i] = ranker.EncodeRankItem(items[i].ItemId, ctr.ConvertLabels(items[i].Labels), ctr.ConvertEmbeddings(items[i].Labels))
	}
	if !ranker.SetRankItems(encoded) {
		return nil, false
	}
	return catalogue, true
}

// rankByClickThroughRateBulk is rankByClickTroughRate (worker/pipeline.go:451-499) for a block of users: one call scores and
// ranks all their candidates against the resident catalogue.  ok = false sends the caller to the per-user path for the whole
// block: no resident model (the predictor is not a ctrRanker, or Fit did not run in this process), a candidate that is not in
// the catalogue (the item cache moved on: encode it again), or an error from the library.  Around THIS call replacement
// candidates and the decay of read items stay in Go, exactly as around the per-user one; a pass that keeps its candidates on the
// device has them there too: logics.CandidateChain.AddReplacement before the ranking and RankByDecayed in place of RankBy
// (gorse_cand_add_replacement, gorse_fm_rank_cand_decayed).
// Ties: the library orders equal scores by candidate position and puts NaN scores last; cache.SortDocuments is
// sort.Slice(score >), which is not stable, so this is one of the orders it can produce.
func (p *Pipeline) rankByClickThroughRateBulk(ctx context.Context, predictor ctr.FactorizationMachines, catalogue *rankCatalogue,
	users []*data.User, candidates [][]cache.Score, recommendTime time.Time) (ranked [][]cache.Score, ok bool) {
	ranker, isRanker := predictor.(ctrRanker)
	if !isRanker || catalogue == nil || len(users) != len(candidates) {
		return nil, false
	}
	block := make([]ctr.RankUser, len(users))
	for t, user := range users {
		indices, values, lead := ranker.EncodeRankUser(user.UserId, ctr.ConvertLabels(user.Labels))
		block[t] = ctr.RankUser{Indices: indices, Values: values, Lead: lead, Candidates: make([]int32, len(candidates[t]))}
		for r, candidate := range candidates[t] {
			row, found := catalogue.row[candidate.Id]
			if !found {
				return nil, false
			}
			block[t].Candidates[r] = row
		}
	}
	scores, order, done := ranker.RankUsers(ctx, block)
	if !done {
		return nil, false
	}
	ranked = make([][]cache.Score, len(users))
	for t := range users {
		ranked[t] = make([]cache.Score, 0, len(order[t]))
		for _, position := range order[t] {
			item := &catalogue.items[block[t].Candidates[position]]
			ranked[t] = append(ranked[t], cache.Score{
				Id:         item.ItemId,
				Score:      float64(scores[t][position]),
				Categories: item.Categories,
				Timestamp:  recommendTime,
			})
		}
	}
	return ranked, true
}
