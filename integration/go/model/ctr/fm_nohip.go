//go:build !cgo || !hip || xla

package ctr

import (
	"context"

	"github.com/gorse-io/gorse/dataset"
	"github.com/samber/lo"
)

// Without the library (or in the XLA build) the hooks of fm.go find no device model: Fit and BatchInternalPredict run the
// reference's own code.
type hipFM struct{}

func (m *hipFM) close() {}

func (fm *AFM) fitHIP(context.Context, dataset.CTRSplit, dataset.CTRSplit, *FitConfig) (Score, bool) {
	return Score{}, false
}

func (fm *AFM) batchPredictHIP([]lo.Tuple2[[]int32, []float32], [][][]uint16) ([]float32, bool) {
	return nil, false
}

// Without the library there is no resident catalogue: the worker ranks user by user through BatchPredict.
type RankItem struct {
	Indices    []int32
	Values     []float32
	Lead       int32
	Embeddings [][]uint16
}

type RankUser struct {
	Indices    []int32
	Values     []float32
	Lead       int32
	Candidates []int32
}

func (fm *AFM) setItemsHIP([]RankItem) bool { return false }

func (fm *AFM) rankUsersHIP(context.Context, []RankUser) ([][]float32, [][]int32, bool) {
	return nil, nil, false
}

func (fm *AFM) SetRankItems(items []RankItem) bool { return fm.setItemsHIP(items) }

func (fm *AFM) RankUsers(ctx context.Context, users []RankUser) ([][]float32, [][]int32, bool) {
	return fm.rankUsersHIP(ctx, users)
}
