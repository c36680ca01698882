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
