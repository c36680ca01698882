//go:build cgo && hip

// NeighbourRecommender: recommendItemToItem and recommendUserToUser (logics/recommend.go:244-348) for many users with ONE call
// (gorse_nbr_recommend) instead of one QueryItemToItem per positive feedback / one QueryUserToUser per user and a Go map per user.
// Both are a two-hop weighted walk over two tables the handle keeps on the device:
//
//	item-to-item: hop 1 = the users' positive feedback, newest first, unweighted; hop 2 = each item's neighbour list, weighted
//	user-to-user: hop 1 = the users' neighbour lists, weighted;                   hop 2 = each neighbour's positive feedback, unweighted
//
// The tables come from the bulk refresh (QuerySimilarBulk / QuerySimilarTypedBulk in gorse_amd/host/gorse_vectors.hpp: the vector
// database's own float32 score goes in, the cache score -- 1 / (1 - s) for the embedding kinds, s * 0.5 for "auto" -- is formed on
// the device).  A user's list is what the reference builds, with the order among equal sums fixed: larger sum first, equal sums by
// ascending item index (the reference leaves it to Go's map iteration order; its test uses ElementsMatch).  The data-store filter of
// recommendUserToUser (:317-345: hidden items, ItemTTL, categories) stays the caller's.
package logics

/*
#cgo LDFLAGS: -lgorse_hip
#include "gorse_hip.h"
*/
import "C"

import (
	"unsafe"

	"github.com/pkg/errors"
)

// NeighbourTable is one hop as a CSR.  Weights == nil: every weight is 1 (feedback rows).
type NeighbourTable struct {
	Indptr  []int64
	Indices []int32
	Weights []float32
	Recip   bool    // the embedding kinds: score = 1 / (1 - s) (item_to_item.go:74-76)
	Scale   float64 // 0.5 for "auto", 1 otherwise (item_to_item.go:77-80)
}

// NeighbourScore is one entry of a user's list.
type NeighbourScore struct {
	Item  int32
	Score float64
}

type NeighbourRecommender struct{ h *C.gorse_nbr }

func nbrError(what string, rc C.int32_t) error {
	return errors.Errorf("%s: %s (%d)", what, C.GoString(C.gorse_hip_last_error()), int(rc))
}

func NewNeighbourRecommender(device, numItems int) (*NeighbourRecommender, error) {
	r := &NeighbourRecommender{}
	if rc := C.gorse_nbr_create(&r.h, C.int32_t(device), C.int64_t(numItems)); rc != C.GORSE_OK {
		return nil, nbrError("gorse_nbr_create", rc)
	}
	return r, nil
}

func (r *NeighbourRecommender) Close() {
	if r.h != nil {
		C.gorse_nbr_destroy(r.h)
		r.h = nil
	}
}

// SetTable replaces hop 1 (which = 0) or hop 2 (which = 1).
func (r *NeighbourRecommender) SetTable(which int, t NeighbourTable) error {
	var idx *C.int32_t
	var w *C.float
	if len(t.Indices) > 0 {
		idx = (*C.int32_t)(unsafe.Pointer(&t.Indices[0]))
		if t.Weights != nil {
			w = (*C.float)(unsafe.Pointer(&t.Weights[0]))
		}
	}
	transform := C.int32_t(C.GORSE_NBR_RAW)
	if t.Recip {
		transform = C.GORSE_NBR_RECIP
	}
	rc := C.gorse_nbr_set_table(r.h, C.int32_t(which), C.int64_t(len(t.Indptr)-1), (*C.int64_t)(unsafe.Pointer(&t.Indptr[0])), idx, w,
		transform, C.double(t.Scale))
	if rc != C.GORSE_OK {
		return nbrError("gorse_nbr_set_table", rc)
	}
	return nil
}

// NeighbourIndex is a similarity index resident on the device: exactly one of Dense (gorse_topk, the embedding kinds) and Sparse
// (gorse_sparse, the tags / users / items / auto kinds) is set.
type NeighbourIndex struct {
	Dense  *C.gorse_topk
	Sparse *C.gorse_sparse
}

// SetTableFromIndex replaces hop 1 (which = 0) or hop 2 (which = 1) by the neighbour lists of the index's stored rows, built on the
// device (gorse_nbr_set_table_from_topk / _from_sparse): row r is the list QueryItemToItem / QueryUserToUser form for stored row
// sources[r] (nil: the index's first numRows rows; a negative source: an empty row) -- QueryVectors(n + 1) under the index's current
// mask, the row itself skipped, scores <= 0 skipped for the Dot kinds (positiveOnly), cut at n -- with the index's row numbers as
// indices and the vector database's float32 score as raw weight.  recip and scale as in NeighbourTable.  The lists never cross to
// the host; the table equals the one SetTable is given after the same searches on the host, bit for bit.
func (r *NeighbourRecommender) SetTableFromIndex(which int, index NeighbourIndex, numRows int, sources []int64, n int, positiveOnly,
	recip bool, scale float64) error {
	var src *C.int64_t
	if sources != nil {
		numRows = len(sources)
		if numRows == 0 {
			sources = []int64{-1} // a table without rows: the pointer only has to be non-nil
		}
		src = (*C.int64_t)(unsafe.Pointer(&sources[0]))
	}
	transform := C.int32_t(C.GORSE_NBR_RAW)
	if recip {
		transform = C.GORSE_NBR_RECIP
	}
	positive := C.int32_t(0)
	if positiveOnly {
		positive = 1
	}
	var rc C.int32_t
	if index.Dense != nil {
		rc = C.gorse_nbr_set_table_from_topk(r.h, C.int32_t(which), index.Dense, C.int64_t(numRows), src, C.int32_t(n), positive, transform,
			C.double(scale))
	} else {
		rc = C.gorse_nbr_set_table_from_sparse(r.h, C.int32_t(which), index.Sparse, C.int64_t(numRows), src, C.int32_t(n), positive,
			transform, C.double(scale))
	}
	if rc != C.GORSE_OK {
		return nbrError("gorse_nbr_set_table_from_index", rc)
	}
	return nil
}

// Recommend returns for query t the n best candidates of a walk from hop-1 row rows[t] (negative: empty list) that are not in
// seen[t] (nil: no such rows).  RecommendSequential (recommend.go:135-156) adds every earlier recommender's results to the exclude
// set: the caller appends them to seen[t] before the next recommender's call.
func (r *NeighbourRecommender) Recommend(rows []int32, n int, seen [][]int32) ([][]NeighbourScore, error) {
	if seen != nil && len(seen) != len(rows) {
		return nil, errors.Errorf("Recommend: %d seen lists for %d queries", len(seen), len(rows))
	}
	out := make([][]NeighbourScore, len(rows))
	if len(rows) == 0 {
		return out, nil
	}
	var seenPtr *C.int64_t
	var seenIdx *C.int32_t
	if seen != nil {
		indptr := make([]int64, len(seen)+1)
		indices := make([]int32, 0, 1)
		for t, s := range seen {
			indices = append(indices, s...)
			indptr[t+1] = int64(len(indices))
		}
		if len(indices) == 0 {
			indices = append(indices, 0)
		}
		seenPtr = (*C.int64_t)(unsafe.Pointer(&indptr[0]))
		seenIdx = (*C.int32_t)(unsafe.Pointer(&indices[0]))
	}
	items := make([]int32, len(rows)*n)
	sums := make([]float64, len(rows)*n)
	counts := make([]int32, len(rows))
	rc := C.gorse_nbr_recommend(r.h, C.int64_t(len(rows)), (*C.int32_t)(unsafe.Pointer(&rows[0])), C.int32_t(n), seenPtr, seenIdx,
		(*C.int32_t)(unsafe.Pointer(&items[0])), (*C.double)(unsafe.Pointer(&sums[0])), (*C.int32_t)(unsafe.Pointer(&counts[0])))
	if rc != C.GORSE_OK {
		return nil, nbrError("gorse_nbr_recommend", rc)
	}
	for t := range rows {
		out[t] = make([]NeighbourScore, counts[t])
		for e := range out[t] {
			out[t][e] = NeighbourScore{Item: items[t*n+e], Score: sums[t*n+e]}
		}
	}
	return out, nil
}
