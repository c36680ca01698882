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
// seen[t] (nil: no such rows).  This is one recommender on its own.  RecommendSequential (recommend.go:135-156) adds every earlier
// recommender's results to the exclude set: CandidateChain below keeps that set on the device and runs this walk as one of its
// stages (AddNeighbour), so no caller has to append lists to seen[t] between two calls.
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

// CandidateChain is RecommendSequential (recommend.go:135-156, limit = 0) for many users with the exclude sets and the candidate
// lists resident on the device (gorse_cand): Begin uploads what NewRecommender puts into excludeSet, every Add* is one configured
// recommender -- filtered by the exclude set, its results added to the set before the next one runs --, Finish drops the candidates
// whose item is gone (worker/pipeline.go:228-243), and the CTR ranker takes its candidates from the chain (RankBy).  Per stage one row
// pointer crosses to the host.  Every attached handle numbers the items alike; mapping ids to indices stays the caller's.
type CandidateChain struct {
	h        *C.gorse_cand
	numItems int
	queries  int
}

// Candidate is one entry of a user's merged list: the recommender (stage) it came from, 0, 1, ... in Add* order.
type Candidate struct {
	Item  int32
	Score float64
	Stage uint8
}

func NewCandidateChain(device, numItems int) (*CandidateChain, error) {
	c := &CandidateChain{numItems: numItems}
	if rc := C.gorse_cand_create(&c.h, C.int32_t(device), C.int64_t(numItems)); rc != C.GORSE_OK {
		return nil, nbrError("gorse_cand_create", rc)
	}
	return c, nil
}

func (c *CandidateChain) Close() {
	if c.h != nil {
		C.gorse_cand_destroy(c.h)
		c.h = nil
	}
}

func flatten(rows [][]int32) ([]int64, []int32) {
	indptr := make([]int64, len(rows)+1)
	indices := make([]int32, 0, 1)
	for t, r := range rows {
		indices = append(indices, r...)
		indptr[t+1] = int64(len(indices))
	}
	if len(indices) == 0 {
		indices = append(indices, 0)
	}
	return indptr, indices
}

func keepPtr(keep []uint8) *C.uint8_t {
	if keep == nil {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&keep[0]))
}

func queryPtr(ids []int32) *C.int32_t {
	if len(ids) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&ids[0]))
}

// Begin starts a pass: exclude[t] is user t's exclude set as NewRecommender builds it (any order, repeats allowed; nil: empty sets),
// capacity the candidates one user can come to hold (the sum of the stages' n at least).
func (c *CandidateChain) Begin(numQueries int, exclude [][]int32, capacity int) error {
	var ptr *C.int64_t
	var idx *C.int32_t
	if exclude != nil {
		if len(exclude) != numQueries {
			return errors.Errorf("Begin: %d exclude sets for %d queries", len(exclude), numQueries)
		}
		indptr, indices := flatten(exclude)
		ptr = (*C.int64_t)(unsafe.Pointer(&indptr[0]))
		idx = (*C.int32_t)(unsafe.Pointer(&indices[0]))
	}
	if rc := C.gorse_cand_begin(c.h, C.int64_t(numQueries), ptr, idx, C.int32_t(capacity)); rc != C.GORSE_OK {
		return nbrError("gorse_cand_begin", rc)
	}
	c.queries = numQueries
	return nil
}

// AddCollaborative is recommendCollaborative behind updateCollaborativeRecommend (pipeline.go:197-204): the search runs under the
// exclude sets as Begin got them, the chain's filter applies the current ones.  mf is the model's gorse_mf handle (model/cf/hip.go);
// users[t] < 0: nothing for query t; itemOK nil: IsItemPredictable.
func (c *CandidateChain) AddCollaborative(mf unsafe.Pointer, users []int32, n int, itemOK, keep []uint8) error {
	rc := C.gorse_cand_add_mf(c.h, (*C.gorse_mf)(mf), queryPtr(users), C.int32_t(n), keepPtr(itemOK), keepPtr(keep))
	if rc != C.GORSE_OK {
		return nbrError("gorse_cand_add_mf", rc)
	}
	return nil
}

// AddNeighbour is recommendItemToItem or recommendUserToUser: NeighbourRecommender.Recommend with seen = the chain's current
// exclude sets, read on the device.  keep is recommendUserToUser's data-store filter (:317-345; nil: keep all): what it drops is
// neither a candidate nor excluded later.
func (c *CandidateChain) AddNeighbour(r *NeighbourRecommender, rows []int32, n int, keep []uint8) error {
	if rc := C.gorse_cand_add_nbr(c.h, r.h, queryPtr(rows), C.int32_t(n), keepPtr(keep)); rc != C.GORSE_OK {
		return nbrError("gorse_cand_add_nbr", rc)
	}
	return nil
}

// AddShared is recommendLatest / recommendNonPersonalized: one list, in its final order, for every user.
func (c *CandidateChain) AddShared(list []NeighbourScore, n int, keep []uint8) error {
	items := make([]int32, len(list)+1)
	scores := make([]float64, len(list)+1)
	for e, s := range list {
		items[e], scores[e] = s.Item, s.Score
	}
	rc := C.gorse_cand_add_shared(c.h, C.int64_t(len(list)), (*C.int32_t)(unsafe.Pointer(&items[0])), (*C.double)(unsafe.Pointer(&scores[0])),
		C.int32_t(n), keepPtr(keep))
	if rc != C.GORSE_OK {
		return nbrError("gorse_cand_add_shared", rc)
	}
	return nil
}

// AddLists is a recommender whose lists exist on the host: an external recommender, or lists read back from a cache.
func (c *CandidateChain) AddLists(lists [][]NeighbourScore, n int, keep []uint8) error {
	if len(lists) != c.queries {
		return errors.Errorf("AddLists: %d lists for %d queries", len(lists), c.queries)
	}
	indptr := make([]int64, len(lists)+1)
	items := make([]int32, 0, 1)
	scores := make([]float64, 0, 1)
	for t, l := range lists {
		for _, s := range l {
			items = append(items, s.Item)
			scores = append(scores, s.Score)
		}
		indptr[t+1] = int64(len(items))
	}
	if len(items) == 0 {
		items, scores = append(items, 0), append(scores, 0)
	}
	rc := C.gorse_cand_add_lists(c.h, (*C.int64_t)(unsafe.Pointer(&indptr[0])), (*C.int32_t)(unsafe.Pointer(&items[0])),
		(*C.double)(unsafe.Pointer(&scores[0])), C.int32_t(n), keepPtr(keep))
	if rc != C.GORSE_OK {
		return nbrError("gorse_cand_add_lists", rc)
	}
	return nil
}

// Finish closes the pass; exists[i] == 0 drops item i's candidates (pipeline.go:228-243; nil: all exist).
func (c *CandidateChain) Finish(exists []uint8) error {
	if rc := C.gorse_cand_finish(c.h, keepPtr(exists)); rc != C.GORSE_OK {
		return nbrError("gorse_cand_finish", rc)
	}
	return nil
}

// Candidates returns the finished pass: every user's merged list in stage order.
func (c *CandidateChain) Candidates() ([][]Candidate, error) {
	var nq, nc C.int64_t
	if rc := C.gorse_cand_info(c.h, &nq, nil, &nc, nil); rc != C.GORSE_OK {
		return nil, nbrError("gorse_cand_info", rc)
	}
	indptr := make([]int64, int(nq)+1)
	items := make([]int32, int(nc)+1)
	scores := make([]float64, int(nc)+1)
	stages := make([]uint8, int(nc)+1)
	rc := C.gorse_cand_get(c.h, (*C.int64_t)(unsafe.Pointer(&indptr[0])), (*C.int32_t)(unsafe.Pointer(&items[0])),
		(*C.double)(unsafe.Pointer(&scores[0])), (*C.uint8_t)(unsafe.Pointer(&stages[0])))
	if rc != C.GORSE_OK {
		return nil, nbrError("gorse_cand_get", rc)
	}
	out := make([][]Candidate, int(nq))
	for t := range out {
		out[t] = make([]Candidate, 0, indptr[t+1]-indptr[t])
		for e := indptr[t]; e < indptr[t+1]; e++ {
			out[t] = append(out[t], Candidate{Item: items[e], Score: scores[e], Stage: stages[e]})
		}
	}
	return out, nil
}

// ExcludeSets returns the current exclude sets, ascending, at any time of a pass.
func (c *CandidateChain) ExcludeSets() ([][]int32, error) {
	var nq, nx C.int64_t
	if rc := C.gorse_cand_info(c.h, &nq, nil, nil, &nx); rc != C.GORSE_OK {
		return nil, nbrError("gorse_cand_info", rc)
	}
	indptr := make([]int64, int(nq)+1)
	items := make([]int32, int(nx)+1)
	if rc := C.gorse_cand_get_exclusion(c.h, (*C.int64_t)(unsafe.Pointer(&indptr[0])), (*C.int32_t)(unsafe.Pointer(&items[0]))); rc != C.GORSE_OK {
		return nil, nbrError("gorse_cand_get_exclusion", rc)
	}
	out := make([][]int32, int(nq))
	for t := range out {
		out[t] = items[indptr[t]:indptr[t+1]]
	}
	return out, nil
}

// UserRows is the user side of rankByClickTroughRate as gorse_fm_rank_users takes it: one feature row per query.
type UserRows struct {
	Indptr  []int64
	Indices []int32
	Values  []float32
	Lead    []int32 // nil: 0 for every user
}

// RankBy scores and orders every user's finished candidates by the CTR model (gorse_fm_rank_cand; fm is the model's gorse_fm handle,
// model/ctr/fm_hip.go, with its item catalogue resident): scores and order are flat in the layout of Candidates(), order[p + r] = the
// position inside the user's list of its r-th ranked candidate.
func (c *CandidateChain) RankBy(fm unsafe.Pointer, users UserRows, batchSize int) ([]float32, []int32, error) {
	var nc C.int64_t
	if rc := C.gorse_cand_info(c.h, nil, nil, &nc, nil); rc != C.GORSE_OK {
		return nil, nil, nbrError("gorse_cand_info", rc)
	}
	scores := make([]float32, int(nc)+1)
	order := make([]int32, int(nc)+1)
	indices, values := users.Indices, users.Values
	if len(indices) == 0 {
		indices, values = []int32{0}, []float32{0}
	}
	var lead *C.int32_t
	if users.Lead != nil {
		lead = (*C.int32_t)(unsafe.Pointer(&users.Lead[0]))
	}
	rc := C.gorse_fm_rank_cand((*C.gorse_fm)(fm), c.h, (*C.int64_t)(unsafe.Pointer(&users.Indptr[0])), (*C.int32_t)(unsafe.Pointer(&indices[0])),
		(*C.float)(unsafe.Pointer(&values[0])), lead, C.int32_t(batchSize), nil, (*C.float)(unsafe.Pointer(&scores[0])),
		(*C.int32_t)(unsafe.Pointer(&order[0])))
	if rc != C.GORSE_OK {
		return nil, nil, nbrError("gorse_fm_rank_cand", rc)
	}
	return scores[:nc], order[:nc], nil
}

// Feedback kinds of AddReplacement: what the caller's match against the positive and the read feedback type expressions gave
// (worker/pipeline.go:584-589); feedback that matches neither is left out.
const (
	HistoryPositive uint8 = C.GORSE_CAND_KIND_POSITIVE
	HistoryRead     uint8 = C.GORSE_CAND_KIND_READ
	// StageReplacement is the Stage of a candidate that AddReplacement appended.
	StageReplacement uint8 = C.GORSE_CAND_STAGE_REPLACEMENT
)

// HistoryItem is one feedback of a user's history: the item and what its type matched.
type HistoryItem struct {
	Item int32
	Kind uint8
}

// AddReplacement is addReplacementCandidates (worker/pipeline.go:573-615) for every user of a finished pass: history[t] is user t's
// feedback (any order, repeats allowed, an item with both kinds is positive), exists[i] == 0 says item i is gone or hidden
// (ItemCache.GetSlice; nil: all exist).  The distinct existing items that are no candidates yet are appended, ascending, with score 0
// and StageReplacement; Candidates and RankBy read the grown lists.  Once per pass; the exclude sets are not touched.
func (c *CandidateChain) AddReplacement(history [][]HistoryItem, exists []uint8) error {
	if len(history) != c.queries {
		return errors.Errorf("AddReplacement: %d histories for %d queries", len(history), c.queries)
	}
	indptr := make([]int64, len(history)+1)
	items := make([]int32, 0, 1)
	kinds := make([]uint8, 0, 1)
	for t, h := range history {
		for _, f := range h {
			items = append(items, f.Item)
			kinds = append(kinds, f.Kind)
		}
		indptr[t+1] = int64(len(items))
	}
	if len(items) == 0 {
		items, kinds = append(items, 0), append(kinds, HistoryPositive)
	}
	rc := C.gorse_cand_add_replacement(c.h, (*C.int64_t)(unsafe.Pointer(&indptr[0])), (*C.int32_t)(unsafe.Pointer(&items[0])),
		(*C.uint8_t)(unsafe.Pointer(&kinds[0])), keepPtr(exists))
	if rc != C.GORSE_OK {
		return nbrError("gorse_cand_add_replacement", rc)
	}
	return nil
}

// RankByDecayed is RankBy followed by applyReplacementDecay (worker/pipeline.go:617-643) on the device
// (gorse_fm_rank_cand_decayed): final[p + r] is candidate r's score, multiplied by positiveDecay or readDecay where its item is in
// the user's history (appended or found by a recommender on its own), and order[p + r] the position of the r-th entry under
// descending final, ties and NaNs in RankBy's order -- one of the orders the reference's sort.Slice can produce.
func (c *CandidateChain) RankByDecayed(fm unsafe.Pointer, users UserRows, batchSize int, positiveDecay, readDecay float64) ([]float64, []int32, error) {
	var nc C.int64_t
	if rc := C.gorse_cand_info(c.h, nil, nil, &nc, nil); rc != C.GORSE_OK {
		return nil, nil, nbrError("gorse_cand_info", rc)
	}
	final := make([]float64, int(nc)+1)
	order := make([]int32, int(nc)+1)
	indices, values := users.Indices, users.Values
	if len(indices) == 0 {
		indices, values = []int32{0}, []float32{0}
	}
	var lead *C.int32_t
	if users.Lead != nil {
		lead = (*C.int32_t)(unsafe.Pointer(&users.Lead[0]))
	}
	rc := C.gorse_fm_rank_cand_decayed((*C.gorse_fm)(fm), c.h, (*C.int64_t)(unsafe.Pointer(&users.Indptr[0])),
		(*C.int32_t)(unsafe.Pointer(&indices[0])), (*C.float)(unsafe.Pointer(&values[0])), lead, C.int32_t(batchSize), nil,
		C.double(positiveDecay), C.double(readDecay), nil, (*C.double)(unsafe.Pointer(&final[0])), (*C.int32_t)(unsafe.Pointer(&order[0])))
	if rc != C.GORSE_OK {
		return nil, nil, nbrError("gorse_fm_rank_cand_decayed", rc)
	}
	return final[:nc], order[:nc], nil
}
