//go:build cgo && hip && !xla

package ctr

// #include <stdlib.h>
// #include "gorse_hip.h"
import "C"

import (
	"context"
	"fmt"
	"sync/atomic"
	"time"
	"unsafe"

	"github.com/chewxy/math32"
	"github.com/gorse-io/gorse/common/log"
	"github.com/gorse-io/gorse/common/monitor"
	"github.com/gorse-io/gorse/common/nn"
	"github.com/gorse-io/gorse/dataset"
	"github.com/gorse-io/gorse/model"
	"github.com/samber/lo"
	"go.uber.org/zap"
)

// hipFM keeps the factorization machine resident on one MI355X between Fit and the BatchInternalPredict calls that follow.
type hipFM struct {
	h *C.gorse_fm
}

func (m *hipFM) close() {
	if m != nil && m.h != nil {
		C.gorse_fm_destroy(m.h)
		m.h = nil
	}
}

// flatRows pads x to width columns (index 0 / value 0), the layout of convertToTensors (fm.go:527-577).
func flatRows(x []lo.Tuple2[[]int32, []float32], width int) ([]int32, []float32) {
	idx := make([]int32, len(x)*width)
	val := make([]float32, len(x)*width)
	for i := range x {
		copy(idx[i*width:], x[i].A)
		copy(val[i*width:], x[i].B)
	}
	return idx, val
}

// flatEmbeddings lays field k's embeddings of the rows out as one n x D matrix of bf16 bit patterns, straight from the rows'
// []uint16 (no fp32 copy): an all-zero row where a sample has none or one of another length (fm.go:555-561).
func flatEmbeddings(e [][][]uint16, n, k, dim int) []uint16 {
	out := make([]uint16, n*dim)
	for i := 0; i < n && i < len(e); i++ {
		if len(e[i]) > k && len(e[i][k]) == dim {
			copy(out[i*dim:], e[i][k])
		}
	}
	return out
}

// fieldTensors returns field k's tensors in Parameters() order (fm.go:136-146, layers.go:173-178): H, Wa, ba, We, be.
func (fm *AFM) fieldTensors(k int) [5][]float32 {
	a := fm.A[k].(*nn.Attention)
	aw := a.W.(*nn.LinearLayer)
	e := fm.E[k].(*nn.LinearLayer)
	return [5][]float32{a.H.Data(), aw.W.Data(), aw.B.Data(), e.W.Data(), e.B.Data()}
}

// fitHIP is AFM.Fit (fm.go:307-417), with or without item embeddings: one gorse_fm_epoch call per epoch; the evaluation
// schedule, the NaN stop and early stopping stay here as written.  It is called right after Init (fm.go:315-322), before the
// reference's epoch-0 evaluation, and builds the scaled training rows itself (fm.go:337-352).  ok = false sends the caller back
// to the CPU code (no device, or a model or training set the device refuses: GORSE_ERR_INVALID beyond the caps of
// gorse_hip.h, GORSE_ERR_NOMEM when the embeddings do not fit) with no handle left resident.
func (fm *AFM) fitHIP(ctx context.Context, trainSet, testSet dataset.CTRSplit, config *FitConfig) (score Score, ok bool) {
	fm.hip.close() // the previous Fit's device model must not score this one's epoch 0
	fm.hip = nil
	if trainSet.Count() == 0 {
		return Score{}, false
	}
	x := make([]lo.Tuple2[[]int32, []float32], trainSet.Count())
	y := make([]float32, trainSet.Count())
	e := make([][][]uint16, trainSet.Count())
	for i := range x {
		indices, values, embeddings, target := trainSet.Get(i)
		e[i] = embeddings
		scaled := make([]float32, len(values))
		copy(scaled, values)
		for j, idx := range indices {
			if scaler, ok := fm.Scalers[idx]; ok {
				scaled[j] = scaler.Transform(values[j])
			}
		}
		x[i], y[i] = lo.Tuple2[[]int32, []float32]{A: indices, B: scaled}, target
	}
	hm := &hipFM{}
	if rc := C.gorse_fm_create(&hm.h, 0, C.int64_t(fm.numFeatures), C.int32_t(fm.nFactors)); rc != 0 {
		log.Logger().Warn("fit AFM: no device, CPU path", zap.String("err", C.GoString(C.gorse_hip_last_error())))
		return Score{}, false
	}
	// Init drew B, W and V in Go (fm.go:247-270); the nn tensors hold them
	width := max(fm.numDimension, 1)
	idx, val := flatRows(x, width)
	giveUp := func(what string) (Score, bool) {
		log.Logger().Warn("fit AFM: "+what+", CPU path", zap.String("err", C.GoString(C.gorse_hip_last_error())))
		hm.close()
		return Score{}, false
	}
	if len(fm.embeddingDim) != 0 { // more than GORSE_FM_MAX_FIELDS fields or a dimension above the cap: GORSE_ERR_INVALID
		dims := make([]C.int32_t, len(fm.embeddingDim))
		for k, dim := range fm.embeddingDim {
			dims[k] = C.int32_t(dim)
		}
		if rc := C.gorse_fm_set_embedding_dims(hm.h, C.int32_t(len(dims)), &dims[0]); rc != 0 {
			return giveUp("gorse_fm_set_embedding_dims")
		}
	}
	if rc := C.gorse_fm_set_params(hm.h, C.float(fm.B.Data()[0]), (*C.float)(&fm.W.Data()[0]), (*C.float)(&fm.V.Data()[0])); rc != 0 {
		return giveUp("gorse_fm_set_params")
	}
	for k := range fm.embeddingDim { // Init drew A[k] and E[k] in Go as well (fm.go:259-264)
		t := fm.fieldTensors(k)
		if rc := C.gorse_fm_set_embedding_params(hm.h, C.int32_t(k), (*C.float)(&t[0][0]), (*C.float)(&t[1][0]), (*C.float)(&t[2][0]),
			(*C.float)(&t[3][0]), (*C.float)(&t[4][0])); rc != 0 {
			return giveUp("gorse_fm_set_embedding_params")
		}
	}
	if rc := C.gorse_fm_set_train(hm.h, C.int64_t(len(y)), C.int32_t(width), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
		(*C.float)(&y[0])); rc != 0 { // e.g. more than 2^31 - 1 padded positions (GORSE_ERR_INVALID)
		log.Logger().Warn("fit AFM: gorse_fm_set_train, CPU path", zap.String("err", C.GoString(C.gorse_hip_last_error())))
		hm.close()
		return Score{}, false
	}
	for k, dim := range fm.embeddingDim { // bf16 as stored, one field at a time; GORSE_ERR_NOMEM when it does not fit
		emb := flatEmbeddings(e, len(y), k, dim)
		if rc := C.gorse_fm_set_train_embeddings(hm.h, C.int32_t(k), (*C.uint16_t)(&emb[0])); rc != 0 {
			return giveUp("gorse_fm_set_train_embeddings")
		}
	}
	fm.hip = hm
	opt := C.int32_t(C.GORSE_OPT_ADAM)
	if fm.optimizer == model.SGD {
		opt = C.GORSE_OPT_SGD
	}
	cancel := (*C.int32_t)(C.malloc(4)) // C memory: the library reads the flag during the call
	defer C.free(unsafe.Pointer(cancel))
	*cancel = 0
	stop := context.AfterFunc(ctx, func() { atomic.StoreInt32((*int32)(unsafe.Pointer(cancel)), 1) })
	defer stop()

	// the test split goes to the device once; every evaluation of this Fit then uploads nothing (resident = false: the
	// reference's EvaluateClassification, which gathers, uploads and sorts per call, stays the route)
	resident := fm.setTestHIP(testSet)
	evaluate := func() Score {
		if resident {
			if s, ok := fm.evaluateResidentHIP(testSet); ok {
				return s
			}
		}
		return EvaluateClassification(fm, testSet, config.Jobs)
	}
	score = evaluate()
	scores := []lo.Tuple2[int, float32]{{A: 0, B: score.AUC}}
	_, span := monitor.Start(ctx, "FM.Fit", fm.nEpochs)
	defer span.End()
	for epoch := 1; epoch <= fm.nEpochs; epoch++ {
		fitStart := time.Now()
		var cost C.float
		rc := C.gorse_fm_epoch(hm.h, C.int32_t(fm.batchSize), opt, C.float(fm.lr), C.float(fm.reg), cancel, &cost)
		if rc == C.GORSE_ERR_CANCELLED {
			log.Logger().Info("fit AFM canceled", zap.Error(ctx.Err()))
			fm.pullParams()
			return Score{}, true
		} else if rc != 0 {
			// a device failure mid-Fit: keep the steps taken in the nn tensors, drop the handle (later scoring runs on the CPU)
			log.Logger().Error("fit AFM", zap.String("err", C.GoString(C.gorse_hip_last_error())))
			fm.pullParams()
			fm.hip.close()
			fm.hip = nil
			return Score{}, true
		}
		fitTime := time.Since(fitStart)
		if epoch%config.Verbose == 0 || epoch == fm.nEpochs {
			evalStart := time.Now()
			score = evaluate() // gorse_fm_evaluate on the resident split
			scores = append(scores, lo.Tuple2[int, float32]{A: epoch, B: score.AUC})
			log.Logger().Info(fmt.Sprintf("fit AFM %v/%v", epoch, fm.nEpochs), append([]zap.Field{
				zap.String("fit_time", fitTime.String()),
				zap.String("eval_time", time.Since(evalStart).String()),
				zap.Float32("loss", float32(cost)),
			}, score.ZapFields()...)...)
			if math32.IsNaN(float32(cost)) || math32.IsNaN(score.GetValue()) {
				log.Logger().Warn("model diverged", zap.Float32("lr", fm.lr))
				break
			}
			if config.Patience > 0 && epoch > config.Patience {
				epochScore := lo.MaxBy(scores, func(a, b lo.Tuple2[int, float32]) bool { return a.B > b.B })
				if epochScore.A <= epoch-config.Patience {
					log.Logger().Info("early stopping", zap.Int("best_epoch", epochScore.A),
						zap.Float32("best_auc", epochScore.B), zap.Int("patience", config.Patience))
					break
				}
			}
		}
		span.Add(1)
	}
	fm.pullParams()
	return score, true
}

// setTestHIP makes the test split resident (gorse_fm_set_test): the rows scaled and padded as BatchInternalPredict has them
// (applyScalers, convertToTensors), the targets, and every field's embeddings as one n x D bf16 matrix.  The library partitions
// them into positives (target > 0) and the rest and gathers the embedding rows once.  false: nothing resident (an empty split, or
// one the device refuses: GORSE_ERR_NOMEM when it does not fit).
func (fm *AFM) setTestHIP(testSet dataset.CTRSplit) bool {
	n := testSet.Count()
	if fm.hip == nil || n == 0 {
		return false
	}
	x := make([]lo.Tuple2[[]int32, []float32], n)
	y := make([]float32, n)
	e := make([][][]uint16, n)
	width := max(fm.numDimension, 1)
	for i := range x {
		indices, values, embeddings, target := testSet.Get(i)
		e[i] = embeddings
		scaled := make([]float32, len(values))
		copy(scaled, values)
		for j, idx := range indices {
			if scaler, ok := fm.Scalers[idx]; ok {
				scaled[j] = scaler.Transform(values[j])
			}
		}
		x[i], y[i] = lo.Tuple2[[]int32, []float32]{A: indices, B: scaled}, target
		width = max(width, len(indices))
	}
	idx, val := flatRows(x, width)
	var embPtr **C.uint16_t
	if len(fm.embeddingDim) != 0 {
		// the matrices live in C memory for the call: a Go pointer to Go pointers must not cross cgo
		ptrs := (*[C.GORSE_FM_MAX_FIELDS]*C.uint16_t)(C.malloc(C.size_t(C.GORSE_FM_MAX_FIELDS) * C.size_t(unsafe.Sizeof(uintptr(0)))))
		defer C.free(unsafe.Pointer(ptrs))
		for k, dim := range fm.embeddingDim {
			emb := flatEmbeddings(e, n, k, dim)
			ptrs[k] = (*C.uint16_t)(C.CBytes(unsafe.Slice((*byte)(unsafe.Pointer(&emb[0])), 2*len(emb))))
			defer C.free(unsafe.Pointer(ptrs[k]))
		}
		embPtr = &ptrs[0]
	}
	if rc := C.gorse_fm_set_test(fm.hip.h, C.int64_t(n), C.int32_t(width), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
		(*C.float)(&y[0]), embPtr); rc != 0 {
		log.Logger().Warn("fit AFM: gorse_fm_set_test, evaluating through BatchInternalPredict",
			zap.String("err", C.GoString(C.gorse_hip_last_error())))
		return false
	}
	return true
}

// evaluateResidentHIP is EvaluateClassification (evaluator.go:46-83) from the resident split: the device scores both sides and
// returns the counts Precision, Recall, Accuracy and AUC (evaluator.go:85-153) are formed from.  Their float32 counters
// (tp++, fp++, correct++) stop growing at 2^24, so a count enters as min(count, 2^24); auc_sum is the reference's own running
// float32 sum.  ok = false (a failure, or a NaN logit: the metrics' own loops then decide) sends the caller to the reference's code.
func (fm *AFM) evaluateResidentHIP(testSet dataset.CTRSplit) (Score, bool) {
	var counts [C.GORSE_FM_EVAL_COUNTS]C.int64_t
	var aucSum C.float
	if rc := C.gorse_fm_evaluate(fm.hip.h, C.int32_t(fm.batchSize), nil, &counts[0], &aucSum, nil); rc != 0 {
		log.Logger().Error("evaluate AFM", zap.String("err", C.GoString(C.gorse_hip_last_error())))
		return Score{}, false
	}
	if counts[5] > 0 {
		return Score{}, false
	}
	counter := func(c C.int64_t) float32 { return float32(min(int64(c), 1<<24)) }
	nPos, nNeg := int(counts[0]), int(counts[1])
	tp, fp, fn := counter(counts[2]), counter(counts[3]), counter(counts[0]-counts[2])
	var s Score
	if tp+fp != 0 {
		s.Precision = tp / (tp + fp)
	}
	if tp+fn != 0 {
		s.Recall = tp / (tp + fn)
	}
	s.Accuracy = counter(counts[2]+counts[4]) / float32(nPos+nNeg)
	if nPos*nNeg != 0 {
		s.AUC = float32(aucSum) / float32(nPos*nNeg)
	}
	return s, true
}

// pullParams copies the device's parameters back into the nn tensors; nn.Save (Marshal) then writes them as today.
func (fm *AFM) pullParams() {
	var b C.float
	if rc := C.gorse_fm_get_params(fm.hip.h, &b, (*C.float)(&fm.W.Data()[0]), (*C.float)(&fm.V.Data()[0])); rc != 0 {
		log.Logger().Error("fit AFM: gorse_fm_get_params", zap.String("err", C.GoString(C.gorse_hip_last_error())))
		return
	}
	fm.B.Data()[0] = float32(b)
	for k := range fm.embeddingDim {
		t := fm.fieldTensors(k)
		if rc := C.gorse_fm_get_embedding_params(fm.hip.h, C.int32_t(k), (*C.float)(&t[0][0]), (*C.float)(&t[1][0]), (*C.float)(&t[2][0]),
			(*C.float)(&t[3][0]), (*C.float)(&t[4][0])); rc != 0 {
			log.Logger().Error("fit AFM: gorse_fm_get_embedding_params", zap.String("err", C.GoString(C.gorse_hip_last_error())))
			return
		}
	}
}

// batchPredictHIP is BatchInternalPredict (fm.go:156-178) on the device for already scaled rows and their embeddings; ok = false
// when the model is not resident (loaded by Unmarshal without a Fit in this process).  With item embeddings the rows are scored in
// slices of fm.batchSize rows, as the reference does: its Softmax makes the slice length part of the result.
func (fm *AFM) batchPredictHIP(x []lo.Tuple2[[]int32, []float32], e [][][]uint16) ([]float32, bool) {
	if fm.hip == nil || fm.hip.h == nil {
		return nil, false
	}
	out := make([]float32, len(x))
	if len(x) == 0 {
		return out, true
	}
	width := max(fm.numDimension, 1)
	for i := range x {
		width = max(width, len(x[i].A))
	}
	idx, val := flatRows(x, width)
	if len(fm.embeddingDim) == 0 {
		if rc := C.gorse_fm_predict(fm.hip.h, C.int64_t(len(x)), C.int32_t(width), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
			(*C.float)(&out[0])); rc != 0 {
			return nil, false
		}
		return out, true
	}
	// the field matrices live in C memory for the call: a Go pointer to Go pointers must not cross cgo
	ptrs := (*[C.GORSE_FM_MAX_FIELDS]*C.uint16_t)(C.malloc(C.size_t(C.GORSE_FM_MAX_FIELDS) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(ptrs))
	for k, dim := range fm.embeddingDim {
		emb := flatEmbeddings(e, len(x), k, dim)
		ptrs[k] = (*C.uint16_t)(C.CBytes(unsafe.Slice((*byte)(unsafe.Pointer(&emb[0])), 2*len(emb))))
		defer C.free(unsafe.Pointer(ptrs[k]))
	}
	if rc := C.gorse_fm_predict_embeddings(fm.hip.h, C.int64_t(len(x)), C.int32_t(width), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
		&ptrs[0], C.int32_t(fm.batchSize), (*C.float)(&out[0])); rc != 0 {
		return nil, false
	}
	return out, true
}

// RankItem is one catalogue entry of setItemsHIP as BatchPredict would encode it (fm.go:189-206): the item-id entry first when the
// index knows the item, then the item labels it knows, values already scaled; Embeddings[k] is field k's vector or nil.
type RankItem struct {
	Indices    []int32
	Values     []float32
	Lead       int32 // 1 when the item-id entry is there, else 0
	Embeddings [][]uint16
}

// EncodeRankItem / EncodeRankUser do BatchPredict's encoding (fm.go:183-206) for one side; the scalers are applied here, as
// BatchInternalPredict applies them (fm.go:160-165), because values reach the library scaled.
func (fm *AFM) EncodeRankItem(itemId string, labels []Label, embeddings []Embedding) RankItem {
	var x lo.Tuple2[[]int32, []float32]
	item := RankItem{Embeddings: make([][]uint16, len(fm.embeddingDim))}
	if itemIndex := fm.Index.EncodeItem(itemId); itemIndex != dataset.NotId {
		x.A, x.B = append(x.A, itemIndex), append(x.B, 1)
		item.Lead = 1
	}
	for _, f := range labels {
		if index := fm.Index.EncodeItemLabel(f.Name); index != dataset.NotId {
			x.A, x.B = append(x.A, index), append(x.B, f.Value)
		}
	}
	if fm.autoScale {
		x = fm.applyScalers([]lo.Tuple2[[]int32, []float32]{x})[0]
	}
	item.Indices, item.Values = x.A, x.B
	if fm.embeddingIndex != nil {
		for _, embedding := range embeddings {
			k := fm.embeddingIndex.ToNumber(embedding.Name)
			if k == dataset.NotId || len(embedding.Value) != fm.embeddingDim[int(k)] {
				continue // unknown embedding or dimension mismatch (fm.go:216-224)
			}
			item.Embeddings[int(k)] = embedding.Value
		}
	}
	return item
}

func (fm *AFM) EncodeRankUser(userId string, labels []Label) (indices []int32, values []float32, lead int32) {
	var x lo.Tuple2[[]int32, []float32]
	if userIndex := fm.Index.EncodeUser(userId); userIndex != dataset.NotId {
		x.A, x.B = append(x.A, userIndex), append(x.B, 1)
		lead = 1
	}
	for _, f := range labels {
		if index := fm.Index.EncodeUserLabel(f.Name); index != dataset.NotId {
			x.A, x.B = append(x.A, index), append(x.B, f.Value)
		}
	}
	if fm.autoScale {
		x = fm.applyScalers([]lo.Tuple2[[]int32, []float32]{x})[0]
	}
	return x.A, x.B, lead
}

// setItemsHIP makes the catalogue resident on the device (gorse_fm_set_items); ok = false when no model is resident or the
// library refuses the catalogue (it then keeps the previous one).
func (fm *AFM) setItemsHIP(items []RankItem) bool {
	if fm.hip == nil || fm.hip.h == nil {
		return false
	}
	n := len(items)
	indptr := make([]int64, n+1)
	lead := make([]int32, max(n, 1))
	var idx []int32
	var val []float32
	for i, item := range items {
		idx = append(idx, item.Indices...)
		val = append(val, item.Values...)
		indptr[i+1] = int64(len(idx))
		lead[i] = item.Lead
	}
	if len(idx) == 0 {
		idx, val = []int32{0}, []float32{0}
	}
	var embPtr **C.uint16_t
	if len(fm.embeddingDim) > 0 && n > 0 {
		// the tables live in C memory for the call: a Go pointer to Go pointers must not cross cgo
		ptrs := (*[C.GORSE_FM_MAX_FIELDS]*C.uint16_t)(C.malloc(C.size_t(C.GORSE_FM_MAX_FIELDS) * C.size_t(unsafe.Sizeof(uintptr(0)))))
		defer C.free(unsafe.Pointer(ptrs))
		for k, dim := range fm.embeddingDim {
			table := make([]uint16, n*dim) // an all-zero row where the item has no embedding (fm.go:555-561)
			for i, item := range items {
				if len(item.Embeddings) > k && len(item.Embeddings[k]) == dim {
					copy(table[i*dim:], item.Embeddings[k])
				}
			}
			ptrs[k] = (*C.uint16_t)(C.CBytes(unsafe.Slice((*byte)(unsafe.Pointer(&table[0])), 2*len(table))))
			defer C.free(unsafe.Pointer(ptrs[k]))
		}
		embPtr = &ptrs[0]
	}
	rc := C.gorse_fm_set_items(fm.hip.h, C.int64_t(n), (*C.int64_t)(&indptr[0]), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
		(*C.int32_t)(&lead[0]), embPtr)
	return rc == 0
}

// RankUser is one user of rankUsersHIP: its encoded row and its candidates as catalogue rows.
type RankUser struct {
	Indices    []int32
	Values     []float32
	Lead       int32
	Candidates []int32
}

// rankUsersHIP scores and ranks every user's candidates in one gorse_fm_rank_users call.  scores[t][r] belongs to
// users[t].Candidates[r]; order[t] lists the positions of user t's candidates best first: descending score, equal scores by
// position, NaN last -- one of the orders sort.Slice(score >) of cache.SortDocuments can produce (it is not stable).
func (fm *AFM) rankUsersHIP(ctx context.Context, users []RankUser) (scores [][]float32, order [][]int32, ok bool) {
	if fm.hip == nil || fm.hip.h == nil || len(users) == 0 {
		return nil, nil, false
	}
	n := len(users)
	uptr, cptr := make([]int64, n+1), make([]int64, n+1)
	lead := make([]int32, n)
	var idx, cand []int32
	var val []float32
	for t, u := range users {
		idx = append(idx, u.Indices...)
		val = append(val, u.Values...)
		cand = append(cand, u.Candidates...)
		uptr[t+1], cptr[t+1] = int64(len(idx)), int64(len(cand))
		lead[t] = u.Lead
	}
	if len(cand) == 0 {
		return make([][]float32, n), make([][]int32, n), true
	}
	if len(idx) == 0 {
		idx, val = []int32{0}, []float32{0}
	}
	flatScores, flatOrder := make([]float32, len(cand)), make([]int32, len(cand))
	cancel := (*C.int32_t)(C.calloc(1, 4)) // C memory: the watcher writes it while the call runs
	defer C.free(unsafe.Pointer(cancel))
	done := make(chan struct{})
	defer close(done)
	go func() {
		select {
		case <-ctx.Done():
			atomic.StoreInt32((*int32)(unsafe.Pointer(cancel)), 1)
		case <-done:
		}
	}()
	rc := C.gorse_fm_rank_users(fm.hip.h, C.int64_t(n), (*C.int64_t)(&uptr[0]), (*C.int32_t)(&idx[0]), (*C.float)(&val[0]),
		(*C.int32_t)(&lead[0]), (*C.int64_t)(&cptr[0]), (*C.int32_t)(&cand[0]), C.int32_t(fm.batchSize), cancel,
		(*C.float)(&flatScores[0]), (*C.int32_t)(&flatOrder[0]))
	if rc != 0 {
		return nil, nil, false
	}
	scores, order = make([][]float32, n), make([][]int32, n)
	for t := range users {
		scores[t], order[t] = flatScores[cptr[t]:cptr[t+1]], flatOrder[cptr[t]:cptr[t+1]]
	}
	return scores, order, true
}

// SetRankItems / RankUsers are what the worker calls (worker/pipeline_hip.go).
func (fm *AFM) SetRankItems(items []RankItem) bool { return fm.setItemsHIP(items) }

func (fm *AFM) RankUsers(ctx context.Context, users []RankUser) ([][]float32, [][]int32, bool) {
	return fm.rankUsersHIP(ctx, users)
}

// SampleSide is the user side of a set in sample form: one encoded row per user (EncodeRankUser), as rankUsersHIP takes them.
type SampleSide struct {
	Indices [][]int32
	Values  [][]float32
	Lead    []int32
}

// setSamplesHIP hands a data set over in the reference's own form (Dataset.Users / Items / Target, model/ctr/data.go:152-267):
// the users' encoded rows and per sample (user row, catalogue row, target).  The item side is the catalogue of setItemsHIP,
// which must be resident; sample i is the row BatchPredict composes for (user[i], item[i]) and its embeddings are the
// catalogue's.  train selects gorse_fm_set_train_samples (what the next gorse_fm_epoch trains) or gorse_fm_set_test_samples
// (what gorse_fm_evaluate scores).  A set with context labels keeps the padded route (fitHIP).  ok = false when no model is
// resident or the library refuses the set (it then keeps the previous one).
func (fm *AFM) setSamplesHIP(train bool, users SampleSide, user, item []int32, target []float32) bool {
	if fm.hip == nil || fm.hip.h == nil || len(user) != len(item) || len(user) != len(target) {
		return false
	}
	nUsers, n := len(users.Indices), len(user)
	if n == 0 && train {
		return false
	}
	uptr := make([]int64, nUsers+1)
	lead := make([]int32, max(nUsers, 1))
	var idx []int32
	var val []float32
	for t := range users.Indices {
		idx = append(idx, users.Indices[t]...)
		val = append(val, users.Values[t]...)
		uptr[t+1] = int64(len(idx))
		lead[t] = users.Lead[t]
	}
	if len(idx) == 0 {
		idx, val = []int32{0}, []float32{0}
	}
	if n == 0 { // no samples: drops the resident test split
		user, item, target = []int32{0}, []int32{0}, []float32{0}
	}
	var rc C.int32_t
	if train {
		rc = C.gorse_fm_set_train_samples(fm.hip.h, C.int64_t(nUsers), (*C.int64_t)(&uptr[0]), (*C.int32_t)(&idx[0]),
			(*C.float)(&val[0]), (*C.int32_t)(&lead[0]), C.int64_t(n), (*C.int32_t)(&user[0]), (*C.int32_t)(&item[0]),
			(*C.float)(&target[0]))
	} else {
		rc = C.gorse_fm_set_test_samples(fm.hip.h, C.int64_t(nUsers), (*C.int64_t)(&uptr[0]), (*C.int32_t)(&idx[0]),
			(*C.float)(&val[0]), (*C.int32_t)(&lead[0]), C.int64_t(n), (*C.int32_t)(&user[0]), (*C.int32_t)(&item[0]),
			(*C.float)(&target[0]))
	}
	if rc != 0 {
		log.Logger().Warn("fit AFM: the sample-form set was refused, keeping the padded route",
			zap.Bool("train", train), zap.Int("samples", n), zap.String("error", C.GoString(C.gorse_hip_last_error())))
		return false
	}
	return true
}

// SetTrainSamples / SetTestSamples: a Fit in sample form calls SetRankItems once, then these two, and trains and evaluates
// with the calls fitHIP uses (gorse_fm_epoch, evaluateResidentHIP); the catalogue stays resident for RankUsers.
func (fm *AFM) SetTrainSamples(users SampleSide, user, item []int32, target []float32) bool {
	return fm.setSamplesHIP(true, users, user, item, target)
}

func (fm *AFM) SetTestSamples(users SampleSide, user, item []int32, target []float32) bool {
	return fm.setSamplesHIP(false, users, user, item, target)
}
