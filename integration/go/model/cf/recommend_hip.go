//go:build cgo && hip

// RecommendUnseen: every user's n best unseen items from the device-resident model with ONE call (gorse_mf_recommend) instead of
// the per-user loop of worker/pipeline.go:403-448.  The result of a user is the prefix of length n (= CacheSize) of the list that
// loop builds: the reference keeps every non-excluded item among its CacheSize + |excludeSet| neighbours, up to |excludeSet| more.
package cf

/*
#cgo LDFLAGS: -lgorse_hip
#include "gorse_hip.h"
*/
import "C"

import (
	"unsafe"

	"github.com/pkg/errors"
)

// Recommended is one entry of a user's list.
type Recommended struct {
	Item  int32
	Score float32
}

// RecommendUnseen ranks for users[t] (an index of the model's user dictionary; negative = not predictable, empty list) the items
// that itemOk admits (nil: the items with training feedback = IsItemPredictable) and that are neither in the user's training row
// held by the handle nor in seen[t] (nil: no such rows).  numItems = the model's item count: the library reads that many itemOk
// flags, and every seen index must lie below it (the library answers GORSE_ERR_RANGE otherwise).
func (m *hipModel) RecommendUnseen(users []int32, n int, seen [][]int32, itemOk []bool, numItems int) ([][]Recommended, error) {
	if n <= 0 {
		return nil, errors.Errorf("RecommendUnseen: n = %d must be positive", n)
	}
	if itemOk != nil && len(itemOk) != numItems {
		return nil, errors.Errorf("RecommendUnseen: %d itemOk flags for %d items", len(itemOk), numItems)
	}
	if seen != nil && len(seen) != len(users) {
		return nil, errors.Errorf("RecommendUnseen: %d seen lists for %d users", len(seen), len(users))
	}
	out := make([][]Recommended, len(users))
	if len(users) == 0 {
		return out, nil
	}
	var okPtr *C.uint8_t
	if len(itemOk) > 0 {
		ok := make([]uint8, len(itemOk))
		for i, b := range itemOk {
			if b {
				ok[i] = 1
			}
		}
		okPtr = (*C.uint8_t)(unsafe.Pointer(&ok[0]))
	}
	var seenPtr *C.int64_t
	var seenIdx *C.int32_t
	if seen != nil {
		indptr, indices := flatten(seen)
		seenPtr = (*C.int64_t)(unsafe.Pointer(&indptr[0]))
		seenIdx = (*C.int32_t)(unsafe.Pointer(&indices[0]))
	}
	items := make([]int32, len(users)*n)
	scores := make([]float32, len(users)*n)
	counts := make([]int32, len(users))
	rc := C.gorse_mf_recommend(m.h, C.int64_t(len(users)), (*C.int32_t)(unsafe.Pointer(&users[0])), C.int32_t(n), okPtr, seenPtr, seenIdx,
		(*C.int32_t)(unsafe.Pointer(&items[0])), (*C.float)(unsafe.Pointer(&scores[0])), (*C.int32_t)(unsafe.Pointer(&counts[0])))
	if rc != C.GORSE_OK {
		return nil, hipError("gorse_mf_recommend", rc)
	}
	for t := range users {
		out[t] = make([]Recommended, counts[t])
		for r := range out[t] {
			out[t][r] = Recommended{Item: items[t*n+r], Score: scores[t*n+r]}
		}
	}
	return out, nil
}
