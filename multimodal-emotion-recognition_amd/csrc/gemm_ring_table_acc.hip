// accumulate form of the ring table launch (gemm_ring_table.hip; m2f_plan_accumulate_grads): ring_epilogue EPI 5 - every dW element and
// bias-gradient row leaves as old + new, one rounded fp32 add of the value the overwrite form stores.  A translation unit of its own: next
// to the overwrite form's instantiation in one unit, hipcc's host pass failed to resolve the producer role of the second kernel.
#include "gemm_ring.h"
hipError_t m2f_ring_launch_table_rc_256x128_acc(const GemmBatch& gb, hipStream_t stream) {
    return launch_ring_grid<256, 128, 3, true, 5>(gb, gb.total_tiles, stream);
}
