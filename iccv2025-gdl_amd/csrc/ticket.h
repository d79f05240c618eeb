// ticket.h -- "the last block folds": every block of a launch publishes its terms, draws a ticket, and the block that draws the
// last one adds all terms in ONE fixed order.  No floating-point atomic; the result does not depend on which block comes last.
//
// Visibility between the blocks (per-XCD L2s are not coherent): a term is an agent-scope (write-through) store, st_agent, waited
// for (s_waitcnt vmcnt(0)) by the lane that issued it before the ticket's agent-scope acq_rel add -- by the drawing lane itself,
// or by another lane that waits and then meets the drawing lane at a block barrier; the reader's loads are agent-scope loads
// (ld_agent) issued after its add has returned.  The counter belongs to one stream (or one caller's workspace): launches of one
// stream are ordered, the last block hands the counter back at zero, so it is 0 at every kernel start.
#pragma once
#include "common.h"

namespace gdl {

__device__ __forceinline__ void ticket_wait_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ONE lane per block, after the agent-scope stores of the block's terms (see above): true for the last of `total` tickets
__device__ __forceinline__ bool ticket_draw(unsigned* cnt, int total) {
    ticket_wait_stores();
    return __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(total - 1);
}
// the last block, when it has read the terms: the counter is 0 for the next launch
__device__ __forceinline__ void ticket_hand_back(unsigned* cnt) { __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The sum of part[0 .. count) on one wave of the last block, returned in every lane.  The order is softmax_ce_block's (head.hip):
// 256 partial sums p[b & 255] taking b, b + 256, ... in turn, then the tree p[i] += p[i + o], o = 128 .. 1 -- lane l holds
// p[l], p[l + 64], p[l + 128], p[l + 192], folds them as the tree's first two levels do, and the xor butterfly 32 .. 1 is the
// rest of the tree.
__device__ __forceinline__ float ticket_fold256(const float* part, int count, int lane) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = lane; i0 < count; i0 += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i0 + 64 * q < count) a[q] += ld_agent(part + i0 + 64 * q);
    float t = (a[0] + a[2]) + (a[1] + a[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    return t;
}

}  // namespace gdl
