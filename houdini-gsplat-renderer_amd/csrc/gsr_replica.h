// gsr_replica.h -- whether the replicas of gsr_multi still agree after a verb that edits every rank's copy of the cloud (remove, add,
// duplicate, transform, grade).  Host only, no HIP, no context: gsr_debug_replica_verdict (gsplat_hip.h states the contract) is this
// function, and tests/test_replica_agreement.py holds it to that contract.
//
// Every rank runs the verb on its own replica and leaves K counts (the splats left, the total, ...), -1 until the verb returns GSR_OK.
// A refusal before any rank's first write leaves the replicas as they were; ranks that disagree, or a HIP failure (it may have come
// behind a rank's first write, so that the rank holds nothing any more), cost every rank its geometry: a multi-GPU frame never
// gathers bands of different clouds.
#pragma once
#include <stdint.h>
#include "../../include/gsplat_hip.h"

// -> GSR_REPLICA_KEEP_REFUSAL, _AGREED, _DROP_ALL; -1 bad argument
static inline int gsr_replica_verdict(int rc, int ranks, int per_rank, const int64_t* counts /* [ranks * per_rank] */)
{
    if (!counts || ranks < 1 || per_rank < 1) return -1;
    const int64_t total = (int64_t)ranks * per_rank;
    bool any_done = false;
    for (int64_t k = 0; k < total; ++k) any_done = any_done || counts[k] >= 0;
    if (rc != GSR_OK && rc != GSR_E_HIP && !any_done) return GSR_REPLICA_KEEP_REFUSAL;
    bool same = rc == GSR_OK;
    for (int64_t k = per_rank; k < total && same; ++k) same = counts[k] == counts[k % per_rank];
    return same ? GSR_REPLICA_AGREED : GSR_REPLICA_DROP_ALL;
}
