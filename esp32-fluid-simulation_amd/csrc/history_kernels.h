// history_kernels.h -- launch interface of the sampler behind sfl_batch_history_* (internal, as kernels.h, whose types it
// uses): one record of include/sfl.h's struct sfl_history_record per recorded member of a batch, in ONE launch of one
// workgroup per member (history.hip).  Called from history.cpp alone.  The launcher is asynchronous on the given stream
// and returns the hipError_t of the launch.  (A context's sample is the streaming passes of stats_kernels.h and
// until_kernels.h pointed at the record: a context may hold 2^28 cells, a member at most 20224.)
#pragma once
#include "../../include/sfl.h"
#include "batch.h"

namespace sfl {

// threads of a workgroup: of members of more than kSmallGridMaxCells cells, and of smaller ones (stated for the tests:
// shapes with fewer cells than threads)
constexpr int kHistoryThreads = 1024;
constexpr int kHistoryThreadsSmall = 256;

// What one sample reads.  The four fields are member 0's, member-major as a batch stores them; the kernel forms each
// member's base in 64-bit.  out: the record of member `first`, `count` records back to back.
struct HistorySample {
    const float *vel;      // the velocity the step left (projected)
    const uint32_t *dye;   // ... and its dye
    const float *p, *d;    // the pressure and the divergence of its solve
    int dim_x, dim_y;
    int first, count;      // the recorded members
    int batch;             // members of the batch: the records of `members`
    long long step;        // the history's step count at this sample
    // the step's parameters: every member's (members == nullptr), or member m's own from the record of `members` that
    // NAMES m (the records are in launch order, most iterations first); counts != nullptr: member m's iterations are
    // counts[2 m] as the step's launch left them (the *_until calls), else the record's (the call's) iters
    float dt, dx, two_dx_inv;
    int iters;
    const BatchMember *members;
    const int *counts;
    struct sfl_history_record *out;
};
// Any shape a batch of either kind holds (dim_x, dim_y >= 2, at most kLargeMemberMaxCells cells); count >= 1.
// No global atomics and nothing zeroed in front: every byte of every record is stored by its workgroup's thread 0.
// threads: 0 = chosen from the member's size (what the library passes); 256, 512 or 1024 forces that workgroup
// (tools/history_pass_probe.hip times all three); anything else returns hipErrorInvalidValue.
hipError_t launch_history_sample(hipStream_t s, const HistorySample &a, int threads = 0);

}  // namespace sfl
