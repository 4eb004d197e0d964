// stats_kernels.h -- launch interface of the kernels behind sfl_flow_stats and sfl_batch_flow_stats[_each] (internal, as
// kernels.h, whose types it uses): the maxima of |v.x|, |v.y| and |calculate_divergence(v)| in one streaming pass over a
// velocity field of any size, and the exact per-channel sums of a dye field in one pass over it (flow_stats.hip).  Called
// from flow_stats.cpp (contexts) and batch.cpp (batches).  The launcher is asynchronous on the given stream and returns
// the hipError_t of its launches.
#pragma once
#include "kernels.h"

namespace sfl {

// The tiles of the velocity pass (tests/test_flow_stats.py places its spikes on both sides of their boundaries): a wave
// owns a strip of kStatsStripCols columns (64 lanes x one 16-byte load of two cells) and a chunk of rows, kStatsChunkRows
// of them on every grid that does not fill the chip several times over (16 or 32 on those: launch_flow_stats).
constexpr int kStatsStripCols = 128;
constexpr int kStatsChunkRows = 8;

// What the passes leave per member: sfl_flow_stats of include/sfl.h word for word (40 bytes), the three maxima as the
// bit patterns of |x|.
struct FlowStatsRecord {
    unsigned max_abs_vx, max_abs_vy, max_abs_div;
    unsigned what;                   // (left 0 by the device: the host fills it in)
    unsigned long long dye_sum[3];
};
static_assert(sizeof(FlowStatsRecord) == 40, "sfl_flow_stats is 40 bytes");

// out[m] (device records, zeroed here on the stream in front of the kernels) = the statistics of member m of `members`
// fields of dim_x x dim_y cells stored back to back from v / dye (a context: members = 1).  what = SFL_STATS_* bits: one
// launch per bit.  The divergence of member m is scaled by member_two_dx_inv[m] (a device array) when that is not null,
// else by two_dx_inv.  Reads only; any dim_x, dim_y >= 2 and any alignment of the fields beyond their elements' own.
hipError_t launch_flow_stats(hipStream_t s, FlowStatsRecord *out, int what, const float *v, const uint32_t *dye, int dim_x,
                             int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv);

}  // namespace sfl
