// ensemble_kernels.h -- launch interface of the kernels behind sfl_distance / sfl_batch_distance (field_distance.hip) and
// sfl_batch_envelope (batch_envelope.hip); internal, as kernels.h, whose types it uses.  Called from ensemble.cpp only.
// Every launcher is asynchronous on the given stream and returns the hipError_t of its launches.
#pragma once
#include "kernels.h"

namespace sfl {

// ---- the distance passes ----------------------------------------------------------------------------------------------
// The tiles of the passes (tests/test_ensemble_gpu.py places its differing words on both sides of their boundaries).  A
// lane holds WHOLE cells: one vector load of kDist*LaneCells cells per operand -- 16 bytes of velocity or pressure, the
// 12 bytes of one dye cell -- each load of the wave contiguous; a workgroup of kDistThreads lanes issues kDistItemLoads
// such loads per lane and operand for one ITEM, the unit in which a member's cells are dealt to the workgroups.  The
// cells behind a member's last whole lane (cells modulo kDist*LaneCells) are read one at a time.
constexpr int kDistThreads = 256;
constexpr int kDistItemLoads = 8;
constexpr int kDistVelocityLaneCells = 2;
constexpr int kDistPressureLaneCells = 4;
constexpr int kDistDyeLaneCells = 1;

// What the passes leave per record: sfl_field_distance of include/sfl.h word for word (64 bytes), the float maxima as
// the bit patterns of |a - b|.
struct DistanceRecord {
    unsigned max_abs_dvx, max_abs_dvy, max_abs_dp;
    unsigned what;   // (left 0 by the device: the host fills it in)
    unsigned velocity_cells_differ, dye_cells_differ, pressure_cells_differ;
    unsigned max_abs_ddye[3];
    unsigned long long sum_abs_ddye[3];
};
static_assert(sizeof(DistanceRecord) == 64, "sfl_field_distance is 64 bytes");

// One side of a distance: the three fields of its FIRST member and the distance from one member to the next in CELLS
// (a batch: dim_x * dim_y; 0: every record is taken against the same member; a context: anything).
struct DistanceSide {
    const float *v;
    const uint32_t *dye;
    const float *p;
    size_t member_cells;
};
// out[k] (device records, zeroed here on the stream in front of the kernels), k in [0, members) = the distance of the
// `cells` cells at a's member k from those at b's member k.  what = SFL_DIST_* bits: one launch per bit; the fields of
// the bits not asked for are not touched and may be null.  Reads only; any cells >= 1 and any alignment of the members
// beyond their elements' own.
hipError_t launch_field_distance(hipStream_t s, DistanceRecord *out, int what, const DistanceSide &a, const DistanceSide &b,
                                 size_t cells, int members);

// ---- the envelope of the dye ------------------------------------------------------------------------------------------
// The members are split into GROUPS of kEnvGroupMembers; a workgroup owns kEnvBlockWords words (one per thread) of one
// group and leaves their partial minimum, maximum and 64-bit sum; a second launch combines the groups' partials, in
// group order and with plain stores, into the four fields.
constexpr int kEnvBlockWords = 256;
constexpr int kEnvGroupMembers = 32;
inline int envelope_groups(int count) { return (count + kEnvGroupMembers - 1) / kEnvGroupMembers; }
// words of uint32 the partials of `count` members of `member_words` words take (sums first: 8-byte aligned)
inline size_t envelope_partial_words(int count, size_t member_words) { return (size_t)envelope_groups(count) * member_words * 4; }

// fields[which * member_words + w], which = SFL_ENV_*, w in [0, member_words) = the mean (floor of the 64-bit sum over
// count), minimum, maximum and maximum - minimum of word w over the `count` members stored member_words apart from
// `dye`.  partials: envelope_partial_words(count, member_words) words, 8-byte aligned, scratch.  count >= 1; member bases
// are formed in 64-bit, member_words <= 2^31 - 1.  Reads the members only; any alignment of theirs.
hipError_t launch_batch_envelope(hipStream_t s, uint32_t *fields, uint32_t *partials, const uint32_t *dye, size_t member_words,
                                 int count);

}  // namespace sfl
