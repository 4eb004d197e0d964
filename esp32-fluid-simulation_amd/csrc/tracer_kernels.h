// tracer_kernels.h -- launch interface of the kernels behind sfl_tracers_* / sfl_batch_tracers_* (tracers.hip); internal,
// as kernels.h, whose types it uses, and batch.h, whose member records it reads.  Called from tracers.cpp only.  Every
// launcher is asynchronous on the given stream and returns the hipError_t of its launch.
#pragma once
#include "batch.h"

namespace sfl {

// One thread per tracer in blocks of kTracerThreads; a batch: a grid of (ceil(count / kTracerThreads), members), so the
// member is uniform over a workgroup and its base offset, dt and shape are scalar values.
constexpr int kTracerThreads = 256;

// The tracers of a context (members == 1) or of every member of a batch, and the field they read.
struct TracerGrid {
    float *xy;             // positions, member-major: member m's tracer k at float 2 * (m * count + k); 8-byte aligned
    unsigned count;        // tracers per member, >= 1 and <= 2^31 - 1
    int members;           // >= 1 and <= 65535 (the launch's grid.y)
    int dim_x, dim_y;      // the shape of one member
    size_t member_cells;   // cells from one member of the field to the next (bases are formed in 64-bit)
};

// Every tracer advanced by its member's dt on `velocity` (member 0's first cell; 8-byte aligned): the rule of
// include/sfl.h ("ADVANCE"), a tracer with a NaN coordinate left as it is.  records == nullptr: every member moves by
// `dt`; else workgroups (., k) move member records[k].member by records[k].dt -- the device records of a *_each or *_until
// step launch, which hold every member exactly once.  trail != nullptr: the new positions (of a tracer that is left as it
// is: the old ones) are also written there, laid out as xy.
hipError_t launch_tracer_advance(hipStream_t s, const TracerGrid &g, const float *velocity, const BatchMember *records, float dt,
                                 float *trail);

// out[m * count + k] = sample<T>(field of member m, x, y, dim_x, dim_y, no_slip) at member m's tracer k, T by `field`
// (SFL_FIELD_* of include/sfl.h): Vector2<float> (8 bytes), Vector3<UQ32> (12), float (4, divergence and pressure).  A
// tracer with a NaN coordinate: NaN in every float, 0 in every dye channel.  Reads the positions and the field only.
hipError_t launch_tracer_sample(hipStream_t s, const TracerGrid &g, int field, const void *field_of_first_member, bool no_slip,
                                void *out);

}  // namespace sfl
