// torque_kernels.h -- launch interface of torque.hip (include/sfl.h "TORQUE"): the moment of pressure and friction on the
// solid bodies of batch members and of a whole-domain context.  Only torque.cpp and torque.hip include this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"

namespace sfl {

// One sample of a batch: the `bodies` records of members [first, first + count) into out, member-major.  One workgroup
// per member.  p: the pressure, v: the velocity (x, y) per cell, both member-major.  codes / labels: the bytes of member m
// start at m * code_stride / m * label_stride (0: shared by all members; the two independently); labels null: every solid
// cell is body 1.  pivot2: (x2, y2) per body, those of member m at m * pivot_stride int32 (0: shared); null: every pivot (0, 0).
struct BatchTorqueSample {
    const float *p;
    const float2 *v;
    const uint8_t *codes, *labels;
    const int32_t *pivot2;
    size_t code_stride, label_stride, pivot_stride;
    int dim_x, dim_y, first, count, bodies;
    struct sfl_body_torque *out;
};
hipError_t launch_batch_torque(hipStream_t s, const BatchTorqueSample &a);

// One sample of a whole-domain context: `bodies` records into out -- zeroed on the stream in front, then pass 1, then the
// pass of the sums.
struct ContextTorqueSample {
    const float *p;
    const float2 *v;
    const uint8_t *codes, *labels;
    const int32_t *pivot2;
    int dim_x, dim_y, bodies;
    struct sfl_body_torque *out;
};
hipError_t launch_context_torque(hipStream_t s, const ContextTorqueSample &a);

// The sample taken while no solids are set: `count` members of `bodies` records that are zero but for pivot2 (member
// first + m reads its pivots at (first + m) * pivot_stride).  It reads no field.
hipError_t launch_torque_empty(hipStream_t s, struct sfl_body_torque *out, const int32_t *pivot2, size_t pivot_stride, int first, int count, int bodies);

}  // namespace sfl
