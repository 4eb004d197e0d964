// friction_kernels.h -- launch interface of friction.hip (include/sfl.h "FRICTION"): the skin friction on the solid bodies
// of batch members and of a whole-domain context.  Only friction.cpp and friction.hip include this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"

namespace sfl {

// One sample of a batch: the `bodies` records of members [first, first + count) into out, member-major.  One workgroup
// per member.  v: the velocity, (x, y) per cell, member-major.  codes / labels: the bytes of member m start at
// m * code_stride / m * label_stride (0: shared by all members; the two independently); labels null: every solid cell is
// body 1.
struct BatchFrictionSample {
    const float2 *v;
    const uint8_t *codes, *labels;
    size_t code_stride, label_stride;
    int dim_x, dim_y, first, count, bodies;
    struct sfl_body_friction *out;
};
hipError_t launch_batch_friction(hipStream_t s, const BatchFrictionSample &a);

// One sample of a whole-domain context: `bodies` records into out -- zeroed on the stream in front, then the pass of the
// maxima, then the pass of the sums.
struct ContextFrictionSample {
    const float2 *v;
    const uint8_t *codes, *labels;
    int dim_x, dim_y, bodies;
    struct sfl_body_friction *out;
};
hipError_t launch_context_friction(hipStream_t s, const ContextFrictionSample &a);

}  // namespace sfl
