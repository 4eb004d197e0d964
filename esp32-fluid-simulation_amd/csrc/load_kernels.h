// load_kernels.h -- launch interface of loads.hip (include/sfl.h "LOADS"): the pressure load on the solid bodies of batch
// members and of a whole-domain context.  Only loads.cpp and loads.hip include this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"

namespace sfl {

// One sample of a batch: the `bodies` records of members [first, first + count) into out, member-major.  One workgroup
// per member.  codes / labels: the bytes of member m start at m * code_stride / m * label_stride (0: shared by all
// members; the two independently); labels null: every solid cell is body 1.
struct BatchLoadSample {
    const float *p;
    const uint8_t *codes, *labels;
    size_t code_stride, label_stride;
    int dim_x, dim_y, first, count, bodies;
    struct sfl_body_load *out;
};
hipError_t launch_batch_loads(hipStream_t s, const BatchLoadSample &a);

// One sample of a whole-domain context: `bodies` records into out -- zeroed on the stream in front, then the pass of the
// maxima, then the pass of the sums.
struct ContextLoadSample {
    const float *p;
    const uint8_t *codes, *labels;
    int dim_x, dim_y, bodies;
    struct sfl_body_load *out;
};
hipError_t launch_context_loads(hipStream_t s, const ContextLoadSample &a);

}  // namespace sfl
