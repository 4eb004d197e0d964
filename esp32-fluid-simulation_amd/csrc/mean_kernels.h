// mean_kernels.h -- launch interface of means.hip (include/sfl.h "AVERAGES"): one sample of the fields held added to the
// per-cell sums of a whole-domain context or of the recorded members of a batch.  Only means.cpp and means.hip include this.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"

namespace sfl {

constexpr int kMeanThreads = 256;     // threads of a workgroup
constexpr int kMeanLaneCells = 2;     // cells a lane takes: 16 bytes of velocity, 16 bytes of every plane
constexpr int kMeanMaxMemberBlocks = 65535;   // members a launch spreads over gridDim.y at most: it strides over the rest

// the cells of a member rounded up to whole lanes: every member's plane starts on 16 bytes
inline size_t mean_member_stride(size_t cells) { return (cells + kMeanLaneCells - 1) / kMeanLaneCells * kMeanLaneCells; }

// One sample: the fields of members [first, first + count) of a batch (a context: first = 0, count = 1) added to the
// planes.  v: (x, y) per cell, p: one float, dye: three words per cell, all member-major with `cells` cells from one
// member to the next, member 0 first; a group that is not in the mask may pass null.  plane[k]: plane id k (SFL_MEAN_PLANE_*)
// of the RECORDED members, member `first` in front, member_stride values of 8 bytes from one member to the next (a multiple
// of kMeanLaneCells, the plane on 16 bytes); null where the mask has no such plane.
struct MeanSample {
    const float *v, *p;
    const uint32_t *dye;
    size_t cells, member_stride;
    int first, count;
    unsigned what;
    double *plane[SFL_MEAN_PLANES];
};
hipError_t launch_mean_sample(hipStream_t s, const MeanSample &a);

}  // namespace sfl
