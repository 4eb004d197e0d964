// tracers.hip -- the kernels behind sfl_tracers_* / sfl_batch_tracers_* (tracer_kernels.h; include/sfl.h "TRACERS"): the
// tracers of a context, or of every member of a batch, advanced by the velocity at their own positions or sampling one
// field there, one thread per tracer, in one launch.
//
// A tracer is sample() (advect.h:24-72) applied at a stored position instead of at a back-traced cell centre, so the
// arithmetic is the one the advection kernels use: classify + sample_global_vec2f / sample_global_uq3 of advect_math.h
// for the velocity and the dye, and the public header's own sample<float> (include/sfl/advect.h, usable on the device)
// for the two scalar fields, which no kernel of the step samples.  Each tracer gathers its four texels straight from
// memory (an 8-byte load per velocity texel); positions are read and written as float2.  No atomics, no LDS.  The member
// of a workgroup is blockIdx.y: its record, base offset and dt are uniform over the workgroup.
//
// Compiled with -ffp-contract=off (bit-exactness contract, see stencil_kernels.hip): u * dt is rounded, then added.
#include "../../include/sfl.h"
#include "../../include/sfl/advect.h"
#include "advect_math.h"
#include "tracer_kernels.h"

#include <algorithm>

namespace sfl {
namespace {

using namespace advect_math;

__device__ __forceinline__ bool has_nan(float2 pos) { return __builtin_isnan(pos.x) || __builtin_isnan(pos.y); }

__global__ void __launch_bounds__(kTracerThreads)
tracer_advance_kernel(float2 *__restrict__ xy, const float2 *__restrict__ velocity, const BatchMember *__restrict__ records,
                      float dt, float2 *__restrict__ trail, unsigned count, int dim_x, int dim_y, size_t member_cells)
{
    size_t member = blockIdx.y;
    if (records) {   // (uniform over the workgroup: scalar loads)
        const BatchMember r = records[blockIdx.y];
        member = (size_t)r.member;
        dt = r.dt;
    }
    const unsigned k = blockIdx.x * kTracerThreads + threadIdx.x;
    if (k >= count) return;
    const size_t at = member * count + k;
    float2 pos = xy[at];
    if (!has_nan(pos)) {   // (side_of(NaN) says "inside" and the conversion to an index is undefined: never sampled)
        const Slab g{dim_x, dim_y, 0, dim_y};
        const SrcPos s = classify(pos.x, pos.y, dim_x, dim_y);
        const float2 u = sample_global_vec2f<true>(velocity + member * member_cells, g, s, pos.x, pos.y);   // ino:253
        const float step_x = u.x * dt, step_y = u.y * dt;
        pos.x = pos.x + step_x;
        pos.y = pos.y + step_y;
        xy[at] = pos;
    }
    if (trail) trail[at] = pos;
}

template <int FIELD, bool NO_SLIP>
__global__ void __launch_bounds__(kTracerThreads)
tracer_sample_kernel(const float2 *__restrict__ xy, const void *__restrict__ field, void *__restrict__ out, unsigned count, int dim_x,
                     int dim_y, size_t member_cells)
{
    const size_t member = blockIdx.y;
    const unsigned k = blockIdx.x * kTracerThreads + threadIdx.x;
    if (k >= count) return;
    const size_t at = member * count + k, cell0 = member * member_cells;
    const float2 pos = xy[at];
    const bool skip = has_nan(pos);
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float nan = __builtin_nanf("");
    if (FIELD == SFL_FIELD_VELOCITY) {
        float2 r = make_float2(nan, nan);
        if (!skip) {
            const SrcPos s = classify(pos.x, pos.y, dim_x, dim_y);
            r = sample_global_vec2f<NO_SLIP>(static_cast<const float2 *>(field) + cell0, g, s, pos.x, pos.y);
        }
        static_cast<float2 *>(out)[at] = r;
    } else if (FIELD == SFL_FIELD_COLOR) {
        uq3 r = {0u, 0u, 0u};
        if (!skip) {
            const SrcPos s = classify(pos.x, pos.y, dim_x, dim_y);
            r = sample_global_uq3<NO_SLIP>(static_cast<const uint32_t *>(field) + 3 * cell0, g, s, pos.x, pos.y);
        }
        store_uq3(static_cast<uint32_t *>(out), at, r);
    } else {   // divergence, pressure: the header's sample<float>
        float r = nan;
        if (!skip) r = sample(const_cast<float *>(static_cast<const float *>(field)) + cell0, pos.x, pos.y, dim_x, dim_y, NO_SLIP);
        static_cast<float *>(out)[at] = r;
    }
}

constexpr int kMaxGridY = 65535;

dim3 grid_of(const TracerGrid &g, int members) { return dim3((g.count + kTracerThreads - 1) / kTracerThreads, (unsigned)members, 1); }

template <int FIELD>
hipError_t launch_sample(hipStream_t s, const TracerGrid &g, const void *field, size_t elem_bytes, bool no_slip, void *out)
{
    // (grid.y holds 65535 members: a larger batch takes one launch per 65535)
    for (int first = 0; first < g.members; first += kMaxGridY) {
        const int members = std::min(kMaxGridY, g.members - first);
        const float2 *xy = reinterpret_cast<const float2 *>(g.xy) + (size_t)first * g.count;
        const void *f = static_cast<const char *>(field) + (size_t)first * g.member_cells * elem_bytes;
        void *o = static_cast<char *>(out) + (size_t)first * g.count * elem_bytes;
        with_bool(no_slip, [&](auto ns) {
            tracer_sample_kernel<FIELD, decltype(ns)::value>
                <<<grid_of(g, members), kTracerThreads, 0, s>>>(xy, f, o, g.count, g.dim_x, g.dim_y, g.member_cells);
        });
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tracer_advance(hipStream_t s, const TracerGrid &g, const float *velocity, const BatchMember *records, float dt,
                                 float *trail)
{
    if (g.count == 0 || g.members < 1) return hipSuccess;
    // (grid.y holds 65535 members: a larger batch takes one launch per 65535.  With records, workgroup (., k) of a launch
    // runs record first + k, whichever member that names; without, member first + k)
    for (int first = 0; first < g.members; first += kMaxGridY) {
        const int members = std::min(kMaxGridY, g.members - first);
        const size_t skip = records ? 0 : (size_t)first * g.count;
        tracer_advance_kernel<<<grid_of(g, members), kTracerThreads, 0, s>>>(
            reinterpret_cast<float2 *>(g.xy) + skip, reinterpret_cast<const float2 *>(velocity) + (records ? 0 : (size_t)first * g.member_cells),
            records ? records + first : nullptr, dt, trail ? reinterpret_cast<float2 *>(trail) + skip : nullptr, g.count, g.dim_x, g.dim_y,
            g.member_cells);
    }
    return hipGetLastError();
}

hipError_t launch_tracer_sample(hipStream_t s, const TracerGrid &g, int field, const void *field_of_first_member, bool no_slip,
                                void *out)
{
    if (g.count == 0 || g.members < 1) return hipSuccess;
    switch (field) {
        case SFL_FIELD_VELOCITY: return launch_sample<SFL_FIELD_VELOCITY>(s, g, field_of_first_member, 8, no_slip, out);
        case SFL_FIELD_COLOR: return launch_sample<SFL_FIELD_COLOR>(s, g, field_of_first_member, 12, no_slip, out);
        case SFL_FIELD_DIVERGENCE: return launch_sample<SFL_FIELD_DIVERGENCE>(s, g, field_of_first_member, 4, no_slip, out);
        case SFL_FIELD_PRESSURE: return launch_sample<SFL_FIELD_PRESSURE>(s, g, field_of_first_member, 4, no_slip, out);
    }
    return hipErrorInvalidValue;
}

}  // namespace sfl
