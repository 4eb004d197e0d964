// friction.hip -- the samplers of the skin friction on solid bodies (gfx950 / MI355X; include/sfl.h "FRICTION"): per body the
// exact integer sums fx and fy of the truncated face terms, the exponent they are scaled by, the largest |tangential
// velocity| on a face, the face counts and the count of faces whose tangential component is not finite.
//
// The scheme of a batch's and a context's sampler, the walks and the kernel bodies are body_walk.h's, shared with loads.hip;
// here is what the friction is as a kind: the fluid cell's velocity is read ONCE as a float2, and a face with the fluid
// cell W or E of the solid one (directions 0, 1) takes .y into fy, one with the fluid cell S or N of it (2, 3) takes .x into
// fx, with its plain sign.  A cell with faces of both kinds may be finite in one component and not in the other: finiteness
// is a matter of the face, not of the cell.
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): DESIGN.md 4.17; no scratch in any of the three kernels.
#include "body_walk.h"
#include "friction_kernels.h"

namespace sfl {
namespace {

struct FrictionKind {
    typedef struct sfl_body_friction Record;
    template <class A>
    static __device__ __forceinline__ const float2 *field(const A &a) { return a.v; }
    static __device__ __forceinline__ unsigned bits(float2 v, int dir) { return tangential(v, dir); }
    static __device__ __forceinline__ void sum(Gathered &g, int body, int dir, long long t) { atomicAdd(dir < 2 ? &g.fy[body] : &g.fx[body], (u64)t); }
    static __device__ __forceinline__ float &maximum(Record &r) { return r.max_abs_t; }
};
static_assert(sizeof(struct sfl_body_friction) == 48, "include/sfl.h: 48 bytes");

__global__ void __launch_bounds__(kT) batch_friction_kernel(const BatchFrictionSample a) { batch_sample<FrictionKind>(a); }

template <bool SUMS>
__global__ void __launch_bounds__(kT) context_friction_kernel(const ContextFrictionSample a, int cells, int groups, bool aligned)
{
    context_sample<FrictionKind, SUMS>(a, cells, groups, aligned);
}

}  // namespace

hipError_t launch_batch_friction(hipStream_t s, const BatchFrictionSample &a) { return launch_batch(s, a, batch_friction_kernel); }

hipError_t launch_context_friction(hipStream_t s, const ContextFrictionSample &a)
{
    return launch_context(s, a, context_friction_kernel<false>, context_friction_kernel<true>);
}

}  // namespace sfl
