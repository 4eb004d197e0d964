// loads.hip -- the samplers of the pressure load on solid bodies (gfx950 / MI355X; include/sfl.h "LOADS"): per body the
// exact integer sums fx and fy of the truncated face terms, the exponent they are scaled by, the largest |p| on a face,
// the face counts and the count of faces with a pressure that is not finite.
//
// The scheme of a batch's and a context's sampler, the walks and the kernel bodies are body_walk.h's, shared with
// friction.hip; here is what the loads are as a kind: a face takes the pressure of its fluid cell, whatever its direction,
// into fx (the fluid cell W or E of the solid one: directions 0, 1) or fy (S or N: 2, 3), negated where the fluid cell lies
// on the positive side (1, 3).
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): DESIGN.md 4.13; no scratch in any of the three kernels.
#include "body_walk.h"
#include "load_kernels.h"

namespace sfl {
namespace {

struct LoadsKind {
    typedef struct sfl_body_load Record;
    template <class A>
    static __device__ __forceinline__ const float *field(const A &a) { return a.p; }
    static __device__ __forceinline__ unsigned bits(float p, int) { return __float_as_uint(p); }
    static __device__ __forceinline__ void sum(Gathered &g, int body, int dir, long long t)
    {
        atomicAdd(dir < 2 ? &g.fx[body] : &g.fy[body], (u64)((dir & 1) ? -t : t));
    }
    static __device__ __forceinline__ float &maximum(Record &r) { return r.max_abs_p; }
};
static_assert(sizeof(struct sfl_body_load) == 48, "include/sfl.h: 48 bytes");

__global__ void __launch_bounds__(kT) batch_loads_kernel(const BatchLoadSample a) { batch_sample<LoadsKind>(a); }

template <bool SUMS>
__global__ void __launch_bounds__(kT) context_loads_kernel(const ContextLoadSample a, int cells, int groups, bool aligned)
{
    context_sample<LoadsKind, SUMS>(a, cells, groups, aligned);
}

}  // namespace

hipError_t launch_batch_loads(hipStream_t s, const BatchLoadSample &a) { return launch_batch(s, a, batch_loads_kernel); }

hipError_t launch_context_loads(hipStream_t s, const ContextLoadSample &a)
{
    return launch_context(s, a, context_loads_kernel<false>, context_loads_kernel<true>);
}

}  // namespace sfl
