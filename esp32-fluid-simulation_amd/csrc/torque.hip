// torque.hip -- the samplers of the torque on solid bodies (gfx950 / MI355X; include/sfl.h "TORQUE"): per body the exact
// integer sums mp and mf of (doubled arm) x (truncated face term) of the pressure and of the tangential velocity, the two
// exponents they are scaled by, the two maxima, the number of faces, the longest doubled arm, the counts of faces whose
// pressure / tangential component is not finite, and the pivot.
//
// The scheme of a batch's and a context's sampler, the walks and the launchers are body_walk.h's, shared with loads.hip and
// friction.hip.  What differs: ONE walk reads BOTH fields -- the fluid cell's pressure and its velocity as a float2, once per
// cell -- and every term is multiplied by an arm about the body's pivot (torque_face.h, shared with the host driver of the
// tests).  The exponents are raised by s = max(0, L(faces) + L(max_arm2) - 30), so that a sum of `faces` products stays
// inside 64 bits: pass 1 therefore gathers faces and max_arm2 beside the two maxima, and the terms wait for all four.
// In a batch the pivots of the member go into LDS first (a workgroup-uniform address); pass 1 folds |p|, |v_t|, the longest
// arm and a count into the body's LDS words -- a maximum only where it beats the value read, so a body costs a handful of LDS
// atomics, not one per face -- and thread k forms body k's exponents between the passes.  In a context the exponents and the
// pivot are the fields that workgroup 0 stores.  There is no float arithmetic: everything happens behind the float's bits.
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): DESIGN.md 4.19; no scratch in any of the kernels.
#include "body_walk.h"
#include "torque_face.h"
#include "torque_kernels.h"

namespace sfl {
namespace {

using torque_face::Arms;

static_assert(sizeof(struct sfl_body_torque) == 64, "include/sfl.h: 64 bytes");

// what a workgroup gathers of its faces, per body
struct TorqueGathered {
    unsigned max_p[kB], max_t[kB], faces[kB], max_arm2[kB], nonfinite_p[kB], nonfinite_t[kB];
    int exp2_p[kB], exp2_f[kB], px2[kB], py2[kB];
    u64 mp[kB], mf[kB];
};

// all zero but the pivots: body k's from pivot2 (workgroup-uniform; null: (0, 0))
__device__ __forceinline__ void clear(TorqueGathered &g, const int32_t *pivot2, int bodies)
{
    if (threadIdx.x < kB) {
        const int k = threadIdx.x;
        g.max_p[k] = g.max_t[k] = g.faces[k] = g.max_arm2[k] = g.nonfinite_p[k] = g.nonfinite_t[k] = 0u;
        g.exp2_p[k] = g.exp2_f[k] = 0;
        g.mp[k] = g.mf[k] = 0ull;
        const bool set = pivot2 && k < bodies;
        g.px2[k] = set ? pivot2[2 * k] : 0;
        g.py2[k] = set ? pivot2[2 * k + 1] : 0;
    }
}

__device__ __forceinline__ void grow(unsigned *word, unsigned value)
{
    if (value > *word) atomicMax(word, value);   // (the word only grows: a stale read costs an atomic, never a maximum)
}

// pass 1: one face of fluid cell (i, j) into the body's maxima and count
__device__ __forceinline__ void see_face(TorqueGathered &g, int body, int dir, int i, int j, unsigned p_bits, unsigned t_bits)
{
    atomicAdd(&g.faces[body], 1u);
    grow(&g.max_arm2[body], torque_face::longest(torque_face::arms_of(i, j, dir, g.px2[body], g.py2[body])));
    const unsigned ap = p_bits & 0x7fffffffu, at = t_bits & 0x7fffffffu;
    if (ap < 0x7f800000u) grow(&g.max_p[body], ap);   // (not finite: no part in the maximum)
    if (at < 0x7f800000u) grow(&g.max_t[body], at);
}

// between the passes: thread k forms body k's exponents from the finished pass 1
__device__ __forceinline__ void exponents(TorqueGathered &g, int bodies)
{
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x, s = torque_face::shift_of(g.faces[k], g.max_arm2[k]);
        g.exp2_p[k] = exp2_of(g.max_p[k]) + s;
        g.exp2_f[k] = exp2_of(g.max_t[k]) + s;
    }
}

// pass 2: one face into the body's sums (two's complement: the sum of the signed products)
__device__ __forceinline__ void add_face(TorqueGathered &g, int body, int dir, int i, int j, unsigned p_bits, unsigned t_bits)
{
    const Arms arms = torque_face::arms_of(i, j, dir, g.px2[body], g.py2[body]);
    if ((p_bits & 0x7f800000u) == 0x7f800000u)
        atomicAdd(&g.nonfinite_p[body], 1u);
    else if (const long long m = torque_face::pressure_moment(arms, dir, term_of(p_bits, g.exp2_p[body])))
        atomicAdd(&g.mp[body], (u64)m);
    if ((t_bits & 0x7f800000u) == 0x7f800000u)
        atomicAdd(&g.nonfinite_t[body], 1u);
    else if (const long long m = torque_face::friction_moment(arms, dir, term_of(t_bits, g.exp2_f[body])))
        atomicAdd(&g.mf[body], (u64)m);
}

__global__ void __launch_bounds__(kT) batch_torque_kernel(const BatchTorqueSample a)
{
    __shared__ TorqueGathered g;
    const int member = a.first + (int)blockIdx.x, dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y, bodies = a.bodies;
    const float *p = a.p + (size_t)member * (size_t)cells;
    const float2 *v = a.v + (size_t)member * (size_t)cells;
    const uint8_t *codes = a.codes + (size_t)member * a.code_stride;
    const uint8_t *labels = a.labels ? a.labels + (size_t)member * a.label_stride : nullptr;
    clear(g, a.pivot2 ? a.pivot2 + (size_t)member * a.pivot_stride : nullptr, bodies);
    __syncthreads();
    // ---- pass 1: the maxima of both fields, the faces, the longest arm
    member_walk(codes, dim_x, dim_y, [&](int c, unsigned faces) {
        const unsigned p_bits = __float_as_uint(p[c]);
        const float2 u = v[c];
        const int j = c / dim_x, i = c - j * dim_x;
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) { see_face(g, body, dir, i, j, p_bits, tangential(u, dir)); });
    });
    __syncthreads();
    exponents(g, bodies);
    __syncthreads();
    // ---- pass 2: the products
    member_walk(codes, dim_x, dim_y, [&](int c, unsigned faces) {
        const unsigned p_bits = __float_as_uint(p[c]);
        const float2 u = v[c];
        const int j = c / dim_x, i = c - j * dim_x;
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) { add_face(g, body, dir, i, j, p_bits, tangential(u, dir)); });
    });
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_torque r;
        r.mp = (int64_t)g.mp[k];
        r.mf = (int64_t)g.mf[k];
        r.exp2_p = g.exp2_p[k];
        r.exp2_f = g.exp2_f[k];
        r.max_abs_p = __uint_as_float(g.max_p[k]);
        r.max_abs_t = __uint_as_float(g.max_t[k]);
        r.faces = g.faces[k];
        r.max_arm2 = g.max_arm2[k];
        r.nonfinite_p = g.nonfinite_p[k];
        r.nonfinite_t = g.nonfinite_t[k];
        r.pivot2[0] = g.px2[k];
        r.pivot2[1] = g.py2[k];
        r.reserved[0] = r.reserved[1] = 0u;
        a.out[(size_t)blockIdx.x * bodies + k] = r;
    }
}

// SUMS false: pass 1 into max_abs_p, max_abs_t, faces and max_arm2 of the zeroed records; true: everything else, from the
// finished pass 1
template <bool SUMS>
__global__ void __launch_bounds__(kT) context_torque_kernel(const ContextTorqueSample a, int cells, int groups, bool aligned)
{
    __shared__ TorqueGathered g;
    const int dim_x = a.dim_x, dim_y = a.dim_y, bodies = a.bodies;
    clear(g, a.pivot2, bodies);
    __syncthreads();
    if (SUMS) {
        if ((int)threadIdx.x < bodies) {
            const struct sfl_body_torque *r = a.out + threadIdx.x;
            const int s = torque_face::shift_of(r->faces, r->max_arm2);
            g.exp2_p[threadIdx.x] = exp2_of(__float_as_uint(r->max_abs_p)) + s;
            g.exp2_f[threadIdx.x] = exp2_of(__float_as_uint(r->max_abs_t)) + s;
        }
        __syncthreads();
    }
    context_walk(a.codes, dim_x, dim_y, cells, groups, aligned, [&](int c, unsigned faces) {
        const unsigned p_bits = __float_as_uint(a.p[c]);
        const float2 u = a.v[c];
        const int j = c / dim_x, i = c - j * dim_x;
        wet_faces(faces, c, dim_x, a.labels, bodies, [&](int body, int dir) {
            if (SUMS)
                add_face(g, body, dir, i, j, p_bits, tangential(u, dir));
            else
                see_face(g, body, dir, i, j, p_bits, tangential(u, dir));
        });
    });
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_torque *r = a.out + k;
        if (!SUMS) {
            if (g.max_p[k]) atomicMax(reinterpret_cast<unsigned *>(&r->max_abs_p), g.max_p[k]);
            if (g.max_t[k]) atomicMax(reinterpret_cast<unsigned *>(&r->max_abs_t), g.max_t[k]);
            if (g.faces[k]) atomicAdd(&r->faces, g.faces[k]);
            if (g.max_arm2[k]) atomicMax(&r->max_arm2, g.max_arm2[k]);
        } else {
            if (g.mp[k]) atomicAdd(reinterpret_cast<u64 *>(&r->mp), g.mp[k]);
            if (g.mf[k]) atomicAdd(reinterpret_cast<u64 *>(&r->mf), g.mf[k]);
            if (g.nonfinite_p[k]) atomicAdd(&r->nonfinite_p, g.nonfinite_p[k]);
            if (g.nonfinite_t[k]) atomicAdd(&r->nonfinite_t, g.nonfinite_t[k]);
            if (blockIdx.x == 0) {   // (fields no atomic touches)
                r->exp2_p = g.exp2_p[k];
                r->exp2_f = g.exp2_f[k];
                r->pivot2[0] = g.px2[k];
                r->pivot2[1] = g.py2[k];
            }
        }
    }
}

// record r of the sample without solids: zeros and the pivot of its body
__global__ void __launch_bounds__(kT) torque_empty_kernel(struct sfl_body_torque *out, const int32_t *pivot2, size_t pivot_stride, int first, int records, int bodies)
{
    const int r = blockIdx.x * kT + threadIdx.x;
    if (r >= records) return;
    const int m = r / bodies, k = r - m * bodies;
    const int32_t *pv = pivot2 ? pivot2 + (size_t)(first + m) * pivot_stride + 2 * k : nullptr;
    struct sfl_body_torque z = {};
    z.pivot2[0] = pv ? pv[0] : 0;
    z.pivot2[1] = pv ? pv[1] : 0;
    out[r] = z;
}

}  // namespace

hipError_t launch_batch_torque(hipStream_t s, const BatchTorqueSample &a) { return launch_batch(s, a, batch_torque_kernel); }

hipError_t launch_context_torque(hipStream_t s, const ContextTorqueSample &a)
{
    return launch_context(s, a, context_torque_kernel<false>, context_torque_kernel<true>);
}

hipError_t launch_torque_empty(hipStream_t s, struct sfl_body_torque *out, const int32_t *pivot2, size_t pivot_stride, int first, int count, int bodies)
{
    if (count < 1 || bodies < 1 || bodies > kB) return hipErrorInvalidValue;
    const int records = count * bodies;   // <= 2^31 / 64: the records fit a buffer
    torque_empty_kernel<<<(records + kT - 1) / kT, kT, 0, s>>>(out, pivot2, pivot_stride, first, records, bodies);
    return hipGetLastError();
}

}  // namespace sfl
