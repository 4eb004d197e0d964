// friction.hip -- the samplers of the skin friction on solid bodies (gfx950 / MI355X; include/sfl.h "FRICTION"): per body the
// exact integer sums fx and fy of the truncated face terms, the exponent they are scaled by, the largest |tangential
// velocity| on a face, the face counts and the count of faces whose tangential component is not finite.
//
// The geometry is that of loads.hip, and the walk over the wet faces and the quantisation are the same code (body_walk.h).
// What differs is the face's value: the fluid cell's velocity is read ONCE as a float2, and a face with the fluid cell W or
// E of the solid one (directions 0, 1) takes .y into fy, one with the fluid cell S or N of it (2, 3) takes .x into fx, with
// its plain sign.  A cell with faces of both kinds may be finite in one component and not in the other: finiteness is a
// matter of the face, not of the cell.
//
//   A batch     one workgroup per member, launched behind the step whose velocity it reads.  Pass 1: every thread keeps
//               the maximum of the bit patterns of |v_t| per body in registers (sixteen words, indexed at compile time), the
//               wave reduces the bodies in use by __shfl_xor and its lane 0 folds them into LDS.  Barrier.  Pass 2: the
//               same walk; every face's term goes into the body's 64-bit LDS accumulator and counters.  Barrier.  Thread k
//               stores the record of body k + 1 with ordinary stores: no global atomics, no memset in front.
//   A context   a streaming pass over the code bytes taken as ONE flat array in groups of 16 (one 16-byte load; the last,
//               partial group -- and every group if the array is not aligned -- by byte loads), skipping a word whose
//               bytes are all 0 or all 0x1F.  Two launches behind a memset of the records: the maxima, then the sums, which
//               read the finished maxima.  Each folds its faces into LDS words per body and issues at most one integer
//               atomic per workgroup and touched field of a body; exp2 is stored by workgroup 0.
// Integer sums, maxima of bit patterns and counts do not depend on the order of reduction: the two samplers write the same
// bytes for the same shape, mask, labels and velocity.
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): DESIGN.md 4.17; no scratch in any of the three kernels.
#include <algorithm>

#include "body_walk.h"
#include "friction_kernels.h"

namespace sfl {
namespace {

constexpr int kT = kFrictionThreads;
static_assert(sizeof(struct sfl_body_friction) == 48 && kT >= kB && kT % 64 == 0, "include/sfl.h: 48 bytes; a thread per body");

// the bits of the tangential component of a face in direction dir
__device__ __forceinline__ unsigned tangential(float2 v, int dir) { return __float_as_uint(dir < 2 ? v.y : v.x); }

// one face into the body's sums (g.max_bits holds the finished maxima)
__device__ __forceinline__ void add_face(Gathered &g, int body, int dir, unsigned bits)
{
    atomicAdd(&g.faces[body][dir], 1u);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        atomicAdd(&g.nonfinite[body], 1u);
        return;
    }
    const long long t = term_of(bits, exp2_of(g.max_bits[body]));
    atomicAdd(dir < 2 ? &g.fy[body] : &g.fx[body], (u64)t);   // (two's complement: the sum of the signed terms)
}

__global__ void __launch_bounds__(kT) batch_friction_kernel(const BatchFrictionSample a)
{
    __shared__ Gathered g;
    const int member = a.first + (int)blockIdx.x, dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y, bodies = a.bodies;
    const float2 *v = a.v + (size_t)member * (size_t)cells;
    const uint8_t *codes = a.codes + (size_t)member * a.code_stride;
    const uint8_t *labels = a.labels ? a.labels + (size_t)member * a.label_stride : nullptr;
    clear(g);
    __syncthreads();
    // ---- pass 1: the maxima, per thread in registers
    unsigned m[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) m[k] = 0u;
    for (int c = threadIdx.x; c < cells; c += kT) {
        const unsigned code = codes[c];
        if (!wet_candidate(code)) continue;
        const unsigned faces = face_bits(code, c, dim_x, dim_y);
        if (!faces) continue;   // (the rim alone: no load of v)
        const float2 u = v[c];
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) {
            const unsigned bits = tangential(u, dir) & 0x7fffffffu;   // |v_t|
            if (bits >= 0x7f800000u) return;                           // (not finite: no part in the maximum)
#pragma unroll
            for (int k = 0; k < kB; ++k) m[k] = (k == body && bits > m[k]) ? bits : m[k];
        });
    }
#pragma unroll
    for (int k = 0; k < kB; ++k)
        if (k < bodies) {   // (uniform)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned t = __shfl_xor(m[k], o);
                m[k] = t > m[k] ? t : m[k];
            }
            if ((threadIdx.x & 63) == 0 && m[k]) atomicMax(&g.max_bits[k], m[k]);
        }
    __syncthreads();
    // ---- pass 2: the terms, the face counts
    for (int c = threadIdx.x; c < cells; c += kT) {
        const unsigned code = codes[c];
        if (!wet_candidate(code)) continue;
        const unsigned faces = face_bits(code, c, dim_x, dim_y);
        if (!faces) continue;
        const float2 u = v[c];
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) { add_face(g, body, dir, tangential(u, dir)); });
    }
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_friction r;
        r.fx = (int64_t)g.fx[k];
        r.fy = (int64_t)g.fy[k];
        r.exp2 = exp2_of(g.max_bits[k]);
        r.max_abs_t = __uint_as_float(g.max_bits[k]);
#pragma unroll
        for (int d = 0; d < 4; ++d) r.faces[d] = g.faces[k][d];
        r.nonfinite = g.nonfinite[k];
        r.reserved = 0u;
        a.out[(size_t)blockIdx.x * bodies + k] = r;
    }
}

// SUMS false: the maxima into max_abs_t of the zeroed records; true: everything else, from the finished maxima
template <bool SUMS>
__global__ void __launch_bounds__(kT) context_friction_kernel(const ContextFrictionSample a, int cells, int groups, bool aligned)
{
    __shared__ Gathered g;
    const int dim_x = a.dim_x, dim_y = a.dim_y, bodies = a.bodies;
    clear(g);
    __syncthreads();
    if (SUMS) {
        if ((int)threadIdx.x < bodies) g.max_bits[threadIdx.x] = __float_as_uint(a.out[threadIdx.x].max_abs_t);
        __syncthreads();
    }
    const auto cell = [&](int c, unsigned code) {
        const unsigned faces = face_bits(code, c, dim_x, dim_y);
        if (!faces) return;   // (the rim alone: no load of v)
        const float2 u = a.v[c];
        wet_faces(faces, c, dim_x, a.labels, bodies, [&](int body, int dir) {
            const unsigned bits = tangential(u, dir);
            if (SUMS)
                add_face(g, body, dir, bits);
            else if ((bits & 0x7f800000u) != 0x7f800000u)
                atomicMax(&g.max_bits[body], bits & 0x7fffffffu);
        });
    };
    for (int grp = blockIdx.x * kT + threadIdx.x; grp < groups; grp += gridDim.x * kT) {
        const int base = grp * kFrictionGroupCells;   // < 2^28
        if (aligned && base + kFrictionGroupCells <= cells) {
            const uint4 w = *reinterpret_cast<const uint4 *>(a.codes + base);
            const unsigned words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (words[k] == 0u || words[k] == 0x1f1f1f1fu) continue;   // four solid cells, or four with every neighbour present
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned code = (words[k] >> (8 * q)) & 0xffu;
                    if (wet_candidate(code)) cell(base + 4 * k + q, code);
                }
            }
        } else {
            const int end = min(base + kFrictionGroupCells, cells);
            for (int c = base; c < end; ++c) {
                const unsigned code = a.codes[c];
                if (wet_candidate(code)) cell(c, code);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_friction *r = a.out + k;
        if (!SUMS) {
            if (g.max_bits[k]) atomicMax(reinterpret_cast<unsigned *>(&r->max_abs_t), g.max_bits[k]);
        } else {
            if (g.fx[k]) atomicAdd(reinterpret_cast<u64 *>(&r->fx), g.fx[k]);
            if (g.fy[k]) atomicAdd(reinterpret_cast<u64 *>(&r->fy), g.fy[k]);
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (g.faces[k][d]) atomicAdd(&r->faces[d], g.faces[k][d]);
            if (g.nonfinite[k]) atomicAdd(&r->nonfinite, g.nonfinite[k]);
            if (blockIdx.x == 0) r->exp2 = exp2_of(g.max_bits[k]);   // (a field no atomic touches)
        }
    }
}

}  // namespace

hipError_t launch_batch_friction(hipStream_t s, const BatchFrictionSample &a)
{
    if (a.count < 1 || a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    batch_friction_kernel<<<a.count, kT, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_context_friction(hipStream_t s, const ContextFrictionSample &a)
{
    if (a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.out, 0, (size_t)a.bodies * sizeof(struct sfl_body_friction), s);
    if (e != hipSuccess) return e;
    const long long cells = (long long)a.dim_x * a.dim_y;   // <= 2^28
    const int groups = (int)((cells + kFrictionGroupCells - 1) / kFrictionGroupCells);
    const int blocks = std::min((groups + kT - 1) / kT, kFrictionMaxBlocks);
    const bool aligned = reinterpret_cast<uintptr_t>(a.codes) % 16 == 0;
    context_friction_kernel<false><<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    context_friction_kernel<true><<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    return hipGetLastError();
}

}  // namespace sfl
