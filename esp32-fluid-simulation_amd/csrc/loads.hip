// loads.hip -- the samplers of the pressure load on solid bodies (gfx950 / MI355X; include/sfl.h "LOADS"): per body the
// exact integer sums fx and fy of the truncated face terms, the exponent they are scaled by, the largest |p| on a face,
// the face counts and the count of faces with a pressure that is not finite.
//
// Both samplers read the code bytes of the solids (solids.cpp solid_codes: bit 0 W, 1 E, 2 S, 3 N neighbour present, bit
// 4 the cell is fluid): a fluid cell with an absent neighbour that is INSIDE THE DOMAIN -- derived from the cell's
// coordinates, not from the byte -- has a solid cell there, whose label (1 without labels) names the body of that wet face.
//
//   A batch     one workgroup per member, launched behind the step whose pressure it reads.  Pass 1: every thread keeps
//               the maximum of the bit patterns of |p| per body in registers (sixteen words, indexed at compile time), the
//               wave reduces the bodies in use by __shfl_xor and its lane 0 folds them into LDS.  Barrier.  Pass 2: the
//               same walk; every face's term goes into the body's 64-bit LDS accumulator and counters.  Barrier.  Thread k
//               stores the record of body k + 1 with ordinary stores: no global atomics, no memset in front.
//   A context   a streaming pass over the code bytes taken as ONE flat array: a thread takes 16 cells with one 16-byte load
//               (the array starts 16-byte aligned, so every group does whatever the width; the cells of the last, partial
//               group -- and every group if the array is not aligned -- come by byte loads) and skips a word whose bytes are
//               all 0 or all 0x1F: nothing wet, which is nearly all of a large grid.  Only a fluid cell with an absent
//               neighbour divides its index into (i, j); only one with a face reads p and its solid neighbours' labels (a
//               cell that merely touches the rim reads neither).  Two launches: the
//               maxima, then the sums, which read the finished maxima.  Each folds its faces into LDS words per body and
//               issues at most one integer atomic per workgroup and touched field of a body, on records the launcher
//               zeroes on the stream in front (update_norm.hip's idiom).
// The term of a face is formed on the float's bits: the mantissa shifted by (its exponent - 23) - q, towards zero -- what
// (int64_t)trunc(ldexp((double)p, -q)) gives, exactly.  Integer sums, maxima of bit patterns and counts do not depend on
// the order of reduction: the two samplers write the same bytes for the same shape, mask, labels and pressure.
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): DESIGN.md 4.13; no scratch in any of the three kernels.
#include <algorithm>

#include "load_kernels.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

constexpr int kT = kLoadThreads, kB = SFL_MAX_BODIES;
static_assert(sizeof(struct sfl_body_load) == 48 && kT >= kB && kT % 64 == 0, "include/sfl.h: 48 bytes; a thread per body");

// q of a body from the bits of its max_abs_p: floor(log2) - 32, denormals included; 0 for 0.0f
__device__ __forceinline__ int exp2_of(unsigned max_bits)
{
    if (max_bits == 0u) return 0;
    const int e = (int)(max_bits >> 23);
    return (e ? e - 127 : (31 - __clz(max_bits)) - 149) - 32;
}

// trunc(p * 2^-q) of a finite p with |p| <= the body's maximum, from p's bits: |result| < 2^33
__device__ __forceinline__ long long term_of(unsigned bits, int q)
{
    const int e = (int)((bits >> 23) & 0xffu);
    const u64 mant = (bits & 0x7fffffu) | (e ? 0x800000u : 0u);
    const int shift = (e ? e : 1) - 150 - q;   // <= 32 (a denormal maximum), <= 9 (a normal one)
    const u64 mag = shift >= 0 ? mant << shift : (shift > -24 ? mant >> -shift : 0ull);
    return (bits >> 31) ? -(long long)mag : (long long)mag;
}

__device__ __forceinline__ bool wet_candidate(unsigned code) { return (code & 16u) && (code & 15u) != 15u; }

// Which neighbours of fluid cell c = dim_x * j + i, whose code byte lacks one, are solid cells INSIDE the domain, by the
// cell's coordinates: bit dir set = a face with the FLUID cell lying dir of the solid one, 0 W, 1 E, 2 S, 3 N.  0 for a
// cell that only touches the rim: it reads neither p nor a label.
__device__ __forceinline__ unsigned face_bits(unsigned code, int c, int dim_x, int dim_y)
{
    const int j = c / dim_x, i = c - j * dim_x;
    return (unsigned)(!(code & 2u) && i < dim_x - 1) | (unsigned)(!(code & 1u) && i > 0) << 1 | (unsigned)(!(code & 8u) && j < dim_y - 1) << 2 |
           (unsigned)(!(code & 4u) && j > 0) << 3;
}

// fn(body - 1, dir) for each face of face_bits that belongs to a body.  labels: the member's, or null (every solid cell is body 1).
template <class Fn>
__device__ __forceinline__ void wet_faces(unsigned faces, int c, int dim_x, const uint8_t *labels, int bodies, Fn fn)
{
    const int at[4] = {c + 1, c - 1, c + dim_x, c - dim_x};
#pragma unroll
    for (int dir = 0; dir < 4; ++dir)
        if (faces >> dir & 1u) {
            const int body = labels ? (int)labels[at[dir]] : 1;
            if (body >= 1 && body <= bodies) fn(body - 1, dir);
        }
}

// what a workgroup gathers of its faces, per body
struct Gathered {
    unsigned max_bits[kB];
    u64 fx[kB], fy[kB];
    unsigned faces[kB][4], nonfinite[kB];
};

__device__ __forceinline__ void clear(Gathered &g)
{
    if (threadIdx.x < kB) {
        const int k = threadIdx.x;
        g.max_bits[k] = 0u;
        g.fx[k] = g.fy[k] = 0ull;
        g.faces[k][0] = g.faces[k][1] = g.faces[k][2] = g.faces[k][3] = g.nonfinite[k] = 0u;
    }
}

// one face into the body's sums (g.max_bits holds the finished maxima)
__device__ __forceinline__ void add_face(Gathered &g, int body, int dir, unsigned bits)
{
    atomicAdd(&g.faces[body][dir], 1u);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        atomicAdd(&g.nonfinite[body], 1u);
        return;
    }
    const long long t = term_of(bits, exp2_of(g.max_bits[body]));
    atomicAdd(dir < 2 ? &g.fx[body] : &g.fy[body], (u64)((dir & 1) ? -t : t));   // (two's complement: the sum of the signed terms)
}

__global__ void __launch_bounds__(kT) batch_loads_kernel(const BatchLoadSample a)
{
    __shared__ Gathered g;
    const int member = a.first + (int)blockIdx.x, dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y, bodies = a.bodies;
    const float *p = a.p + (size_t)member * (size_t)cells;
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
        if (!faces) continue;                                         // (the rim alone: no load of p)
        const unsigned bits = __float_as_uint(p[c]) & 0x7fffffffu;   // |p|
        if (bits >= 0x7f800000u) continue;                            // (not finite: no part in the maximum)
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int) {
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
        const unsigned bits = __float_as_uint(p[c]);
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) { add_face(g, body, dir, bits); });
    }
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_load r;
        r.fx = (int64_t)g.fx[k];
        r.fy = (int64_t)g.fy[k];
        r.exp2 = exp2_of(g.max_bits[k]);
        r.max_abs_p = __uint_as_float(g.max_bits[k]);
#pragma unroll
        for (int d = 0; d < 4; ++d) r.faces[d] = g.faces[k][d];
        r.nonfinite = g.nonfinite[k];
        r.reserved = 0u;
        a.out[(size_t)blockIdx.x * bodies + k] = r;
    }
}

// SUMS false: the maxima into max_abs_p of the zeroed records; true: everything else, from the finished maxima
template <bool SUMS>
__global__ void __launch_bounds__(kT) context_loads_kernel(const ContextLoadSample a, int cells, int groups, bool aligned)
{
    __shared__ Gathered g;
    const int dim_x = a.dim_x, dim_y = a.dim_y, bodies = a.bodies;
    clear(g);
    __syncthreads();
    if (SUMS) {
        if ((int)threadIdx.x < bodies) g.max_bits[threadIdx.x] = __float_as_uint(a.out[threadIdx.x].max_abs_p);
        __syncthreads();
    }
    const auto cell = [&](int c, unsigned code) {
        const unsigned faces = face_bits(code, c, dim_x, dim_y);
        if (!faces) return;   // (the rim alone: no load of p)
        const unsigned bits = __float_as_uint(a.p[c]);
        if (!SUMS && (bits & 0x7f800000u) == 0x7f800000u) return;
        wet_faces(faces, c, dim_x, a.labels, bodies, [&](int body, int dir) {
            if (SUMS)
                add_face(g, body, dir, bits);
            else
                atomicMax(&g.max_bits[body], bits & 0x7fffffffu);
        });
    };
    for (int grp = blockIdx.x * kT + threadIdx.x; grp < groups; grp += gridDim.x * kT) {
        const int base = grp * kLoadGroupCells;   // < 2^28
        if (aligned && base + kLoadGroupCells <= cells) {
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
            const int end = min(base + kLoadGroupCells, cells);
            for (int c = base; c < end; ++c) {
                const unsigned code = a.codes[c];
                if (wet_candidate(code)) cell(c, code);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        struct sfl_body_load *r = a.out + k;
        if (!SUMS) {
            if (g.max_bits[k]) atomicMax(reinterpret_cast<unsigned *>(&r->max_abs_p), g.max_bits[k]);
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

hipError_t launch_batch_loads(hipStream_t s, const BatchLoadSample &a)
{
    if (a.count < 1 || a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    batch_loads_kernel<<<a.count, kT, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_context_loads(hipStream_t s, const ContextLoadSample &a)
{
    if (a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.out, 0, (size_t)a.bodies * sizeof(struct sfl_body_load), s);
    if (e != hipSuccess) return e;
    const long long cells = (long long)a.dim_x * a.dim_y;   // <= 2^28
    const int groups = (int)((cells + kLoadGroupCells - 1) / kLoadGroupCells);
    const int blocks = std::min((groups + kT - 1) / kT, kLoadMaxBlocks);
    const bool aligned = reinterpret_cast<uintptr_t>(a.codes) % 16 == 0;
    context_loads_kernel<false><<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    context_loads_kernel<true><<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    return hipGetLastError();
}

}  // namespace sfl
