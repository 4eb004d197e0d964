// body_walk.h -- the samplers of one record per solid body, whatever is summed over the body's wet faces, written once for
// loads.hip (include/sfl.h "LOADS": the pressure of the fluid cell), friction.hip ("FRICTION": its tangential velocity) and
// torque.hip ("TORQUE": both, times an arm): the walks over the wet faces, the exact-integer quantisation of a face's term,
// the launchers, and the kernel bodies of the two kinds that sum ONE field (loads, friction), generic over that kind.
// Included by those three units only; everything lives in the including unit's anonymous namespace.
//
// All read the code bytes of the solids (solids.cpp solid_codes: bit 0 W, 1 E, 2 S, 3 N neighbour present, bit 4 the cell
// is fluid): a fluid cell with an absent neighbour that is INSIDE THE DOMAIN -- derived from the cell's coordinates, not from
// the byte -- has a solid cell there, whose label (1 without labels) names the body of that wet face.  Only such a cell
// divides its index into (i, j), and only one with a face reads a field and its solid neighbours' labels.
//
//   A batch     one workgroup per member (member_walk), launched behind the step whose fields it reads.  Pass 1 gathers per
//               body what the scale of the terms needs (the maxima); barrier; pass 2, the same walk, puts every face's term
//               into the body's 64-bit LDS accumulator and counters; barrier.  Thread k stores the record of body k + 1 with
//               ordinary stores: no global atomics, no memset in front.
//   A context   a streaming pass (context_walk) over the code bytes taken as ONE flat array: a thread takes 16 cells with one
//               16-byte load (the array starts 16-byte aligned, so every group does whatever the width; the cells of the last,
//               partial group -- and every group if the array is not aligned -- come by byte loads) and skips a word whose
//               bytes are all 0 or all 0x1F: nothing wet, which is nearly all of a large grid.  Two launches (launch_context):
//               pass 1, then the sums, which read the finished pass 1.  Each folds its faces into LDS words per body and
//               issues at most one integer atomic per workgroup and touched field of a body, on records the launcher zeroes
//               on the stream in front (update_norm.hip's idiom); the fields no atomic touches are stored by workgroup 0.
// The term of a face is formed on the float's bits: the mantissa shifted by (its exponent - 23) - q, towards zero -- what
// (int64_t)trunc(ldexp((double)x, -q)) gives, exactly.  Integer sums, maxima of bit patterns and counts do not depend on the
// order of reduction: the two samplers of a kind write the same bytes for the same shape, mask, labels and fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/sfl.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

constexpr int kB = SFL_MAX_BODIES;
constexpr int kT = 256;            // threads of a sampler's workgroup, batch and context
constexpr int kGroupCells = 16;    // code bytes a thread of a context's passes takes with one load
constexpr int kMaxBlocks = 2048;   // workgroups of a context's pass at most: they stride over the groups
static_assert(kT >= kB && kT % 64 == 0 && kGroupCells == 16, "a thread per body, whole waves; a group is one uint4");

// q of a body from the bits of its maximum: floor(log2) - 32, denormals included; 0 for 0.0f
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

// the bits of the tangential component of a face in direction dir
__device__ __forceinline__ unsigned tangential(float2 v, int dir) { return __float_as_uint(dir < 2 ? v.y : v.x); }

__device__ __forceinline__ bool wet_candidate(unsigned code) { return (code & 16u) && (code & 15u) != 15u; }

// Which neighbours of fluid cell c = dim_x * j + i, whose code byte lacks one, are solid cells INSIDE the domain, by the
// cell's coordinates: bit dir set = a face with the FLUID cell lying dir of the solid one, 0 W, 1 E, 2 S, 3 N.  0 for a
// cell that only touches the rim: it reads neither a field nor a label.
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

// fn(c, faces) for the cell of code byte `code`, if it is fluid and face_bits finds a face
template <class Fn>
__device__ __forceinline__ void wet_cell(unsigned code, int c, int dim_x, int dim_y, Fn fn)
{
    if (!wet_candidate(code)) return;
    const unsigned faces = face_bits(code, c, dim_x, dim_y);
    if (faces) fn(c, faces);   // (the rim alone: no load of a field)
}

// A batch's walk: fn(c, faces) for every cell of a member with a wet face, strided over the workgroup.
template <class Fn>
__device__ __forceinline__ void member_walk(const uint8_t *codes, int dim_x, int dim_y, Fn fn)
{
    for (int c = threadIdx.x; c < dim_x * dim_y; c += kT) wet_cell(codes[c], c, dim_x, dim_y, fn);
}

// A context's streaming pass: fn(c, faces) for every cell with a wet face, the groups of 16 code bytes strided over the grid.
template <class Fn>
__device__ __forceinline__ void context_walk(const uint8_t *codes, int dim_x, int dim_y, int cells, int groups, bool aligned, Fn fn)
{
    for (int grp = blockIdx.x * kT + threadIdx.x; grp < groups; grp += gridDim.x * kT) {
        const int base = grp * kGroupCells;   // < 2^28
        if (aligned && base + kGroupCells <= cells) {
            const uint4 w = *reinterpret_cast<const uint4 *>(codes + base);
            const unsigned words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (words[k] == 0u || words[k] == 0x1f1f1f1fu) continue;   // four solid cells, or four with every neighbour present
#pragma unroll
                for (int q = 0; q < 4; ++q) wet_cell((words[k] >> (8 * q)) & 0xffu, base + 4 * k + q, dim_x, dim_y, fn);
            }
        } else {
            const int end = min(base + kGroupCells, cells);
            for (int c = base; c < end; ++c) wet_cell(codes[c], c, dim_x, dim_y, fn);
        }
    }
}

// One sample of a batch: a workgroup per member.  A: the kind's Batch...Sample (its *_kernels.h).
template <class A>
hipError_t launch_batch(hipStream_t s, const A &a, void (*kernel)(A))
{
    if (a.count < 1 || a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    kernel<<<a.count, kT, 0, s>>>(a);
    return hipGetLastError();
}

// One sample of a context: the records zeroed, then kernel<false> (pass 1), then kernel<true> (the sums).  A: the kind's Context...Sample.
template <class A>
hipError_t launch_context(hipStream_t s, const A &a, void (*pass1)(A, int, int, bool), void (*sums)(A, int, int, bool))
{
    if (a.bodies < 1 || a.bodies > kB) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.out, 0, (size_t)a.bodies * sizeof(*a.out), s);
    if (e != hipSuccess) return e;
    const long long cells = (long long)a.dim_x * a.dim_y;   // <= 2^28
    const int groups = (int)((cells + kGroupCells - 1) / kGroupCells);
    const int blocks = std::min((groups + kT - 1) / kT, kMaxBlocks);
    const bool aligned = reinterpret_cast<uintptr_t>(a.codes) % 16 == 0;
    pass1<<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    sums<<<blocks, kT, 0, s>>>(a, (int)cells, groups, aligned);
    return hipGetLastError();
}

// ---- the kinds that sum one field: fx, fy, an exponent, a maximum, the face counts (sfl_body_load, sfl_body_friction) ----
// For loads.hip and friction.hip only: torque.hip gathers other quantities (its TorqueGathered) and instantiates none of this.  A
// kind K (the device side of LoadsKind / FrictionKind of loads.cpp / friction.cpp) is a struct of statics:
//     field(a)                 the field of a sample struct, a pointer to one Value per cell
//     bits(value, dir)         the float's bits that a face in direction dir takes of its fluid cell's value
//     sum(g, body, dir, t)     the face's signed term t into the body's fx or fy
//     maximum(record)          the record's maximum, a float lvalue

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
template <class K>
__device__ __forceinline__ void add_face(Gathered &g, int body, int dir, unsigned bits)
{
    atomicAdd(&g.faces[body][dir], 1u);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        atomicAdd(&g.nonfinite[body], 1u);
        return;
    }
    K::sum(g, body, dir, term_of(bits, exp2_of(g.max_bits[body])));   // (two's complement: the sum of the signed terms)
}

// Pass 1: every thread keeps the maximum of the bit patterns of |value| per body in registers (sixteen words, indexed at
// compile time), the wave reduces the bodies in use by __shfl_xor and its lane 0 folds them into LDS.
template <class K, class A>
__device__ __forceinline__ void batch_sample(const A &a)
{
    __shared__ Gathered g;
    const int member = a.first + (int)blockIdx.x, dim_x = a.dim_x, dim_y = a.dim_y, bodies = a.bodies;
    const auto *field = K::field(a) + (size_t)member * (size_t)(dim_x * dim_y);
    const uint8_t *codes = a.codes + (size_t)member * a.code_stride;
    const uint8_t *labels = a.labels ? a.labels + (size_t)member * a.label_stride : nullptr;
    clear(g);
    __syncthreads();
    unsigned m[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) m[k] = 0u;
    member_walk(codes, dim_x, dim_y, [&](int c, unsigned faces) {
        const auto value = field[c];
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) {
            const unsigned bits = K::bits(value, dir) & 0x7fffffffu;
            if (bits >= 0x7f800000u) return;   // (not finite: no part in the maximum)
#pragma unroll
            for (int k = 0; k < kB; ++k) m[k] = (k == body && bits > m[k]) ? bits : m[k];
        });
    });
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
    member_walk(codes, dim_x, dim_y, [&](int c, unsigned faces) {
        const auto value = field[c];
        wet_faces(faces, c, dim_x, labels, bodies, [&](int body, int dir) { add_face<K>(g, body, dir, K::bits(value, dir)); });
    });
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        typename K::Record r;
        r.fx = (int64_t)g.fx[k];
        r.fy = (int64_t)g.fy[k];
        r.exp2 = exp2_of(g.max_bits[k]);
        K::maximum(r) = __uint_as_float(g.max_bits[k]);
#pragma unroll
        for (int d = 0; d < 4; ++d) r.faces[d] = g.faces[k][d];
        r.nonfinite = g.nonfinite[k];
        r.reserved = 0u;
        a.out[(size_t)blockIdx.x * bodies + k] = r;
    }
}

// SUMS false: the maxima into the maximum of the zeroed records; true: everything else, from the finished maxima
template <class K, bool SUMS, class A>
__device__ __forceinline__ void context_sample(const A &a, int cells, int groups, bool aligned)
{
    __shared__ Gathered g;
    const int dim_x = a.dim_x, dim_y = a.dim_y, bodies = a.bodies;
    clear(g);
    __syncthreads();
    if (SUMS) {
        if ((int)threadIdx.x < bodies) g.max_bits[threadIdx.x] = __float_as_uint(K::maximum(a.out[threadIdx.x]));
        __syncthreads();
    }
    context_walk(a.codes, dim_x, dim_y, cells, groups, aligned, [&](int c, unsigned faces) {
        const auto value = K::field(a)[c];
        wet_faces(faces, c, dim_x, a.labels, bodies, [&](int body, int dir) {
            const unsigned bits = K::bits(value, dir);
            if (SUMS)
                add_face<K>(g, body, dir, bits);
            else if ((bits & 0x7f800000u) != 0x7f800000u)
                atomicMax(&g.max_bits[body], bits & 0x7fffffffu);
        });
    });
    __syncthreads();
    if ((int)threadIdx.x < bodies) {
        const int k = threadIdx.x;
        typename K::Record *r = a.out + k;
        if (!SUMS) {
            if (g.max_bits[k]) atomicMax(reinterpret_cast<unsigned *>(&K::maximum(*r)), g.max_bits[k]);
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
}  // namespace sfl
