// body_walk.h -- the walk over the wet faces of solid bodies and the exact-integer quantisation of a face's term, written once
// for the two samplers that use them: loads.hip (include/sfl.h "LOADS": the pressure of the fluid cell) and friction.hip
// ("FRICTION": its tangential velocity).  Device code only; everything lives in the including unit's anonymous namespace.
//
// Both read the code bytes of the solids (solids.cpp solid_codes: bit 0 W, 1 E, 2 S, 3 N neighbour present, bit 4 the cell
// is fluid): a fluid cell with an absent neighbour that is INSIDE THE DOMAIN -- derived from the cell's coordinates, not from
// the byte -- has a solid cell there, whose label (1 without labels) names the body of that wet face.
// The term of a face is formed on the float's bits: the mantissa shifted by (its exponent - 23) - q, towards zero -- what
// (int64_t)trunc(ldexp((double)x, -q)) gives, exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sfl.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

constexpr int kB = SFL_MAX_BODIES;

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

}  // namespace
}  // namespace sfl
