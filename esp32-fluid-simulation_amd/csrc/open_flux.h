// open_flux.h -- the flux through the live open cells of a grid (include/sfl.h "INFLOW PROFILES AND FLUX"), written ONCE for
// the kernels of inflow.hip and for a host program (tests/cpp/inflow_driver.cpp), like diffuse_tile.h and sor_open_tile.h:
// the walk over the rim, the outward normal of a cell, the loads' quantisation (loads.hip exp2_of, term_of: word for word)
// and the two passes -- the maximum, then the sums -- as what one lane or one host loop gathers.  Plain integer arithmetic
// on the bits of the floats: no float is added or compared anywhere.
//
// OPEN BITS of a cell, five of them: which neighbour is open (1 W, 2 E, 4 S, 8 N) and 16 = the opening is an outflow -- the
// open byte of a context (sor_open_tile.h) and bits 8..12 of a batch's open code (advect_math.h).  They are nonzero only
// in a FLUID cell whose map byte is nonzero: a live open cell.
#pragma once
#include <stdint.h>

#include "../../include/sfl.h"

#if defined(__HIPCC__)
#define SFL_FLUX_HD __host__ __device__ __forceinline__
#else
#define SFL_FLUX_HD inline
#endif

namespace sfl {
namespace open_flux {

constexpr unsigned kSides = 15u, kOutflow = 16u;

// the rim of a dim_x x dim_y grid as a list: the S row, the N row, then the W and E cells of rows 1 .. dim_y - 2 in turn.
// Corners come with the rows; they carry no opening.
SFL_FLUX_HD int rim_cells(int dim_x, int dim_y) { return 2 * dim_x + 2 * (dim_y > 2 ? dim_y - 2 : 0); }
SFL_FLUX_HD int rim_cell(int r, int dim_x, int dim_y)
{
    if (r < dim_x) return r;
    if (r < 2 * dim_x) return (dim_y - 1) * dim_x + (r - dim_x);
    const int k = r - 2 * dim_x;
    return (1 + (k >> 1)) * dim_x + ((k & 1) ? dim_x - 1 : 0);
}

// the bits of n, the outward normal component: -v.x on the W rim, +v.x on E, -v.y on S, +v.y on N
SFL_FLUX_HD unsigned normal_bits(unsigned open, unsigned vx_bits, unsigned vy_bits)
{
    const unsigned comp = (open & 3u) ? vx_bits : vy_bits;
    return (open & 5u) ? comp ^ 0x80000000u : comp;
}
SFL_FLUX_HD bool is_nonfinite(unsigned bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// q from the bits of max_abs_n: floor(log2) - 32, denormals included; 0 for 0.0f
SFL_FLUX_HD int exp2_of(unsigned max_bits)
{
    if (max_bits == 0u) return 0;
    const int e = (int)(max_bits >> 23);
    return (e ? e - 127 : (31 - __builtin_clz(max_bits)) - 149) - 32;
}

// trunc(n * 2^-q) of a finite n with |n| <= the maximum, from n's bits: |result| < 2^33
SFL_FLUX_HD long long term_of(unsigned bits, int q)
{
    const int e = (int)((bits >> 23) & 0xffu);
    const unsigned long long mant = (bits & 0x7fffffu) | (e ? 0x800000u : 0u);
    const int shift = (e ? e : 1) - 150 - q;   // <= 32 (a denormal maximum), <= 9 (a normal one)
    const unsigned long long mag = shift >= 0 ? mant << shift : (shift > -24 ? mant >> -shift : 0ull);
    return (bits >> 31) ? -(long long)mag : (long long)mag;
}

// what one lane (or the host's one loop) gathers
struct Partial {
    unsigned max_bits, in_cells, out_cells, nonfinite;
    long long in, out;   // the sums of t over the inflow and over the outflow cells
};

// pass 1 of a live open cell: the counts and the maximum
SFL_FLUX_HD void gather_max(Partial &p, unsigned open, unsigned n_bits)
{
    if (open & kOutflow) ++p.out_cells;
    else ++p.in_cells;
    if (is_nonfinite(n_bits)) {
        ++p.nonfinite;
        return;
    }
    const unsigned a = n_bits & 0x7fffffffu;
    p.max_bits = a > p.max_bits ? a : p.max_bits;
}

// pass 2 of a live open cell: its term into the sum of its kind
SFL_FLUX_HD void gather_term(Partial &p, unsigned open, unsigned n_bits, int q)
{
    if (is_nonfinite(n_bits)) return;
    const long long t = term_of(n_bits, q);
    if (open & kOutflow) p.out += t;
    else p.in += t;
}

// the record from what all lanes gathered
SFL_FLUX_HD void finish(struct sfl_open_flux *r, const Partial &p)
{
    union {
        unsigned u;
        float f;
    } m;
    m.u = p.max_bits;
    r->inflow = -p.in;   // positive when fluid enters
    r->outflow = p.out;
    r->exp2 = exp2_of(p.max_bits);
    r->max_abs_n = m.f;
    r->inflow_cells = p.in_cells;
    r->outflow_cells = p.out_cells;
    r->nonfinite = p.nonfinite;
    r->reserved = 0u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole record of one grid on the host, by the walk and the passes of the kernels.  v: (x, y) per cell as bits; open:
// the open bits of cell c.
template <class Open>
inline void flux_on_host(struct sfl_open_flux *r, const uint32_t *v_bits, Open open, int dim_x, int dim_y)
{
    Partial p = {0u, 0u, 0u, 0u, 0, 0};
    const int rim = rim_cells(dim_x, dim_y);
    for (int k = 0; k < rim; ++k) {
        const int c = rim_cell(k, dim_x, dim_y);
        const unsigned o = open(c);
        if (o & kSides) gather_max(p, o, normal_bits(o, v_bits[2 * c], v_bits[2 * c + 1]));
    }
    const int q = exp2_of(p.max_bits);
    for (int k = 0; k < rim; ++k) {
        const int c = rim_cell(k, dim_x, dim_y);
        const unsigned o = open(c);
        if (o & kSides) gather_term(p, o, normal_bits(o, v_bits[2 * c], v_bits[2 * c + 1]), q);
    }
    finish(r, p);
}
#endif

}  // namespace open_flux
}  // namespace sfl
