// advect_math.h -- per-cell arithmetic of the sim step outside the pressure solve (semi-Lagrangian advection,
// divergence, v - grad p), each stencil written ONCE and shared by the one-thread-per-cell kernels
// (stencil_kernels.hip), the LDS-staged tile kernels (advect_tiled.hip, advect_seam.h) and the one-workgroup
// step (small_step_body.inc).
//
// Numerics contract: compiled with -ffp-contract=off; every product and sum is
// individually rounded in the order the reference evaluates it.  Reference citations are file:line
// under /root/reference/ESP32-fluid-simulation/.
#pragma once
#include "kernels.h"
#include <type_traits>

namespace sfl {
namespace advect_math {

__device__ __forceinline__ size_t lcell(const Slab &g, int i, int gj)
{
    return (size_t)(gj - g.grow0) * (size_t)g.dim_x + (size_t)i;
}

// lerp(t, a, b) = a*(1-t) + b*t  (advect.h:13-16)
__device__ __forceinline__ float mix1(float t, float a, float b)
{
    const float wa = 1.0f - t;
    const float pa = a * wa;
    const float pb = b * t;
    return pa + pb;
}

// uq32.h:13 / :15
__device__ __forceinline__ uint32_t uq_narrow(float x) { return (uint32_t)(x + 0.5f); }
__device__ __forceinline__ float uq_widen(uint32_t raw) { return (float)raw; }

struct SrcPos {
    bool x_under, y_under, x_oob, y_oob;
    int ci, cj;
    float di, dj;
};

// advect.h:26-35
__device__ __forceinline__ SrcPos classify(float si, float sj, int dim_x, int gdim_y)
{
    SrcPos s;
    const bool x_over = si >= (float)(dim_x - 1);
    const bool y_over = sj >= (float)(gdim_y - 1);
    const float fi = floorf(si), fj = floorf(sj);
    s.x_under = si < 0.0f;
    s.y_under = sj < 0.0f;
    s.x_oob = s.x_under || x_over;
    s.y_oob = s.y_under || y_over;
    s.di = si - fi;
    s.dj = sj - fj;
    s.ci = s.x_oob ? (s.x_under ? 0 : dim_x - 1) : (int)fi;
    s.cj = s.y_oob ? (s.y_under ? 0 : gdim_y - 1) : (int)fj;
    return s;
}

// advect.h:62-70
__device__ __forceinline__ float wall_discount(const SrcPos &s, float si, float sj, int dim_x,
                                               int gdim_y)
{
    float factor = 1.0f;
    if (s.x_oob) {
        const float over = s.x_under ? -si : si - (float)(dim_x - 1);
        factor *= (over < 0.5f) ? (1.0f - 2.0f * over) : 0.0f;
    }
    if (s.y_oob) {
        const float over = s.y_under ? -sj : sj - (float)(gdim_y - 1);
        factor *= (over < 0.5f) ? (1.0f - 2.0f * over) : 0.0f;
    }
    return factor;
}

// rows of p touched by a sample at s: [cj, cj + (y in range ? 1 : 0)]
__device__ __forceinline__ bool rows_available(const SrcPos &s, int valid_begin, int valid_end)
{
    const int last = s.cj + (s.y_oob ? 0 : 1);
    return s.cj >= valid_begin && last < valid_end;
}

// the four texels of an in-domain sample mixed (advect.h:40-43): pIJ = texel (ci + I - 1, cj + J - 1)
__device__ __forceinline__ float mix4(const SrcPos &s, float p11, float p12, float p21, float p22)
{
    return mix1(s.di, mix1(s.dj, p11, p12), mix1(s.dj, p21, p22));
}
__device__ __forceinline__ float2 mix4(const SrcPos &s, float2 p11, float2 p12, float2 p21, float2 p22)
{
    float2 r;
    r.x = mix4(s, p11.x, p12.x, p21.x, p22.x);
    r.y = mix4(s, p11.y, p12.y, p21.y, p22.y);
    return r;
}

// sample() of a float2 field (advect.h:37-72); texel(a, b) is the field at cell (s.ci + a, s.cj + b), a and b
// 0 or 1, of a domain of dim_x x gdim_y cells
template <bool NO_SLIP, class T>
__device__ __forceinline__ float2 sample_vec2f(const SrcPos &s, float si, float sj, int dim_x, int gdim_y,
                                               T texel)
{
    float2 r;
    if (!s.x_oob && !s.y_oob) {
        const float2 p11 = texel(0, 0), p12 = texel(0, 1), p21 = texel(1, 0), p22 = texel(1, 1);
        r = mix4(s, p11, p12, p21, p22);
    } else {
        if (s.x_oob && s.y_oob) {
            r = texel(0, 0);
        } else if (s.x_oob) {
            const float2 a = texel(0, 0), b = texel(0, 1);
            r.x = mix1(s.dj, a.x, b.x);
            r.y = mix1(s.dj, a.y, b.y);
        } else {
            const float2 a = texel(0, 0), b = texel(1, 0);
            r.x = mix1(s.di, a.x, b.x);
            r.y = mix1(s.di, a.y, b.y);
        }
        if (NO_SLIP) {
            const float f = wall_discount(s, si, sj, dim_x, gdim_y);
            r.x = r.x * f;
            r.y = r.y * f;
        }
    }
    return r;
}

// the same of a field's array in memory; gs = geometry of that array
template <bool NO_SLIP>
__device__ __forceinline__ float2 sample_global_vec2f(const float2 *p, const Slab &gs, const SrcPos &s, float si,
                                                      float sj)
{
    const size_t t = lcell(gs, s.ci, s.cj);
    return sample_vec2f<NO_SLIP>(s, si, sj, gs.dim_x, gs.gdim_y,
                                 [&](int a, int b) { return p[t + b * gs.dim_x + a]; });
}

// the same of a float2 field in LDS: the pointer carries the address space, so the gathers are LDS reads whatever the
// compiler can or cannot infer about where p points (batch_play.hip: the source region changes from step to step).
// p = the field's first float; the two components of a texel are read as floats and put together.
typedef const __attribute__((address_space(3))) float lds_cfloat;
template <bool NO_SLIP>
__device__ __forceinline__ float2 sample_lds_vec2f(lds_cfloat *p, const Slab &gs, const SrcPos &s, float si, float sj)
{
    const int t = (s.cj - gs.grow0) * gs.dim_x + s.ci;
    return sample_vec2f<NO_SLIP>(s, si, sj, gs.dim_x, gs.gdim_y, [&](int a, int b) {
        const int c = 2 * (t + b * gs.dim_x + a);
        return make_float2(p[c], p[c + 1]);
    });
}

// calculate_divergence for one cell (finitediff.cpp:9-31), before the factor 1 / (2 dx); q points at the cell,
// in an LDS window or an array in memory, rows `stride` apart
__device__ __forceinline__ float divergence_sum(const float2 *q, int stride, int i, int gj, int i_max, int j_max)
{
    float s;
    if (i > 0 && i < i_max && gj > 0 && gj < j_max) {  // div_expr_fast, :29
        const float hx = -q[-1].x + q[1].x;
        const float hy = -q[-stride].y + q[stride].y;
        s = hx + hy;
    } else {  // div_expr_safe, :15-20: ghost velocity = -own
        const float2 own = q[0];
        s = 0.0f;
        s += (i > 0) ? -q[-1].x : own.x;
        s += (i < i_max) ? q[1].x : -own.x;
        s += (gj > 0) ? -q[-stride].y : own.y;
        s += (gj < j_max) ? q[stride].y : -own.y;
    }
    return s;
}

// subtract_gradient for one cell (finitediff.cpp:41-73): v - grad p, a missing neighbour's pressure is the
// cell's own; pressure_at(a, b) is the pressure of cell (a, b)
template <class P>
__device__ __forceinline__ float2 project_cell(float2 u, int i, int gj, int i_max, int j_max, float two_dx_inv,
                                               P pressure_at)
{
    const float pc = pressure_at(i, gj);
    const float pw = (i > 0) ? pressure_at(i - 1, gj) : pc;
    const float pe = (i < i_max) ? pressure_at(i + 1, gj) : pc;
    const float ps = (gj > 0) ? pressure_at(i, gj - 1) : pc;
    const float pn = (gj < j_max) ? pressure_at(i, gj + 1) : pc;
    const float gx = (pe - pw) * two_dx_inv;
    const float gy = (pn - ps) * two_dx_inv;
    u.x = u.x - gx;
    u.y = u.y - gy;
    return u;
}
// the same with q pointing at the cell's pressure, rows `stride` apart (the offsets fold to constants)
__device__ __forceinline__ float2 project_cell(float2 u, const float *q, int stride, int i, int gj, int i_max,
                                               int j_max, float two_dx_inv)
{
    return project_cell(u, i, gj, i_max, j_max, two_dx_inv,
                        [=](int a, int b) { return q[(b - gj) * stride + (a - i)]; });
}

// ---- solid cells inside a grid (include/sfl.h "SOLIDS"; batch_solids.hip) -------------------------------------------
// One code byte per cell says everything a stencil needs to know: bit 0 W, 1 E, 2 S, 3 N neighbour PRESENT (inside the
// domain and fluid), bit 4 the cell itself is fluid; a solid cell's byte is 0.  A set neighbour bit implies that the
// neighbour is inside the domain, so a stencil keyed on the byte reads nothing outside the field.
constexpr int kSolidW = 1, kSolidE = 2, kSolidS = 4, kSolidN = 8, kSolidFluid = 16, kSolidAll = 15;

// The stencils above know "absent" as "outside the domain": (i > 0), (i < i_max), (gj > 0), (gj < j_max).  A code byte says
// the same through coordinates made for the purpose -- a cell at i = 1 or 0 (W present or not) of a row that ends at i + 1
// or i (E present or not), and so for the rows -- so the ONE statement of each stencil serves solids too, and the kernels
// that exist keep their instructions.
struct SolidSpot {
    int i, gj, i_max, j_max;
};
__device__ __forceinline__ SolidSpot solid_spot(int code)
{
    SolidSpot t;
    t.i = (code & kSolidW) ? 1 : 0;
    t.gj = (code & kSolidS) ? 1 : 0;
    t.i_max = t.i + ((code & kSolidE) ? 1 : 0);
    t.j_max = t.gj + ((code & kSolidN) ? 1 : 0);
    return t;
}

// divergence_sum with "absent" read from the code byte: all four present div_expr_fast, otherwise div_expr_safe with an
// absent neighbour's term the cell's own component (ghost velocity = -own); a solid cell has no divergence (0.0f)
__device__ __forceinline__ float divergence_sum_solid(const float2 *q, int stride, int code)
{
    if (!(code & kSolidFluid)) return 0.0f;
    const SolidSpot t = solid_spot(code);
    return divergence_sum(q, stride, t.i, t.gj, t.i_max, t.j_max);
}

// project_cell with "absent" read from the code byte: an absent neighbour's pressure is the cell's own; a solid cell's
// velocity is (0, 0).  q points at the cell's pressure, rows `stride` apart.
__device__ __forceinline__ float2 project_cell_solid(float2 u, const float *q, int stride, int code, float two_dx_inv)
{
    if (!(code & kSolidFluid)) return make_float2(0.0f, 0.0f);
    const SolidSpot t = solid_spot(code);
    return project_cell(u, q, stride, t.i, t.gj, t.i_max, t.j_max, two_dx_inv);
}

// ---- openings on the rim of a grid (include/sfl.h "OPENINGS"; batch_openings.hip) -----------------------------------
// A cell's OPEN CODE is its code byte with the opening above it: bits 8..11 say which neighbour -- W, E, S, N, the one outside
// the domain -- is OPEN, bit 12 that the opening is an outflow (else an inflow).  Set only in a fluid rim cell that is no
// corner; the bit of the open side is never set among bits 0..3.  With bits 8..12 clear the functions below are the solids'.
constexpr int kOpenShift = 8, kOpenOutflow = 1 << 12;
__device__ __forceinline__ int open_sides(int code) { return (code >> kOpenShift) & kSolidAll; }
// a fluid cell that holds the inflow velocity (item 2a)
__device__ __forceinline__ bool is_inflow_cell(int code) { return open_sides(code) != 0 && !(code & kOpenOutflow); }

// an absent neighbour's term of div_expr_safe: the wall's ghost term as it stands, or with the opposite sign where the
// neighbour is open -- the ghost moves with the cell and the flow passes
__device__ __forceinline__ float ghost_term(float wall_term, int open) { return open ? -wall_term : wall_term; }

// divergence_sum_solid for open codes: a cell with an open neighbour takes the safe form
__device__ __forceinline__ float divergence_sum_open(const float2 *q, int stride, int code)
{
    const int open = open_sides(code);
    if (!open) return divergence_sum_solid(q, stride, code & 0xff);
    const float2 own = q[0];
    float s = 0.0f;
    s += (code & kSolidW) ? -q[-1].x : ghost_term(own.x, open & kSolidW);
    s += (code & kSolidE) ? q[1].x : ghost_term(-own.x, open & kSolidE);
    s += (code & kSolidS) ? -q[-stride].y : ghost_term(own.y, open & kSolidS);
    s += (code & kSolidN) ? q[stride].y : ghost_term(-own.y, open & kSolidN);
    return s;
}

// project_cell_solid for open codes: an outflow neighbour's pressure is +0.0f, an inflow neighbour's the cell's own as an
// absent one's.  The outflow side is handed to project_cell as present and answered here, without a read.
__device__ __forceinline__ float2 project_cell_open(float2 u, const float *q, int stride, int code, float two_dx_inv)
{
    if (!(code & kSolidFluid)) return make_float2(0.0f, 0.0f);
    const int out = (code & kOpenOutflow) ? open_sides(code) : 0;
    const SolidSpot t = solid_spot(code | out);
    return project_cell(u, t.i, t.gj, t.i_max, t.j_max, two_dx_inv, [=](int a, int b) {
        const int di = a - t.i, dj = b - t.gj;
        const int side = di < 0 ? kSolidW : di > 0 ? kSolidE : dj < 0 ? kSolidS : dj > 0 ? kSolidN : 0;
        return (side & out) ? 0.0f : q[dj * stride + di];
    });
}

// the neighbours that count in item 5's k: the present ones, and an outflow's ghost pressure of zero
__device__ __forceinline__ int open_neighbour_count(int code)
{
    return __builtin_popcount(code & kSolidAll) + ((code & kOpenOutflow) ? 1 : 0);
}

// The stencils by the TYPE of a member's codes, for the bodies that serve both (small_grid_core.h, batch_member.h): a
// uint8_t is a code byte and takes the solids' functions, a uint16_t an open code.
template <class Code>
__device__ __forceinline__ float divergence_sum_coded(const float2 *q, int stride, int code)
{
    if constexpr (sizeof(Code) == 1) return divergence_sum_solid(q, stride, code);
    else return divergence_sum_open(q, stride, code);
}
template <class Code>
__device__ __forceinline__ float2 project_cell_coded(float2 u, const float *q, int stride, int code, float two_dx_inv)
{
    if constexpr (sizeof(Code) == 1) return project_cell_solid(u, q, stride, code, two_dx_inv);
    else return project_cell_open(u, q, stride, code, two_dx_inv);
}

struct uq3 {
    uint32_t x, y, z;
};

__device__ __forceinline__ uq3 load_uq3(const uint32_t *p, size_t cell)
{
    const uint32_t *q = p + 3 * cell;
    return {q[0], q[1], q[2]};
}
__device__ __forceinline__ void store_uq3(uint32_t *p, size_t cell, const uq3 &r)
{
    uint32_t *q = p + 3 * cell;
    q[0] = r.x;
    q[1] = r.y;
    q[2] = r.z;
}

__device__ __forceinline__ uint32_t uq_mix(float t, uint32_t a, uint32_t b)
{
    return uq_narrow(mix1(t, uq_widen(a), uq_widen(b)));
}
// one dye channel of an in-domain sample: widen, mix, narrow once
__device__ __forceinline__ uint32_t uq_mix4(const SrcPos &s, uint32_t p11, uint32_t p12, uint32_t p21,
                                            uint32_t p22)
{
    return uq_narrow(mix4(s, uq_widen(p11), uq_widen(p12), uq_widen(p21), uq_widen(p22)));
}

// sample() of a Vector3<UQ32> field from its array in memory (advect.h:37-72 + uq32.h)
template <bool NO_SLIP>
__device__ __forceinline__ uq3 sample_global_uq3(const uint32_t *p, const Slab &gs, const SrcPos &s, float si,
                                                 float sj)
{
    const size_t t = lcell(gs, s.ci, s.cj);
    uq3 r;
    if (!s.x_oob && !s.y_oob) {
        const uq3 p11 = load_uq3(p, t), p12 = load_uq3(p, t + gs.dim_x);
        const uq3 p21 = load_uq3(p, t + 1), p22 = load_uq3(p, t + gs.dim_x + 1);
        r = {uq_mix4(s, p11.x, p12.x, p21.x, p22.x), uq_mix4(s, p11.y, p12.y, p21.y, p22.y),
             uq_mix4(s, p11.z, p12.z, p21.z, p22.z)};
    } else {
        // "T p_edge" narrows once (advect.h:45-54); returned raw when !no_slip (:57-59)
        if (s.x_oob && s.y_oob) {
            r = load_uq3(p, t);
        } else if (s.x_oob) {
            const uq3 a = load_uq3(p, t), b = load_uq3(p, t + gs.dim_x);
            r = {uq_mix(s.dj, a.x, b.x), uq_mix(s.dj, a.y, b.y), uq_mix(s.dj, a.z, b.z)};
        } else {
            const uq3 a = load_uq3(p, t), b = load_uq3(p, t + 1);
            r = {uq_mix(s.di, a.x, b.x), uq_mix(s.di, a.y, b.y), uq_mix(s.di, a.z, b.z)};
        }
        if (NO_SLIP) {  // widen, scale, narrow again (advect.h:71)
            const float f = wall_discount(s, si, sj, gs.dim_x, gs.gdim_y);
            r.x = uq_narrow(uq_widen(r.x) * f);
            r.y = uq_narrow(uq_widen(r.y) * f);
            r.z = uq_narrow(uq_widen(r.z) * f);
        }
    }
    return r;
}

// a runtime bool as a template argument of a launch: go(std::true_type{}) or go(std::false_type{})
template <class F>
inline void with_bool(bool b, F go)
{
    if (b) go(std::true_type{});
    else go(std::false_type{});
}

}  // namespace advect_math
}  // namespace sfl
