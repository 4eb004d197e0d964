// diffuse_tile.h -- the implicit diffusion of the velocity (include/sfl.h "VISCOSITY", item 3a of a step): the update,
// written ONCE for every user -- the batch members' kernels (batch_viscous.hip), the contexts' tile below
// (context_viscous.hip) and a host program that runs the tile (tests/cpp/viscosity_driver.cpp) --, the coefficients as the
// host forms them, and the core of the contexts' kernel: red-black sweeps on a field of two floats per cell of any size,
// blocked in time over an LDS window exactly as sor_solid_tile.h blocks the masked solve.  Plain C++ between SFL_HD, no
// builtin, no barrier: the caller places the barriers (the kernel) or runs the threads of a phase one after the other
// (the host).
//
// THE TILE.  A workgroup owns kTX x kTY cells at (x0, y0) and works on the WINDOW of kWX x kWY cells that reaches
// 2 * kD cells further on every side.  It loads the window's velocity into LDS, runs k <= kD sweeps -- 2k colour
// half-sweeps -- there and stores its owned cells to another buffer.  An update is a deterministic function of the
// cell's own value, its u0 and its four neighbours', so a window cell is exact after half-sweep h when the cells it
// has read were: the ring of cells on the window's edge is never updated and is exact for h = 0 only, the ring inside
// it up to h = 1, and so on.  The owned cells are 2 * kD from the edge and 2k <= 2 * kD: they leave with the bits a
// sweep over the whole grid gives them.
//
// THE ONLY BOUNDARY FACTS are "inside the domain" and the cell's fluid bit (bit 4 of its code byte, solids.cpp; `codes`
// is null without solids: every cell is fluid).  A window cell outside the domain, on the window's edge ring, or solid
// is never updated.  An updated cell reads a neighbour only where it is inside the domain -- a solid one as it is --;
// a neighbour outside contributes the cell's own value negated, which needs no read.  A cell's colour is (i + j) & 1
// of domain coordinates; the window's origin is even in both, so it is (wi + wj) & 1 of window coordinates as well.
//
// LDS holds u alone, two floats per cell, the two colours apart: cell (wi, wj) lives at colour * kPerColour + wj * kHalf
// + (wi >> 1), so that every access of a half-sweep is unit-stride (sor_solid_tile.h has the reasoning).  What else a
// thread needs of its cells -- u0 and which neighbours are inside -- stays in its registers between the half-sweeps
// (Cells); the value itself is read back from LDS, which saves the registers that two workgroups per CU need.  More than
// kD sweeps are ceil(sweeps / kD) launches: u0 is read again by each of them from the buffer it was left in, which no
// launch writes.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the header's order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SFL_HD
#define SFL_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef SFL_HD
#define SFL_HD inline
#endif
#endif

namespace sfl {
namespace diffuse {

// ---- the update, once ----------------------------------------------------------------------------------------------------
constexpr int kInW = 1, kInE = 2, kInS = 4, kInN = 8, kUpdate = 16;   // a neighbour is inside the domain; the cell is updated

// one component: u = (u0 + a * (((W + E) + S) + N)) * c
SFL_HD float diffused(float u0, float a, float c, float w, float e, float s, float n)
{
    const float sum = ((w + e) + s) + n;
    return (u0 + a * sum) * c;
}

// both components of one cell.  V: two floats x, y (float2, Vec2).  `inside`: the kIn* bits; a neighbour outside the
// domain contributes the cell's own component as it stands, negated (its argument is not looked at).
template <class V>
SFL_HD V diffused_cell(V u0, V own, float a, float c, int inside, V w, V e, V s, V n)
{
    V ghost = own;
    ghost.x = -own.x;
    ghost.y = -own.y;
    if (!(inside & kInW)) w = ghost;
    if (!(inside & kInE)) e = ghost;
    if (!(inside & kInS)) s = ghost;
    if (!(inside & kInN)) n = ghost;
    V u = own;
    u.x = diffused(u0.x, a, c, w.x, e.x, s.x, n.x);
    u.y = diffused(u0.y, a, c, w.y, e.y, s.y, n.y);
    return u;
}

// the kIn* bits of cell (i, j) of a dim_x x dim_y domain
SFL_HD int inside_bits(int i, int j, int dim_x, int dim_y)
{
    return (i > 0 ? kInW : 0) | (i < dim_x - 1 ? kInE : 0) | (j > 0 ? kInS : 0) | (j < dim_y - 1 ? kInN : 0);
}

// a = (nu * dt) / (dx * dx), c = 1.0f / (1.0f + 4.0f * a): float32, every operation rounded on its own (host)
struct Coefficients {
    float a, c;
};
inline Coefficients coefficients(float nu, float dt, float dx)
{
    Coefficients k;
    const float nu_dt = nu * dt, dx2 = dx * dx;
    k.a = nu_dt / dx2;
    const float four_a = 4.0f * k.a;
    k.c = 1.0f / (1.0f + four_a);
    return k;
}

// ---- the tile of a context -----------------------------------------------------------------------------------------------
// The shape is the masked solve's (DESIGN.md 4.13 has the timings): tests/test_viscosity.py reads these three with a regular expression
constexpr int kTX = 64;
constexpr int kTY = 32;
constexpr int kD = 8;
constexpr int kThreads = 1024;

constexpr int kHalo = 2 * kD;                        // window cells beyond the tile on every side
constexpr int kWX = kTX + 2 * kHalo, kWY = kTY + 2 * kHalo;
constexpr int kHalf = kWX / 2;                       // cells of one colour in a window row
constexpr int kPerColour = kWY * kHalf;              // ... in the window
constexpr int kSlots = (kPerColour + kThreads - 1) / kThreads;   // cells of one colour a thread owns at most
constexpr int kLdsCells = 2 * kPerColour;            // of two floats each
static_assert(kTX % 2 == 0 && kTY % 2 == 0, "the window's origin must be even in x and y: a cell's colour is (wi + wj) & 1");
static_assert(kTX <= 128 && kTY <= 64, "the test shapes span several ragged tiles");

struct alignas(8) Vec2 {
    float x, y;
};

// one launch's work on one tile
struct Tile {
    const Vec2 *u_in;       // the velocity the sweeps start from
    const Vec2 *u0;         // what items 1 to 3 left (the first launch: u_in itself)
    Vec2 *u_out;            // the owned cells' result; aliases neither
    const uint8_t *codes;   // one code byte per cell; null: no solids
    int dim_x, dim_y;
    int x0, y0;             // the tile's first cell
    int k;                  // sweeps of this launch, 1 .. kD
    float a, c;
    bool zero_solids;       // inside a step (item 3): a solid cell's velocity is read as (0, 0), and stored so where owned
};

// what a thread keeps of its cells between the half-sweeps (registers once the loops over the slots are unrolled)
struct Cells {
    Vec2 u0[2][kSlots];
    int bits[2][kSlots];    // kUpdate | kIn*; 0: no cell, outside the domain, on the window's edge ring, or solid -- never updated
};

// slot (colour, s) of thread tid: its position in the colour's array and the window cell there
struct Spot {
    int q, wi, wj;
    bool have;
};
SFL_HD Spot spot_of(int tid, int colour, int s)
{
    Spot t;
    t.q = tid + s * kThreads;
    t.have = t.q < kPerColour;
    t.wj = t.q / kHalf;
    t.wi = 2 * (t.q - t.wj * kHalf) + ((t.wj + colour) & 1);
    return t;
}

// PHASE 1: the thread's cells from memory into its registers and their velocity into LDS.  (A barrier behind it.)
SFL_HD void load(Cells &c, Vec2 *lds, const Tile &t, int tid)
{
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const Spot o = spot_of(tid, colour, s);
            const int gx = t.x0 - kHalo + o.wi, gy = t.y0 - kHalo + o.wj;
            const bool inside = o.have && gx >= 0 && gx < t.dim_x && gy >= 0 && gy < t.dim_y;
            const bool ring = o.wi == 0 || o.wi == kWX - 1 || o.wj == 0 || o.wj == kWY - 1;
            const size_t g = inside ? (size_t)gy * (size_t)t.dim_x + (size_t)gx : 0;
            const bool fluid = inside && (!t.codes || (t.codes[g] & 16));
            const bool update = fluid && !ring;
            Vec2 own, first;   // (loaded under a branch, member by member: a `cond ? memory : constant` of the struct goes through a stack slot)
            own.x = own.y = first.x = first.y = 0.0f;
            if (inside && (fluid || !t.zero_solids)) {
                const Vec2 r = t.u_in[g];
                own.x = r.x;
                own.y = r.y;
            }
            if (update) {
                const Vec2 r = t.u0[g];
                first.x = r.x;
                first.y = r.y;
            }
            c.u0[colour][s] = first;
            c.bits[colour][s] = update ? (kUpdate | inside_bits(gx, gy, t.dim_x, t.dim_y)) : 0;
            if (o.have) lds[colour * kPerColour + o.q] = own;
        }
}

// PHASE 2, 2k times: one colour's half-sweep -- reads the other colour's array, writes this one's.  (A barrier behind each.)
SFL_HD void half_sweep(Cells &c, Vec2 *lds, int colour, const Tile &t, int tid)
{
    const Vec2 *other = lds + (1 - colour) * kPerColour;
    Vec2 *mine = lds + colour * kPerColour;
    Vec2 own[kSlots], w[kSlots], e[kSlots], s_[kSlots], n[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {   // all reads of the thread's cells go out together: the cell itself and its neighbours
        const int q = tid + s * kThreads, bits = c.bits[colour][s];
        const int wj = q / kHalf;
        const int odd = (wj + colour) & 1;           // wi is odd: W is word q of the other array, E word q + 1; even: q - 1 and q
        const Vec2 zero = {0.0f, 0.0f};              // (what an absent neighbour's slot holds is not looked at)
        own[s] = bits ? mine[q] : zero;
        w[s] = (bits & kInW) ? other[q - 1 + odd] : zero;
        e[s] = (bits & kInE) ? other[q + odd] : zero;
        s_[s] = (bits & kInS) ? other[q - kHalf] : zero;
        n[s] = (bits & kInN) ? other[q + kHalf] : zero;
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int q = tid + s * kThreads, bits = c.bits[colour][s];
        const Vec2 fresh = diffused_cell(c.u0[colour][s], own[s], t.a, t.c, bits, w[s], e[s], s_[s], n[s]);
        if (bits) mine[q] = fresh;
    }
}

// PHASE 3: the owned cells inside the domain from LDS to the other buffer -- solid cells too, with the value they were read with
SFL_HD void store(const Vec2 *lds, const Tile &t, int tid)
{
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const Spot o = spot_of(tid, colour, s);
            const int gx = t.x0 - kHalo + o.wi, gy = t.y0 - kHalo + o.wj;
            const bool owned = o.have && o.wi >= kHalo && o.wi < kHalo + kTX && o.wj >= kHalo && o.wj < kHalo + kTY && gx < t.dim_x && gy < t.dim_y;
            if (owned) t.u_out[(size_t)gy * (size_t)t.dim_x + (size_t)gx] = lds[colour * kPerColour + o.q];
        }
}

// ---- the launch segmentation of a diffusion (host) -------------------------------------------------------------------
// `sweeps` sweeps take ceil(sweeps / kD) launches of kD sweeps each, the last one of what is left
inline int launches_of(int sweeps) { return (sweeps + kD - 1) / kD; }
inline int sweeps_of_launch(int sweeps, int launch) { return sweeps - launch * kD < kD ? sweeps - launch * kD : kD; }
inline int tiles_x(int dim_x) { return (dim_x + kTX - 1) / kTX; }
inline int tiles_y(int dim_y) { return (dim_y + kTY - 1) / kTY; }

}  // namespace diffuse
}  // namespace sfl
