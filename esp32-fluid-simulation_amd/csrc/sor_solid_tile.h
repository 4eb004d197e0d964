// sor_solid_tile.h -- the core of the masked pressure solve of a whole-domain context (include/sfl.h "SOLIDS OF A CONTEXT";
// context_solids.hip): red-black SOR over a grid of any size whose boundary facts are one code byte per cell, blocked in
// time over an LDS tile.  Shared, as sor_stream_core.h is, by the kernel and by a host program that runs one workgroup's
// tile thread after thread (tests/cpp/context_solids_driver.cpp): plain C++ between SFL_HD, no builtin, no barrier -- the
// caller places the barriers (the kernel) or runs the threads of a phase one after the other (the host).
//
// THE TILE.  A workgroup owns kTX x kTY cells at (x0, y0) and works on the WINDOW of kWX x kWY cells that reaches
// 2 * kD cells further on every side.  It loads the window's pressure into LDS, runs k <= kD iterations -- 2k colour
// half-sweeps -- there, and stores its owned cells to the ping-pong partner of p.  A relaxation is a deterministic
// function of the cell's own value and its four neighbours', so a window cell is exact after half-sweep h when the cells
// it has read were: the ring of cells on the window's edge is never relaxed (their neighbours are not all loaded) and is
// exact for h = 0 only, the ring inside it reads that ring's other colour and is exact up to h = 1, and so on -- after
// half-sweep h the cells at least h from the window's edge are exact.  The owned cells are 2 * kD from it and
// 2k <= 2 * kD: they leave with the bits a sweep over the whole grid gives them.
//
// WALLS ARE THE MASK.  A window cell outside the domain, and a cell of the window's edge ring, has code 0 like a solid
// cell: never relaxed, never stored.  A relaxed cell reads a neighbour only where its code byte says PRESENT, which
// implies inside the domain; a neighbour's absence contributes -0.0f.  The four presence bits are the only boundary
// logic there is.  A cell's colour is (i + j) & 1 of domain coordinates; the window's origin is even in both, so it is
// (wi + wj) & 1 of window coordinates as well.
//
// LDS holds p alone, the two colours apart: cell (wi, wj) lives at colour * kPerColour + wj * kHalf + (wi >> 1).  A
// thread's slot s of a colour is position q = tid + s * kThreads of that array, so the 64 lanes of a wave touch 64
// consecutive words for their own cells and for the S and N neighbours (q -+ kHalf of the other array), and for W and E
// words q - 1 .. q + 1 of it: every access of a half-sweep is unit-stride, which the 64 LDS banks serve without a
// conflict (where a wave crosses from one window row to the next the W / E offsets differ by one word: one bank hit twice).
// Storing the colours interleaved would make every access stride 2 -- each bank hit twice -- and padding the pitch
// does not cure that; splitting the colours does.  What else a thread needs of its cells -- the rounded dx * d, the
// code byte, the k-factor, the value itself -- stays in its registers between the half-sweeps (Cells).
//
// THE ARITHMETIC is the rule's (include/sfl.h "SOLIDS", item 5), stated here once for the solve's tile, the host's
// emulation of it and the streaming update norm of context_solids.hip: k_factor, z_term, gauss_seidel, relaxed.
// Numerics contract: -ffp-contract=off, every operation individually rounded.
#pragma once
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
namespace solid_tile {

// The shape (DESIGN.md 4.12 has the reasons): tests/test_context_solids.py reads these three with a regular expression
constexpr int kTX = 64;
constexpr int kTY = 32;
constexpr int kD = 8;
constexpr int kThreads = 1024;

constexpr int kHalo = 2 * kD;                        // window cells beyond the tile on every side
constexpr int kWX = kTX + 2 * kHalo, kWY = kTY + 2 * kHalo;
constexpr int kHalf = kWX / 2;                       // cells of one colour in a window row
constexpr int kPerColour = kWY * kHalf;              // ... in the window
constexpr int kSlots = (kPerColour + kThreads - 1) / kThreads;   // cells of one colour a thread owns at most
constexpr int kLdsFloats = 2 * kPerColour;
static_assert(kTX % 2 == 0 && kTY % 2 == 0, "the window's origin must be even in x and y: a cell's colour is (wi + wj) & 1");
static_assert(kTX <= 128 && kTY <= 64, "the test shapes span several ragged tiles");

// the code byte (advect_math.h states it for the device): bits 0..3 W, E, S, N neighbour present, bit 4 the cell is fluid
constexpr int kW = 1, kE = 2, kS = 4, kN = 8, kFluid = 16, kAll = 15;

SFL_HD int present_of(int code)
{
    return (code & 1) + ((code >> 1) & 1) + ((code >> 2) & 1) + ((code >> 3) & 1);
}
// k = -1 / present; beyond the reference's table -1.0f for one present neighbour and 0.0f for none
SFL_HD float k_factor(int present)
{
    return present == 4 ? -0.25f : present == 3 ? (float)(-1.0 / 3.0) : present == 2 ? (float)(-1.0 / 2.0) : present == 1 ? -1.0f : 0.0f;
}
// the running sum starts from -0.0f where all four neighbours are present (the reference's ((W + E) + S) + N), else from +0.0f
SFL_HD float z_term(int present) { return present == 4 ? -0.0f : 0.0f; }
// p_gs = k * (dx * d - ((((z + W) + E) + S) + N)); rhs = the rounded dx * d, an absent neighbour's value -0.0f
SFL_HD float gauss_seidel(float rhs, float kf, float z, float w, float e, float s, float n)
{
    const float sum = (((z + w) + e) + s) + n;
    return kf * (rhs - sum);
}
SFL_HD float relaxed(float own, float p_gs, float omega, float one_minus_omega) { return one_minus_omega * own + omega * p_gs; }

// one launch's work on one tile
struct Tile {
    const float *p_in;      // the pressure the iterations start from; null: zero everywhere (a solve's first launch)
    float *p_out;           // its ping-pong partner: the owned cells' result
    const float *d;
    const uint8_t *codes;
    int dim_x, dim_y;
    int x0, y0;             // the tile's first cell
    int k;                  // iterations of this launch, 1 .. kD
    float dx, omega, one_minus_omega;
};

// what a thread keeps of its cells between the half-sweeps (registers: every index below is a compile-time constant
// once the loops over the slots are unrolled)
struct Cells {
    float own[2][kSlots], rhs[2][kSlots], kf[2][kSlots];
    int code[2][kSlots];    // 0: no cell, outside the domain, on the window's edge ring, or solid -- never relaxed
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

// PHASE 1: the thread's cells from memory into its registers and their pressure into LDS.  (A barrier behind it.)
SFL_HD void load(Cells &c, float *lds, const Tile &t, int tid)
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
            const int code = inside ? (int)t.codes[g] : 0;
            const bool relax = inside && !ring && (code & kFluid);
            const int present = present_of(code);
            c.own[colour][s] = inside && t.p_in ? t.p_in[g] : 0.0f;
            c.rhs[colour][s] = relax ? t.dx * t.d[g] : 0.0f;
            c.kf[colour][s] = k_factor(present);
            c.code[colour][s] = relax ? code : 0;
            if (o.have) lds[colour * kPerColour + o.q] = c.own[colour][s];
        }
}

// PHASE 2, 2k times: one colour's half-sweep -- reads the other colour's array, writes this one's.  (A barrier behind each.)
SFL_HD void half_sweep(Cells &c, float *lds, int colour, const Tile &t, int tid)
{
    const float *other = lds + (1 - colour) * kPerColour;
    float *mine = lds + colour * kPerColour;
    float w[kSlots], e[kSlots], s_[kSlots], n[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {   // all neighbour reads of the thread's cells go out together
        const int q = tid + s * kThreads, code = c.code[colour][s];
        const int wj = q / kHalf;
        const int odd = (wj + colour) & 1;           // wi is odd: W is word q of the other array, E word q + 1; even: q - 1 and q
        w[s] = (code & kW) ? other[q - 1 + odd] : -0.0f;
        e[s] = (code & kE) ? other[q + odd] : -0.0f;
        s_[s] = (code & kS) ? other[q - kHalf] : -0.0f;
        n[s] = (code & kN) ? other[q + kHalf] : -0.0f;
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int q = tid + s * kThreads, code = c.code[colour][s];
        const float p_gs = gauss_seidel(c.rhs[colour][s], c.kf[colour][s], z_term(present_of(code)), w[s], e[s], s_[s], n[s]);
        const float fresh = relaxed(c.own[colour][s], p_gs, t.omega, t.one_minus_omega);
        if (code) {
            c.own[colour][s] = fresh;
            mine[q] = fresh;
        }
    }
}

// PHASE 3: the owned cells inside the domain to the partner -- solid cells too, with the value they came with
SFL_HD void store(const Cells &c, const Tile &t, int tid)
{
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const Spot o = spot_of(tid, colour, s);
            const int gx = t.x0 - kHalo + o.wi, gy = t.y0 - kHalo + o.wj;
            const bool owned = o.have && o.wi >= kHalo && o.wi < kHalo + kTX && o.wj >= kHalo && o.wj < kHalo + kTY && gx < t.dim_x && gy < t.dim_y;
            if (owned) t.p_out[(size_t)gy * (size_t)t.dim_x + (size_t)gx] = c.own[colour][s];
        }
}

// ---- the launch segmentation of a solve (host) -----------------------------------------------------------------------
// `iters` iterations take ceil(iters / kD) launches of kD iterations each, the last one of what is left
inline int launches_of(int iters) { return (iters + kD - 1) / kD; }
inline int iterations_of_launch(int iters, int launch) { return iters - launch * kD < kD ? iters - launch * kD : kD; }
inline int tiles_x(int dim_x) { return (dim_x + kTX - 1) / kTX; }
inline int tiles_y(int dim_y) { return (dim_y + kTY - 1) / kTY; }

}  // namespace solid_tile
}  // namespace sfl
