// small_grid_core.h -- the device code of the one-workgroup kernels, shared by small_grid.hip (one grid per launch) and
// batch_grid.hip (one grid per workgroup, many grids per launch): the whole step or the whole pressure solve of a grid of
// at most kSmallGridMaxCells cells with its velocity, divergence and pressure in the workgroup's LDS.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the
// reference's order.  Reference citations are file:line under /root/reference/ESP32-fluid-simulation/.
// Offsets inside one grid are 32-bit ints (at most 6144 cells); a caller that places grids side by side
// passes each grid's base pointers, computed in 64-bit.
#pragma once
#include "advect_math.h"
#include "kernels.h"

namespace sfl {
namespace small_core {

using namespace advect_math;

// cells of one colour a thread may own (registers): a grid qualifies when its rows x ceil(dim_x / 2) positions of
// one colour fit (small_grid_fits; only widths of 3 .. 7 cells with thousands of rows do not)
template <int kThreads>
constexpr int cells_per_colour() { return kSmallGridMaxCells / 2 / kThreads; }

struct Lds {
    float2 *v;   // advected (then projected) velocity
    float *d;    // divergence
    float *p;    // pressure
};

__device__ __forceinline__ Lds carve(char *base, int cells)
{
    Lds l;
    l.v = reinterpret_cast<float2 *>(base);
    l.d = reinterpret_cast<float *>(base + (size_t)cells * 8);
    l.p = l.d + cells;
    return l;
}

// iters x two colour passes of poisson.cpp:14-112 on p (zero-filled here, :117-119) in LDS.
// A thread owns the same cells in every pass: their pressure, dx * d, -1/n and the boundary facts stay in
// registers; LDS holds p for the neighbours.  A pass is branch-free: all neighbour reads of the thread's cells go
// out together, and both reference formulas are evaluated as (((z + W) + E) + S) + N -- an absent neighbour
// contributes -0.0f, the additive identity, z = -0.0f inside and +0.0f on the perimeter (the fused kernel's
// formulation, sor_stream_core.h): interior ((W + E) + S) + N  (pois_sor_fast, :107-109), perimeter the running
// sum from 0 over the neighbours present (pois_gs_safe, :67-89).
template <int kThreads>
__device__ __forceinline__ void sor_in_lds(float *p, const float *d, int dim_x, int dim_y, int iters, SorParams prm)
{
    constexpr int kCellsPerColour = cells_per_colour<kThreads>();
    const int cells = dim_x * dim_y, half = (dim_x + 1) / 2;
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    for (int c = threadIdx.x; c < cells; c += kThreads) p[c] = 0.0f;
    __syncthreads();   // (also: d is complete)
    const int per_colour = dim_y * half;                              // positions of one colour, row-major
    const int kmax = (per_colour + kThreads - 1) / kThreads;          // block-uniform, <= kCellsPerColour
    int cm[2][kCellsPerColour];      // cell index | neighbour mask << 16 (bit 0 W, 1 E, 2 S, 3 N present; bit 4: cell exists)
    float own[2][kCellsPerColour], rhs[2][kCellsPerColour], kf[2][kCellsPerColour], z[2][kCellsPerColour];
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            const int q = threadIdx.x + k * kThreads;
            const int gj = q / half, ii = q - gj * half;
            const int i = 2 * ii + ((gj + colour) & 1);
            const bool have = k < kmax && gj < dim_y && i < dim_x;
            const int c = have ? gj * dim_x + i : 0;
            const int m = (i > 0 ? 1 : 0) | (i < i_max ? 2 : 0) | (gj > 0 ? 4 : 0) | (gj < j_max ? 8 : 0);
            const int present = __builtin_popcount(m);
            cm[colour][k] = have ? (c | ((m | 16) << 16)) : 0;
            own[colour][k] = 0.0f;
            rhs[colour][k] = have ? prm.dx * d[c] : 0.0f;   // dx * d, :108 / :88 (the same product every pass)
            kf[colour][k] = (present == 2) ? (float)(-1.0 / 2.0) : (present == 3) ? (float)(-1.0 / 3.0) : -0.25f;  // :67
            z[colour][k] = (present == 4) ? -0.0f : 0.0f;
        }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int colour = 0; colour < 2; ++colour) {  // colour 0 = even (i + j) first, poisson.cpp:22,57-60
            float w[kCellsPerColour], e[kCellsPerColour], s[kCellsPerColour], n[kCellsPerColour];
#pragma unroll
            for (int k = 0; k < kCellsPerColour; ++k) {
                if (k >= kmax) break;
                const int c = cm[colour][k] & 0xffff, m = cm[colour][k] >> 16;
                w[k] = (m & 1) ? p[c - 1] : -0.0f;
                e[k] = (m & 2) ? p[c + 1] : -0.0f;
                s[k] = (m & 4) ? p[c - dim_x] : -0.0f;
                n[k] = (m & 8) ? p[c + dim_x] : -0.0f;
            }
#pragma unroll
            for (int k = 0; k < kCellsPerColour; ++k) {
                if (k >= kmax) break;
                const float sum = (((z[colour][k] + w[k]) + e[k]) + s[k]) + n[k];
                const float p_gs = kf[colour][k] * (rhs[colour][k] - sum);
                const float fresh = prm.one_minus_omega * own[colour][k] + prm.omega * p_gs;  // :98, :111
                own[colour][k] = fresh;
                if (cm[colour][k] >> 20) p[cm[colour][k] & 0xffff] = fresh;
            }
            __syncthreads();
        }
    }
}

// ---- sor_in_lds that stops at a tolerance (include/sfl.h sfl_member_stop) -------------------------------------------
// The registers of sor_in_lds as a record, its set-up and its iteration as functions, for sor_until_in_lds below.  The
// same ownership of cells, the same pass and the same expressions, written a second time: sor_in_lds itself keeps its
// text, because built from these pieces it compiles to other instructions (the arithmetic is the same either way), and
// the kernels that exist keep theirs.
template <int kThreads>
struct SorCells {
    static constexpr int kCellsPerColour = cells_per_colour<kThreads>();
    int kmax;                        // cells of one colour this workgroup's threads own at most: block-uniform, <= kCellsPerColour
    int cm[2][kCellsPerColour];      // cell index | neighbour mask << 16 (bit 0 W, 1 E, 2 S, 3 N present; bit 4: cell exists)
    float own[2][kCellsPerColour], rhs[2][kCellsPerColour], kf[2][kCellsPerColour], z[2][kCellsPerColour];
};

// the thread's cells of both colours on p = 0; d is complete in LDS (behind a barrier)
template <int kThreads>
__device__ __forceinline__ void sor_cells_init(SorCells<kThreads> &t, const float *d, int dim_x, int dim_y, float dx)
{
    constexpr int kCellsPerColour = SorCells<kThreads>::kCellsPerColour;
    const int half = (dim_x + 1) / 2;
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    const int per_colour = dim_y * half;                              // positions of one colour, row-major
    t.kmax = (per_colour + kThreads - 1) / kThreads;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            const int q = threadIdx.x + k * kThreads;
            const int gj = q / half, ii = q - gj * half;
            const int i = 2 * ii + ((gj + colour) & 1);
            const bool have = k < t.kmax && gj < dim_y && i < dim_x;
            const int c = have ? gj * dim_x + i : 0;
            const int m = (i > 0 ? 1 : 0) | (i < i_max ? 2 : 0) | (gj > 0 ? 4 : 0) | (gj < j_max ? 8 : 0);
            const int present = __builtin_popcount(m);
            t.cm[colour][k] = have ? (c | ((m | 16) << 16)) : 0;
            t.own[colour][k] = 0.0f;
            t.rhs[colour][k] = have ? dx * d[c] : 0.0f;   // dx * d, :108 / :88 (the same product every pass)
            t.kf[colour][k] = (present == 2) ? (float)(-1.0 / 2.0) : (present == 3) ? (float)(-1.0 / 3.0) : -0.25f;  // :67
            t.z[colour][k] = (present == 4) ? -0.0f : 0.0f;
        }
}

// one iteration: the two colour passes, each behind its barrier
template <int kThreads>
__device__ __forceinline__ void sor_iteration(SorCells<kThreads> &t, float *p, int dim_x, const SorParams &prm)
{
    constexpr int kCellsPerColour = SorCells<kThreads>::kCellsPerColour;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour) {  // colour 0 = even (i + j) first, poisson.cpp:22,57-60
        float w[kCellsPerColour], e[kCellsPerColour], s[kCellsPerColour], n[kCellsPerColour];
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            if (k >= t.kmax) break;
            const int c = t.cm[colour][k] & 0xffff, m = t.cm[colour][k] >> 16;
            w[k] = (m & 1) ? p[c - 1] : -0.0f;
            e[k] = (m & 2) ? p[c + 1] : -0.0f;
            s[k] = (m & 4) ? p[c - dim_x] : -0.0f;
            n[k] = (m & 8) ? p[c + dim_x] : -0.0f;
        }
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            if (k >= t.kmax) break;
            const float sum = (((t.z[colour][k] + w[k]) + e[k]) + s[k]) + n[k];
            const float p_gs = t.kf[colour][k] * (t.rhs[colour][k] - sum);
            const float fresh = prm.one_minus_omega * t.own[colour][k] + prm.omega * p_gs;  // :98, :111
            t.own[colour][k] = fresh;
            if (t.cm[colour][k] >> 20) p[t.cm[colour][k] & 0xffff] = fresh;
        }
        __syncthreads();
    }
}

// What a solve by the rule leaves: the iterations run and the update norm of the pressure they left, as bits.  Both are
// the same in every thread and wave-uniform by construction (SGPRs).
struct UntilResult {
    int iters;
    unsigned norm_bits;
};

// sor_in_lds -- the same cells, the same iteration -- with a check in front of iteration k = 0, every, 2 * every, ...
// < cap and once more at the iteration the solve ends with: the update norm u_k of the pressure as it stands, formed
// FROM THE REGISTERS OF THE SOLVE: p_gs = kf * (rhs - ((((z + W) + E) + S) + N)) with the neighbours of both colours
// read from LDS (nothing is updated in between), |p_gs - own| as unsigned bits -- own is the bit pattern the thread
// stored into p[c], rhs the product dx * d[c] of update_norm_in_lds (below): term for term that walk's
// arithmetic, without its reads of d and its index derivation.  One cell at a time, not a colour's cells together as a
// pass reads them: what a check keeps in flight comes on top of everything the iteration loop keeps in registers, and
// the budget is 64 (profiles/batch_until.txt has the forms tried).  The maximum: wave by __shfl_xor, then one LDS
// atomicMax per wave (a maximum over bit patterns does not depend on the order; any NaN wins).
// The solve stops at the first checkpoint with u_k <= tol or u_k a NaN, given tol >= 0 (a negative tol stops nothing,
// a NaN included: the member runs to its cap as under sor_in_lds), else at k = cap.  The verdict is read back by
// every thread behind a barrier and made wave-uniform by readfirstlane, so the loop, its branches and its barriers stay
// scalar-controlled.  Two LDS words used alternately: check n accumulates into word n & 1 while thread 0 clears the other
// one, which every thread has finished reading at check n - 1 before it passed the barriers of the iteration in
// between -- no third barrier.  The last check is the report: no walk afterwards.
template <int kThreads>
__device__ __forceinline__ UntilResult sor_until_in_lds(float *p, const float *d, int dim_x, int dim_y, int cap,
                                                        SorParams prm, float tol, int every)
{
    constexpr int kCellsPerColour = SorCells<kThreads>::kCellsPerColour;
    __shared__ unsigned worst[2];
    const int cells = dim_x * dim_y;
    for (int c = threadIdx.x; c < cells; c += kThreads) p[c] = 0.0f;
    if (threadIdx.x == 0) worst[0] = 0u;
    __syncthreads();   // (also: d is complete)
    SorCells<kThreads> t;
    sor_cells_init(t, d, dim_x, dim_y, prm.dx);
    UntilResult r{0, 0u};
    int next_check = 0, word = 0;
    for (;;) {
        if (r.iters == next_check || r.iters >= cap) {   // scalar: a checkpoint, or the end
            unsigned mx = 0u;
#pragma unroll
            for (int colour = 0; colour < 2; ++colour)
#pragma unroll
                for (int k = 0; k < kCellsPerColour; ++k) {
                    if (k >= t.kmax) break;
                    const int c = t.cm[colour][k] & 0xffff, m = t.cm[colour][k] >> 16;
                    const float w = (m & 1) ? p[c - 1] : -0.0f;
                    const float e = (m & 2) ? p[c + 1] : -0.0f;
                    const float s = (m & 4) ? p[c - dim_x] : -0.0f;
                    const float n = (m & 8) ? p[c + dim_x] : -0.0f;
                    const float sum = (((t.z[colour][k] + w) + e) + s) + n;
                    const float p_gs = t.kf[colour][k] * (t.rhs[colour][k] - sum);
                    const unsigned bits = __float_as_uint(p_gs - t.own[colour][k]) & 0x7fffffffu;   // |p_gs - p|
                    if (m >> 4) mx = bits > mx ? bits : mx;   // (a position without a cell has no say)
                }
            for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
                const unsigned u = __shfl_xor(mx, o);
                mx = u > mx ? u : mx;
            }
            if ((threadIdx.x & 63) == 0) atomicMax(&worst[word], mx);
            if (threadIdx.x == 0) worst[word ^ 1] = 0u;   // for the next check (see above)
            __syncthreads();
            r.norm_bits = __builtin_amdgcn_readfirstlane(worst[word]);
            word ^= 1;
            const float u = __uint_as_float(r.norm_bits);
            if (r.iters >= cap || (tol >= 0.0f && !(u > tol))) break;   // !(u > tol): u <= tol, or u is a NaN
            next_check += every;
        }
        sor_iteration(t, p, dim_x, prm);
        ++r.iters;
    }
    return r;
}

// ---- `iters` MORE iterations on the pressure p holds (include/sfl.h sfl_poisson_continue) -------------------------------
// sor_in_lds without its zero fill: the same ownership of cells, the same iteration (sor_iteration), the thread's
// registers started from the pressure in LDS instead of zero -- own is the bit pattern p[c] holds, which is what the
// iterations before left there.  p and d are complete in LDS behind a barrier of the caller's; a cell is read here and
// written later by its owner alone.
template <int kThreads>
__device__ __forceinline__ void sor_warm_in_lds(float *p, const float *d, int dim_x, int dim_y, int iters, SorParams prm)
{
    constexpr int kCellsPerColour = SorCells<kThreads>::kCellsPerColour;
    SorCells<kThreads> t;
    sor_cells_init(t, d, dim_x, dim_y, prm.dx);
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k)
            if (t.cm[colour][k] >> 20) t.own[colour][k] = p[t.cm[colour][k] & 0xffff];
    for (int it = 0; it < iters; ++it) sor_iteration(t, p, dim_x, prm);
}

// ---- the update norm of one member: max over all cells of |p_gs(c) - p(c)| on the pressure as it stands ------------
// (what the *_each kernels of batch_grid.hip and batch_play.hip end with)
// p_gs is the value a plain Gauss-Seidel update would put into the cell, in the algebra of sor_in_lds: (((z + W) + E)
// + S) + N with -0.0f for an absent neighbour, z = -0.0f inside and +0.0f on the perimeter, k = -1/2, -1/3, -1/4
// (poisson.cpp:67-89, :107-109).  Nothing is updated: both colours are read from the same p.  The maximum is taken over
// the bit patterns of |p_gs - p| as unsigned integers, which orders finite values and +inf as floats do and lets any NaN
// win: a diverged member reports a NaN, never a finite number.  A maximum does not depend on the order of reduction.
// p and d are only read, so no barrier is needed in front as long as the caller's last writes to them are behind one;
// `worst` is LDS of its own (static, 4 B), touched by nothing else.  One plain store by thread 0.
template <int kT>
__device__ __forceinline__ void update_norm_in_lds(const float *p, const float *d, int dim_x, int dim_y, float dx, float *out)
{
    __shared__ unsigned worst;
    if (threadIdx.x == 0) worst = 0u;
    const int cells = dim_x * dim_y, i_max = dim_x - 1, j_max = dim_y - 1;
    unsigned m = 0u;
    // (gj, i) of the thread's cells by stepping, one division per thread instead of one per cell: the pass costs about
    // what the divisions cost (profiles/batch_params.txt)
    const int step_j = kT / dim_x, step_i = kT - step_j * dim_x;   // workgroup-uniform
    int gj = (int)threadIdx.x / dim_x, i = (int)threadIdx.x - gj * dim_x;
    for (int c = threadIdx.x; c < cells; c += kT, gj += step_j, i += step_i) {
        if (i >= dim_x) {
            i -= dim_x;
            ++gj;
        }
        const int present = (i > 0) + (i < i_max) + (gj > 0) + (gj < j_max);
        const float w = (i > 0) ? p[c - 1] : -0.0f;
        const float e = (i < i_max) ? p[c + 1] : -0.0f;
        const float s = (gj > 0) ? p[c - dim_x] : -0.0f;
        const float n = (gj < j_max) ? p[c + dim_x] : -0.0f;
        const float z = (present == 4) ? -0.0f : 0.0f;
        const float kf = (present == 2) ? (float)(-1.0 / 2.0) : (present == 3) ? (float)(-1.0 / 3.0) : -0.25f;
        const float sum = (((z + w) + e) + s) + n;
        const float p_gs = kf * (dx * d[c] - sum);
        const unsigned bits = __float_as_uint(p_gs - p[c]) & 0x7fffffffu;   // |p_gs - p|
        m = bits > m ? bits : m;
    }
    for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    __syncthreads();   // worst = 0 is visible
    if ((threadIdx.x & 63) == 0) atomicMax(&worst, m);
    __syncthreads();
    if (threadIdx.x == 0) *out = __uint_as_float(worst);
}

// ---- members whose cells carry CODES: solid cells inside the grid, openings on its rim -------------------------------
// (include/sfl.h "SOLIDS" and "OPENINGS"; batch_member.h has the kernels' bodies)
// ONE text for both kinds of code, over the element type (advect_math.h): a uint8_t is the solids' code byte -- bits 0..3
// neighbour present, bit 4 the cell is fluid, a solid cell's byte 0 -- and a uint16_t an open code, that byte with the
// opening in bits 8..12.  Read as a byte, bits 8..12 are known to be clear, and what asks for them folds away: the byte
// instantiation is the solids' rule and nothing more.
//
// The k of item 5 from n = the neighbours that count (open_neighbour_count: the present ones, plus one for an outflow's
// ghost pressure of zero).  Beyond the reference's table: -1.0f for one, 0.0f for none (a fluid cell walled in on all sides).
__device__ __forceinline__ float coded_k_factor(int n)
{
    return (n == 4) ? -0.25f : (n == 3) ? (float)(-1.0 / 3.0) : (n == 2) ? (float)(-1.0 / 2.0) : (n == 1) ? -1.0f : 0.0f;
}

// sor_cells_init with the boundary facts read from the member's codes instead of derived from (i, j): a solid or an open
// neighbour is one more reason for a neighbour to be absent -- the loop reads -0.0f for it and z is +0.0f, as for a wall.
// The low byte of a fluid cell's code IS the (m | 16) that sor_cells_init packs into cm; a solid cell gets cm = 0 like a
// position without a cell -- its existence bit is clear, so sor_iteration never stores it and p keeps the zero of the
// fill; no fluid cell has a neighbour bit that points at it, so it is never read either.
// `codes` is memory (one load per owned cell, here and nowhere in the loop): sor_iteration runs as it stands.
template <int kThreads, class Code>
__device__ __forceinline__ void sor_cells_init_coded(SorCells<kThreads> &t, const float *d, const Code *codes, int dim_x, int dim_y,
                                                     float dx)
{
    constexpr int kCellsPerColour = SorCells<kThreads>::kCellsPerColour;
    const int half = (dim_x + 1) / 2;
    const int per_colour = dim_y * half;                              // positions of one colour, row-major
    t.kmax = (per_colour + kThreads - 1) / kThreads;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            const int q = threadIdx.x + k * kThreads;
            const int gj = q / half, ii = q - gj * half;
            const int i = 2 * ii + ((gj + colour) & 1);
            const bool have = k < t.kmax && gj < dim_y && i < dim_x;
            const int c = have ? gj * dim_x + i : 0;
            const int code = have ? (int)codes[c] : 0;
            const bool fluid = (code & kSolidFluid) != 0;
            const int present = __builtin_popcount(code & kSolidAll);
            t.cm[colour][k] = fluid ? (c | ((code & 0xff) << 16)) : 0;
            t.own[colour][k] = 0.0f;
            t.rhs[colour][k] = fluid ? dx * d[c] : 0.0f;
            t.kf[colour][k] = coded_k_factor(open_neighbour_count(code));
            t.z[colour][k] = (present == 4) ? -0.0f : 0.0f;
        }
}

// sor_in_lds over a member with codes: the zero fill, the set-up above, the iterations of sor_iteration
template <int kThreads, class Code>
__device__ __forceinline__ void sor_coded_in_lds(float *p, const float *d, const Code *codes, int dim_x, int dim_y, int iters,
                                                 SorParams prm)
{
    const int cells = dim_x * dim_y;
    for (int c = threadIdx.x; c < cells; c += kThreads) p[c] = 0.0f;
    __syncthreads();   // (also: d is complete)
    SorCells<kThreads> t;
    sor_cells_init_coded(t, d, codes, dim_x, dim_y, prm.dx);
    for (int it = 0; it < iters; ++it) sor_iteration(t, p, dim_x, prm);
}

// update_norm_in_lds over the FLUID cells of a member with codes: `present`, which neighbours are read and k -- the
// solve's -- come from the code; a solid cell has no say, and a member without a fluid cell reports 0.0f.  The same
// reduction, the same barriers.
template <int kT, class Code>
__device__ __forceinline__ void update_norm_coded_in_lds(const float *p, const float *d, const Code *codes, int dim_x, int dim_y,
                                                         float dx, float *out)
{
    __shared__ unsigned worst;
    if (threadIdx.x == 0) worst = 0u;
    const int cells = dim_x * dim_y;
    unsigned m = 0u;
    for (int c = threadIdx.x; c < cells; c += kT) {
        const int code = codes[c];
        const int present = __builtin_popcount(code & kSolidAll);
        const float w = (code & kSolidW) ? p[c - 1] : -0.0f;
        const float e = (code & kSolidE) ? p[c + 1] : -0.0f;
        const float s = (code & kSolidS) ? p[c - dim_x] : -0.0f;
        const float n = (code & kSolidN) ? p[c + dim_x] : -0.0f;
        const float z = (present == 4) ? -0.0f : 0.0f;
        const float kf = coded_k_factor(open_neighbour_count(code));
        const float sum = (((z + w) + e) + s) + n;
        const float p_gs = kf * (dx * d[c] - sum);
        const unsigned bits = __float_as_uint(p_gs - p[c]) & 0x7fffffffu;   // |p_gs - p|
        if (code & kSolidFluid) m = bits > m ? bits : m;
    }
    for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    __syncthreads();   // worst = 0 is visible
    if ((threadIdx.x & 63) == 0) atomicMax(&worst, m);
    __syncthreads();
    if (threadIdx.x == 0) *out = __uint_as_float(worst);
}

// ---- poisson_solve (poisson.cpp:114-125) alone: d_in -> p_out of ONE grid ------------------------
template <int kThreads>
__device__ __forceinline__ void solve_in_lds(char *lds_raw, float *p_out, const float *d_in,
                                             int dim_x, int dim_y, int iters, SorParams prm)
{
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) l.d[c] = d_in[c];
    sor_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, iters, prm);   // (its first barrier also covers the copy of d)
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[c] = l.p[c];
}

// (the step itself: small_step_body.inc)

}  // namespace small_core

// more than 64 KB of dynamic LDS has to be granted once per kernel and device (host side of the launchers)
inline hipError_t allow_small_grid_lds(const void *kernel, bool *granted)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (granted[dev]) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmallGridMaxCells * 16);
    if (e == hipSuccess) granted[dev] = true;
    return e;
}

}  // namespace sfl
