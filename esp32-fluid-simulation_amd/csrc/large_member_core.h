// large_member_core.h -- the device code of the large-member batch kernels (batch_large.hip): the whole step or the whole
// pressure solve of ONE grid of at most kLargeMemberMaxCells cells by one workgroup of 1024 threads whose LDS holds 8 B
// per cell -- first the advected velocity, then, in the same bytes, the divergence and the pressure.
//
// The step never needs the three in LDS together: the advected velocity is read by a cell's NEIGHBOURS only until the
// divergence is formed; afterwards each cell's velocity is read by that cell alone (the projection), and it comes back
// from the member's own array in memory, reloaded by the thread that stored it.  The phases and the barriers between them:
//
//   A  region = float2 v[cells]   advect v_in -> v | barrier | forces (thread 0) | barrier | divergence of the thread's
//                                 cells into registers, v -> v_out, divergence -> div | BARRIER: nobody reads a velocity
//                                 neighbour any more
//   B  region = float d[cells],   d from the registers, p = 0 | barrier | red-black SOR on p (a barrier behind every
//               float p[cells]    colour pass), the update norm / the stopping rule where the call asks for them
//   C                             per cell: own velocity from v_out, v - grad p with p from LDS -> v_out, p -> memory,
//                                 the dye back-trace with the projected velocity
//
// The solve keeps per thread only the packed index and neighbour mask of its cells (ten of each colour at most); the
// cell's own pressure and dx * d come from LDS in every pass, and -1/n and the zero of the sum are derived from the mask.
// The expressions, their order and the pass order are those of small_grid_core.h's sor_in_lds: (((z + W) + E) + S) + N
// with -0.0f for an absent neighbour, z = -0.0f inside and +0.0f on the perimeter, k = -1/2, -1/3, -1/4 narrowed from
// double; dx * d formed again in every pass is the same rounded product.  The update norm and the stopping rule are
// those of include/sfl.h (sfl_batch_residual, sfl_member_stop): both colours read from the same p, the maximum over the
// bit patterns of |p_gs - p| (a NaN wins), the verdict wave-uniform.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order;
// the stencils are advect_math.h's.  Citations are file:line of the reference sketch, as in small_grid_core.h.
// Offsets inside one grid are 32-bit ints; the caller passes each grid's base pointers, computed in 64-bit.
#pragma once
#include "advect_math.h"
#include "batch.h"

namespace sfl {
namespace large_core {

using namespace advect_math;

constexpr int kThreads = 1024;
constexpr int kCellsPerThread = (kLargeMemberMaxCells + kThreads - 1) / kThreads;   // 20: thread t owns cells t, t + 1024, ...
constexpr int kCellsPerColour = kLargeMemberMaxColour / kThreads;                   // 10 positions of one colour per thread
static_assert(kCellsPerColour * kThreads == kLargeMemberMaxColour, "a colour's positions must divide among the threads");
static_assert(kLargeMemberMaxCells < 65536, "a cell index is packed into 16 bits");
static_assert(kLargeMemberMaxCells * 8 + 2048 <= 163840, "static + dynamic LDS of one workgroup: at most a CU's 160 KiB");

// how a solve ends: 0 = after `iters` iterations, nothing reported (step_n, poisson_solve); 1 = the same, then the
// update norm (*_each); 2 = by the stopping rule, the norm and the iterations run reported (*_until)
enum Mode { kUniform = 0, kEach = 1, kUntil = 2 };

// the thread's cells of both colours: cell index | neighbour mask << 16 (bit 0 W, 1 E, 2 S, 3 N present; bit 4: the cell
// exists).  Position q = thread + k * 1024 of a colour, row-major over rows of ceil(dim_x / 2) positions.
struct Cells {
    int kmax;   // positions of one colour a thread owns at most: block-uniform, <= kCellsPerColour
    int cm[2][kCellsPerColour];
};

__device__ __forceinline__ void cells_init(Cells &t, int dim_x, int dim_y)
{
    const int half = (dim_x + 1) / 2;
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    const int per_colour = dim_y * half;
    t.kmax = (per_colour + kThreads - 1) / kThreads;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            const int q = threadIdx.x + k * kThreads;
            const int gj = q / half, ii = q - gj * half;
            const int i = 2 * ii + ((gj + colour) & 1);
            const bool have = k < t.kmax && gj < dim_y && i < dim_x;
            const int c = gj * dim_x + i;
            const int m = (i > 0 ? 1 : 0) | (i < i_max ? 2 : 0) | (gj > 0 ? 4 : 0) | (gj < j_max ? 8 : 0);
            t.cm[colour][k] = have ? (c | ((m | 16) << 16)) : 0;
        }
}

// what one cell's update reads: its neighbours (-0.0f where there is none), its own pressure and dx * d (poisson.cpp:108 / :88).
// A position without a cell (record 0) reads cell 0 and is never stored.
struct Around {
    float w, e, s, n, own, rhs;
};

// (the record as the iteration loop sees it: a value the compiler cannot look through, so that what is derived from it
// -- addresses, -1/n, the zero of the sum: some hundred values per thread -- is formed again where it is used, a few
// integer operations, and not kept across the loop in registers the thread does not have.  No instruction.)
__device__ __forceinline__ int opaque(int record)
{
    asm volatile("" : "+v"(record));
    return record;
}

__device__ __forceinline__ Around gather(int record, const float *p, const float *d, int dim_x, float dx)
{
    const int c = record & 0xffff, m = record >> 16;
    Around a;
    a.w = (m & 1) ? p[c - 1] : -0.0f;
    a.e = (m & 2) ? p[c + 1] : -0.0f;
    a.s = (m & 4) ? p[c - dim_x] : -0.0f;
    a.n = (m & 8) ? p[c + dim_x] : -0.0f;
    a.own = p[c];
    a.rhs = dx * d[c];
    return a;
}

// p_gs of the cell: interior ((W + E) + S) + N (pois_sor_fast, poisson.cpp:107-109), perimeter the running sum from 0
// over the neighbours present (pois_gs_safe, :67-89), both as (((z + W) + E) + S) + N
__device__ __forceinline__ float gs_target(int record, const Around &a)
{
    const int present = __builtin_popcount((record >> 16) & 15);
    const float kf = (present == 2) ? (float)(-1.0 / 2.0) : (present == 3) ? (float)(-1.0 / 3.0) : -0.25f;   // :67
    const float z = (present == 4) ? -0.0f : 0.0f;
    const float sum = (((z + a.w) + a.e) + a.s) + a.n;
    return kf * (a.rhs - sum);
}

// one iteration: the two colour passes, each behind its barrier; colour 0 = even (i + j) first, poisson.cpp:22,57-60.
// All reads of a pass go out together; a pass writes cells of its colour only and reads, of that colour, only the
// thread's own cells.
__device__ __forceinline__ void sor_iteration(const Cells &t, float *p, const float *d, int dim_x, const SorParams &prm)
{
#pragma unroll
    for (int colour = 0; colour < 2; ++colour) {
        Around a[kCellsPerColour];
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            if (k < t.kmax) a[k] = gather(opaque(t.cm[colour][k]), p, d, dim_x, prm.dx);
        }
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            if (k < t.kmax) {
                const int record = opaque(t.cm[colour][k]);
                const float p_gs = gs_target(record, a[k]);
                const float fresh = prm.one_minus_omega * a[k].own + prm.omega * p_gs;  // :98, :111
                if (record >> 20) p[record & 0xffff] = fresh;
            }
        }
        __syncthreads();
    }
}

// the thread's share of the update norm of p as it stands: max over its cells of |p_gs - p| as unsigned bits (orders
// finite values and +inf as floats do, any NaN wins).  Reads only, one cell at a time.
__device__ __forceinline__ unsigned norm_of_own_cells(const Cells &t, const float *p, const float *d, int dim_x, float dx)
{
    unsigned mx = 0u;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            if (k < t.kmax) {
                const int record = opaque(t.cm[colour][k]);
                const Around a = gather(record, p, d, dim_x, dx);
                const unsigned bits = __float_as_uint(gs_target(record, a) - a.own) & 0x7fffffffu;   // |p_gs - p|
                if (record >> 20) mx = bits > mx ? bits : mx;   // (a position without a cell has no say)
            }
        }
    return mx;
}

// what a solve leaves besides p: the iterations run and the update norm of the pressure they left, as bits (kUniform:
// no norm).  The same in every thread and wave-uniform.
struct Solved {
    int iters;
    unsigned norm_bits;
};

// The solve on p = 0 and d, both complete in LDS once every thread has passed the barrier at the top (the caller's last
// writes to them are in front of it).
//   kUniform  `cap` iterations.
//   kEach     `cap` iterations, then the update norm.
//   kUntil    a check in front of iteration k = 0, every, 2 * every, ... < cap and once more at the iteration the solve
//             ends with; it stops at the first check with u_k <= tol or u_k a NaN, given tol >= 0, else at k = cap.
// A check: the threads' maxima by __shfl_xor within a wave, one LDS atomicMax per wave, a barrier, and every thread reads
// the word back through readfirstlane, so that the loop, its branches and its barriers stay scalar-controlled.  Two words
// used alternately: check n accumulates into word n & 1 while thread 0 clears the other one, which every thread finished
// reading at check n - 1 before it passed the barriers of the iteration in between (two checks are always at least one
// iteration apart).  The last check is the report.
template <int kMode>
__device__ __forceinline__ Solved solve_in_lds(float *p, const float *d, int dim_x, int dim_y, int cap, const SorParams &prm,
                                               float tol, int every)
{
    __shared__ unsigned worst[2];
    if (kMode != kUniform && threadIdx.x == 0) worst[0] = 0u;
    __syncthreads();
    Cells t;
    cells_init(t, dim_x, dim_y);
    Solved r{0, 0u};
    if (kMode == kUniform) {
        for (; r.iters < cap; ++r.iters) sor_iteration(t, p, d, dim_x, prm);
        return r;
    }
    int next_check = (kMode == kUntil) ? 0 : cap, word = 0;
    for (;;) {
        if (r.iters == next_check || r.iters >= cap) {   // scalar: a checkpoint, or the end
            unsigned mx = norm_of_own_cells(t, p, d, dim_x, prm.dx);
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
        sor_iteration(t, p, d, dim_x, prm);
        ++r.iters;
    }
    return r;
}

// ---- poisson_solve (poisson.cpp:114-125) alone: d_in -> p_out of ONE grid; lds = 8 B per cell ------------------------
template <int kMode>
__device__ __forceinline__ Solved solve_member(char *lds, float *p_out, const float *d_in, int dim_x, int dim_y, int cap,
                                               const SorParams &prm, float tol, int every)
{
    const int cells = dim_x * dim_y;
    float *d = reinterpret_cast<float *>(lds), *p = d + cells;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        d[c] = d_in[c];
        p[c] = 0.0f;   // :117-119
    }
    const Solved r = solve_in_lds<kMode>(p, d, dim_x, dim_y, cap, prm, tol, every);
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[c] = p[c];
    return r;
}

// ---- one whole step (ino:252-287) of ONE grid: `a` with every pointer at the grid's first cell; lds = 8 B per cell ----
template <int kMode>
__device__ __forceinline__ Solved step_member(char *lds, const SmallStep &a, float tol, int every)
{
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y;
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in);
    float2 *v_out = reinterpret_cast<float2 *>(a.v_out);

    // ---- phase A: the region is the advected velocity
    float2 *v = reinterpret_cast<float2 *>(lds);
    // advect(v_next, v, v, dt, no_slip): ino:252-256, advect.h:78-84
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float2 u = v_in[c];
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        v[c] = sample_global_vec2f<true>(v_in, g, s, si, sj);
    }
    __syncthreads();
    // drag forces, in queue order: later entries win (ino:264-269)
    if (a.n_forces > 0) {
        if (threadIdx.x == 0)
            for (int k = 0; k < a.n_forces; ++k) {
                const int i = a.force_cells[2 * k], gj = a.force_cells[2 * k + 1];
                if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                v[gj * dim_x + i] = make_float2(a.force_vel[2 * k], a.force_vel[2 * k + 1]);
            }
        __syncthreads();
    }
    // calculate_divergence (ino:274, finitediff.cpp:9-39) of the thread's cells into registers; the advected velocity
    // goes to memory for phase C, the divergence for the caller
    float dv[kCellsPerThread];
#pragma unroll
    for (int k = 0; k < kCellsPerThread; ++k) {
        const int c = threadIdx.x + k * kThreads;
        if (c < cells) {
            const int gj = c / dim_x, i = c - gj * dim_x;
            dv[k] = divergence_sum(v + c, dim_x, i, gj, i_max, j_max) * a.two_dx_inv;
            v_out[c] = v[c];
            a.div[c] = dv[k];
        }
    }
    __syncthreads();   // the last read of a velocity neighbour is behind every thread: the region changes its role

    // ---- phase B: the region is the divergence and the pressure
    float *d = reinterpret_cast<float *>(lds), *p = d + cells;
#pragma unroll
    for (int k = 0; k < kCellsPerThread; ++k) {
        const int c = threadIdx.x + k * kThreads;
        if (c < cells) {
            d[c] = dv[k];
            p[c] = 0.0f;   // poisson.cpp:117-119
        }
    }
    // poisson_solve: ino:275 (its first barrier orders the writes above)
    const Solved r = solve_in_lds<kMode>(p, d, dim_x, dim_y, a.iters, a.prm, tol, every);

    // ---- phase C: subtract_gradient (ino:276, finitediff.cpp:41-82) on the cell's own advected velocity -- stored to v_out
    // by this very thread in phase A -- then the dye back-trace with the projected velocity of the cell itself
    // (ino:281-287, advect.h:81); p is final since the solve's last barrier and only read from here on
    const uint32_t *col_in = a.col_in;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float pc = p[c];
        const float2 u = project_cell(v_out[c], p + c, dim_x, i, gj, i_max, j_max, a.two_dx_inv);
        v_out[c] = u;
        a.p[c] = pc;
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        store_uq3(a.col_out, (size_t)c, sample_global_uq3<false>(col_in, g, s, si, sj));
    }
    return r;
}

}  // namespace large_core
}  // namespace sfl
