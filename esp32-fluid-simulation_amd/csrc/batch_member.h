// batch_member.h -- what the kernels of a batch with 16 B of LDS per cell share (gfx950 / MI355X): batch_grid.hip,
// batch_play.hip, batch_solids.hip, batch_viscous.hip and batch_openings.hip; batch_large.hip takes member_step and
// apply_member alone.  Each of those files is a list of kernels and launchers over the pieces here:
//
//   * the workgroup's shape: SFL_BATCH_THREADS, SFL_BATCH_WAVES_PER_EU, SFL_BATCH_BOUNDS, kThreads;
//   * member_step and apply_member: the SmallStep of one member, and a BatchMember record's parameters put into it;
//   * launch_members: one workgroup per member, 16 B of dynamic LDS per cell;
//   * step_in_lds: the ONE text of a member's step for every rule beyond the plain one -- codes (the solids' bytes or
//     open codes: advect_math.h, small_grid_core.h), item 3a (the viscosity) and a profile row, in any combination a
//     kernel asks for by template arguments.  A feature is a branch here, once, not a copy of the step;
//   * coded_solve_in_lds: solve_in_lds for a member with codes;
//   * velocity_stats_of and launch_coded_velocity_stats: the velocity statistics of members with codes.
//
// What keeps a text of its own, and why: the plain step is small_step_body.inc, which small_step_kernel shares and whose
// instructions must not move; step_in_lds<void> with item 3a is that step for the viscous kernels alone.  The kernels
// themselves stay in their files under their names, one object each: a parallel build, and profiles and instruction
// comparisons by object and by name.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#pragma once
#include <type_traits>

#include "batch.h"
#include "diffuse_tile.h"
#include "small_grid_core.h"
#include "stats_kernels.h"
#include "viscous_kernels.h"

// Workgroup shape and occupancy are build knobs (batch_grid.hip has the reasons, profiles/batch_throughput.txt the sweep)
#ifndef SFL_BATCH_THREADS
#define SFL_BATCH_THREADS 1024
#endif
#ifndef SFL_BATCH_WAVES_PER_EU
#define SFL_BATCH_WAVES_PER_EU 8
#endif
#if SFL_BATCH_WAVES_PER_EU > 0
#define SFL_BATCH_BOUNDS __launch_bounds__(SFL_BATCH_THREADS) __attribute__((amdgpu_waves_per_eu(SFL_BATCH_WAVES_PER_EU)))
#else
#define SFL_BATCH_BOUNDS __launch_bounds__(SFL_BATCH_THREADS)
#endif

namespace sfl {
namespace batch_member {

using namespace small_core;

constexpr int kThreads = SFL_BATCH_THREADS;
// every workgroup size must own the same cells of one colour in total as small_grid.hip's 1024 threads: the batch
// accepts exactly the shapes small_grid_fits accepts
static_assert(cells_per_colour<kThreads>() * kThreads == kSmallGridMaxCells / 2, "SFL_BATCH_THREADS must divide 3072");

// the step of one member: every pointer at that member's first cell, its force records
__device__ __forceinline__ SmallStep member_step(const BatchStep &b, size_t member)
{
    const size_t base = member * (size_t)b.step.dim_x * (size_t)b.step.dim_y;   // 64-bit: cells before this member
    SmallStep a = b.step;
    a.v_in += 2 * base;
    a.v_out += 2 * base;
    a.col_in += 3 * base;
    a.col_out += 3 * base;
    a.div += base;
    a.p += base;
    a.n_forces = 0;
    if (b.force_offsets) {   // this member's records, in queue order
        const int f0 = b.force_offsets[member], f1 = b.force_offsets[member + 1];
        a.force_cells += 2 * (size_t)f0;
        a.force_vel += 2 * (size_t)f0;
        a.n_forces = f1 - f0;
    }
    return a;
}

// the parameters of one member's record in place of the launch's (the record is read at a workgroup-uniform address:
// scalar loads; the host hands out long members first)
__device__ __forceinline__ void apply_member(SmallStep &a, const BatchMember &q)
{
    a.dt = q.dt;
    a.two_dx_inv = q.two_dx_inv;
    a.iters = q.iters;
    a.prm = q.prm;
}

// every step or solve launch: one workgroup per member, 16 B of LDS per cell, which a kernel is granted once per device
template <auto KERNEL, class... A>
hipError_t launch_members(hipStream_t s, int dim_x, int dim_y, int batch, A... args)
{
    static bool granted[64];
    const size_t lds = (size_t)dim_x * dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(KERNEL), granted);
    if (e != hipSuccess) return e;
    KERNEL<<<batch, kThreads, lds, s>>>(args...);
    return hipGetLastError();
}

// the codes of one member, BatchSolids' bytes or BatchOpenings' open codes: stride 0 = one set for all members
template <class Codes>
__device__ __forceinline__ auto member_codes(const Codes &s, size_t member) { return s.codes + member * s.member_stride; }
__device__ __forceinline__ float2 member_inflow(const BatchOpenings &o, size_t member)
{
    return make_float2(o.inflow[2 * member], o.inflow[2 * member + 1]);
}

// the row of one member in the profile's table ("INFLOW PROFILES AND FLUX"); none for a step without a profile
struct ProfileRow {
    const uint32_t *cells;
    const float2 *vel;
    int n;
};
__device__ __forceinline__ ProfileRow member_profile(const BatchProfile &t, size_t member)
{
    const int r0 = t.offsets[member], r1 = t.offsets[member + 1];   // workgroup-uniform: scalar loads
    return ProfileRow{t.cells + r0, reinterpret_cast<const float2 *>(t.vel) + r0, r1 - r0};
}

// Item 3a: `q.sweeps` sweeps on u = l.v, u0 in the 8 B per cell where d and p will live: THE DIFFUSION RUNS IN LDS WITH NO
// EXTRA BYTES.  carve() places d and p side by side behind the velocity, and both are dead until item 4.  A thread owns
// the same cells of a colour in every half-sweep (the ownership of sor_in_lds: position q = thread + k * threads of the
// colour's row-major list) and keeps their index and which neighbours are inside the domain in three registers per
// colour; a half-sweep reads the other colour's cells from l.v and writes its own -- a barrier behind each.  The update is
// diffuse_tile.h's, the one every user shares.  l.v is complete (a barrier in front).  Code, codes: as for step_in_lds below.
template <class Code>
__device__ __forceinline__ void diffuse_in_lds(const Lds &l, const Code *__restrict__ codes, int dim_x, int dim_y, BatchViscous q)
{
    constexpr int kCellsPerColour = cells_per_colour<kThreads>();
    float2 *u0 = reinterpret_cast<float2 *>(l.d);   // (d and p side by side: cells * 8 bytes, 8-byte aligned behind l.v)
    const int half = (dim_x + 1) / 2;
    const int kmax = (dim_y * half + kThreads - 1) / kThreads;   // block-uniform, <= kCellsPerColour
    int cm[2][kCellsPerColour];   // cell index | (diffuse::kUpdate | kIn*) << 16; 0: no cell there, or a solid one
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int k = 0; k < kCellsPerColour; ++k) {
            const int pos = threadIdx.x + k * kThreads;
            const int gj = pos / half, ii = pos - gj * half;
            const int i = 2 * ii + ((gj + colour) & 1);
            const bool have = k < kmax && gj < dim_y && i < dim_x;
            const int c = have ? gj * dim_x + i : 0;
            bool fluid = have;
            if constexpr (!std::is_void_v<Code>) fluid = have && (codes[c] & kSolidFluid);
            cm[colour][k] = fluid ? (c | ((diffuse::kUpdate | diffuse::inside_bits(i, gj, dim_x, dim_y)) << 16)) : 0;
            if (fluid) u0[c] = l.v[c];   // (the cell's own thread reads it back: no barrier needed for u0)
        }
    for (int it = 0; it < q.sweeps; ++it) {
#pragma unroll
        for (int colour = 0; colour < 2; ++colour) {   // colour 0 = even (i + j) first
#pragma unroll
            for (int k = 0; k < kCellsPerColour; ++k) {
                if (k >= kmax) break;
                const int c = cm[colour][k] & 0xffff, bits = cm[colour][k] >> 16;
                if (!bits) continue;
                const float2 own = l.v[c];
                const float2 w = (bits & diffuse::kInW) ? l.v[c - 1] : own;   // (an absent neighbour's slot is not looked at)
                const float2 e = (bits & diffuse::kInE) ? l.v[c + 1] : own;
                const float2 s = (bits & diffuse::kInS) ? l.v[c - dim_x] : own;
                const float2 n = (bits & diffuse::kInN) ? l.v[c + dim_x] : own;
                l.v[c] = diffuse::diffused_cell(u0[c], own, q.a, q.c, bits, w, e, s, n);
            }
            __syncthreads();
        }
    }
}

// what a kernel does not ask of step_in_lds it leaves out, or names by these where a later argument follows
constexpr BatchViscous kNoViscosity{0.0f, 0.0f, 0};
__device__ __forceinline__ float2 no_inflow() { return make_float2(0.0f, 0.0f); }

// ONE WHOLE STEP of the grid `a` describes, in the order of small_step_body.inc (the rule of include/sfl.h, items 1 - 7
// with 2a and 3a); returns the carved LDS (p and d final, for the update norm of the *_each kernels).
//   Code      the type of the member's codes at `codes`: uint8_t = code bytes (the solids' rule), uint16_t = open codes
//             (the openings' rule, `inflow` the member's), void = none (codes null; the stencils from (i, j) and
//             sor_in_lds, the plain member step).  What the bytes cannot say -- an inflow cell -- folds away for them.
//   kViscous  item 3a by `visc` between the forces and the divergence; a member with sweeps == 0 (the host stores that
//             for nu == 0 too) skips it by a workgroup-uniform branch: no bit of it changes.
//   kProfile  the records of `row` -- unique fluid inflow cells, which the force loop never writes -- go into l.v by all
//             threads behind the advection's barrier, beside the forces, and ONE barrier that every workgroup reaches
//             stands in front of the divergence instead of the forces' own.
//   kWalls    the records of `walls` (include/sfl.h "WALL VELOCITIES") -- unique SOLID cells, which neither the force loop
//             nor the profile writes -- go into l.v beside the profile's, behind the same barriers (the extended item 3:
//             only item 3a ever reads them), and into v_out behind the projection's stores with a barrier between
//             (item 8: item 6 has just stored (0, 0) there, by whichever thread owns the cell).
// Imposing the inflow and zeroing the solids happen where a cell's velocity is stored and where a force record is
// skipped: together the same as doing both after the forces, without a pass and a barrier of their own.
template <class Code, bool kViscous = false, bool kProfile = false, bool kWalls = false>
__device__ __forceinline__ Lds step_in_lds(const SmallStep &a, const Code *__restrict__ codes, char *lds_raw, float2 inflow = no_inflow(),
                                           BatchViscous visc = kNoViscosity, ProfileRow row = ProfileRow{nullptr, nullptr, 0},
                                           ProfileRow walls = ProfileRow{nullptr, nullptr, 0})
{
    constexpr bool kCoded = !std::is_void_v<Code>;
    constexpr bool kRows = kProfile || kWalls;   // a table's rows stand beside the forces: one barrier for both
    static_assert(!kProfile || kCoded, "a profile's cells are inflow cells");
    static_assert(!kWalls || kCoded, "a wall's cells are solid cells");
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in);
    float2 *v_out = reinterpret_cast<float2 *>(a.v_out);

    // advect(v_next, v, v, dt, no_slip) on every cell (item 1); an inflow cell holds the inflow (item 2a), a solid one
    // (0, 0) (item 3)
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float2 u = v_in[c];
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        const float2 r = sample_global_vec2f<true>(v_in, g, s, si, sj);
        if constexpr (kCoded) {
            const int code = codes[c];
            l.v[c] = !(code & kSolidFluid) ? make_float2(0.0f, 0.0f) : is_inflow_cell(code) ? inflow : r;
        } else {
            l.v[c] = r;
        }
    }
    __syncthreads();
    if constexpr (kProfile)   // the profile's part of item 2a
        for (int k = threadIdx.x; k < row.n; k += kThreads) l.v[row.cells[k]] = row.vel[k];
    if constexpr (kWalls)     // the walls' part of item 3
        for (int k = threadIdx.x; k < walls.n; k += kThreads) l.v[walls.cells[k]] = walls.vel[k];
    // drag forces, in queue order: later entries win; a record on a solid or an inflow cell has no effect (items 2, 2a, 3)
    if (a.n_forces > 0) {
        if (threadIdx.x == 0)
            for (int k = 0; k < a.n_forces; ++k) {
                const int i = a.force_cells[2 * k], gj = a.force_cells[2 * k + 1];
                if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                if constexpr (kCoded) {
                    const int code = codes[gj * dim_x + i];
                    if (!(code & kSolidFluid) || is_inflow_cell(code)) continue;
                }
                l.v[gj * dim_x + i] = make_float2(a.force_vel[2 * k], a.force_vel[2 * k + 1]);
            }
        if constexpr (!kRows) __syncthreads();
    }
    if constexpr (kRows) __syncthreads();   // the records and the forces are visible to the diffusion and the divergence
    // the diffusion (item 3a); skipped whole by a member without one
    if constexpr (kViscous)
        if (visc.sweeps > 0) diffuse_in_lds(l, codes, dim_x, dim_y, visc);
    // the divergence of a fluid cell; 0.0f in a solid one (item 4)
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        float dv;
        if constexpr (kCoded) {
            const int code = codes[c];
            const float sum = divergence_sum_coded<Code>(l.v + c, dim_x, code);
            dv = (code & kSolidFluid) ? sum * a.two_dx_inv : 0.0f;
        } else {
            const int gj = c / dim_x, i = c - gj * dim_x;
            dv = divergence_sum(l.v + c, dim_x, i, gj, i_max, j_max) * a.two_dx_inv;
        }
        // (with item 3a d lies where u0 lay: cell c's d is written while another thread may still read its neighbours'
        // velocity, never u0)
        l.d[c] = dv;
        a.div[c] = dv;
    }
    // the pressure (item 5; the barrier inside also orders the divergence writes above)
    if constexpr (kCoded)
        sor_coded_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, a.iters, a.prm);
    else
        sor_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, a.iters, a.prm);
    // the gradient (item 6), then the dye back-trace with the projected velocity of the cell itself (item 7)
    const uint32_t *col_in = a.col_in;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float pc = l.p[c];
        float2 u;
        if constexpr (kCoded)
            u = project_cell_coded<Code>(l.v[c], l.p + c, dim_x, codes[c], a.two_dx_inv);
        else
            u = project_cell(l.v[c], l.p + c, dim_x, i, gj, i_max, j_max, a.two_dx_inv);
        v_out[c] = u;
        a.p[c] = pc;
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        store_uq3(a.col_out, (size_t)c, sample_global_uq3<false>(col_in, g, s, si, sj));
    }
    if constexpr (kWalls) {   // item 8: the walls hold their velocity again, behind every thread's (0, 0) of item 6
        __syncthreads();
        for (int k = threadIdx.x; k < walls.n; k += kThreads) v_out[walls.cells[k]] = walls.vel[k];
    }
    return l;
}

// poisson_solve of ONE grid with codes: d_in -> p_out (solve_in_lds); returns the carved LDS as step_in_lds does
template <class Code>
__device__ __forceinline__ Lds coded_solve_in_lds(char *lds_raw, float *p_out, const float *d_in, const Code *__restrict__ codes,
                                                  int dim_x, int dim_y, int iters, SorParams prm)
{
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) l.d[c] = d_in[c];
    sor_coded_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, iters, prm);   // (its first barrier also covers the copy of d)
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[c] = l.p[c];
    return l;
}

// ---- the velocity statistics of members with codes ------------------------------------------------------------------
// max |v.x|, max |v.y| over all cells and max |divergence| by item 4 of the rule over all cells (0.0f in a solid one), as
// bit patterns into records zeroed in front (flow_stats.hip's reduction: a maximum does not depend on the order).  A
// member is at most 6144 cells: blockIdx.y is the member, the workgroups of blockIdx.x share its cells, a thread a cell
// at a time with its neighbours read from memory -- L2 at this size.  The body of the two kernels, BatchSolids' and
// BatchOpenings', that carry their names in batch_solids.hip and batch_openings.hip.
constexpr int kStatsThreads = 256;

template <class Codes>
__device__ __forceinline__ void velocity_stats_of(const float *__restrict__ v, const Codes &coded, int dim_x, int dim_y, float two_dx_inv,
                                                  const float *__restrict__ member_two_dx_inv, FlowStatsRecord *__restrict__ out)
{
    using Code = std::remove_cv_t<std::remove_pointer_t<decltype(coded.codes)>>;
    const size_t member = blockIdx.y;
    const int cells = dim_x * dim_y;
    const float2 *q = reinterpret_cast<const float2 *>(v) + member * (size_t)cells;
    const Code *codes = member_codes(coded, member);
    const float scale = member_two_dx_inv ? member_two_dx_inv[member] : two_dx_inv;
    unsigned m[3] = {0u, 0u, 0u};
    for (int c = blockIdx.x * kStatsThreads + threadIdx.x; c < cells; c += gridDim.x * kStatsThreads) {
        const int code = codes[c];
        const float2 own = q[c];
        const float sum = divergence_sum_coded<Code>(q + c, dim_x, code);
        const float dv = (code & kSolidFluid) ? sum * scale : 0.0f;
        const unsigned bx = __float_as_uint(own.x) & 0x7fffffffu, by = __float_as_uint(own.y) & 0x7fffffffu;
        const unsigned bd = __float_as_uint(dv) & 0x7fffffffu;
        m[0] = bx > m[0] ? bx : m[0];
        m[1] = by > m[1] ? by : m[1];
        m[2] = bd > m[2] ? bd : m[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
            const unsigned t = __shfl_xor(m[k], o);
            m[k] = t > m[k] ? t : m[k];
        }
    if ((threadIdx.x & 63) == 0) {
        FlowStatsRecord *rec = out + member;
        atomicMax(&rec->max_abs_vx, m[0]);
        atomicMax(&rec->max_abs_vy, m[1]);
        atomicMax(&rec->max_abs_div, m[2]);
    }
}

// its launches: gridDim.y is a 16-bit number, so 65535 members at a time, every per-member pointer moved on
template <auto KERNEL, class Codes>
hipError_t launch_coded_velocity_stats(hipStream_t s, FlowStatsRecord *out, const float *v, const Codes &coded, int dim_x, int dim_y,
                                       int members, float two_dx_inv, const float *member_two_dx_inv)
{
    const int cells = dim_x * dim_y;
    const int per_member = (cells + 4 * kStatsThreads - 1) / (4 * kStatsThreads);   // four cells per thread, at most six workgroups
    for (int first = 0; first < members; first += 65535) {
        const int count = members - first < 65535 ? members - first : 65535;
        Codes part = coded;
        part.codes += (size_t)first * coded.member_stride;
        KERNEL<<<dim3(per_member, count), kStatsThreads, 0, s>>>(v + 2 * (size_t)first * cells, part, dim_x, dim_y, two_dx_inv,
                                                                 member_two_dx_inv ? member_two_dx_inv + first : nullptr, out + first);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace batch_member
}  // namespace sfl
