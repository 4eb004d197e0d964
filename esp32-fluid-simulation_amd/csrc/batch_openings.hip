// batch_openings.hip -- batch members with openings on the rim of their grids (gfx950 / MI355X; include/sfl.h "OPENINGS"):
// the step, the pressure solve and the velocity statistics of batch_solids.hip for a batch whose members carry a map of
// inflow and outflow cells, with or without solid cells.  Kernels of their own, written a third time: those of
// batch_grid.hip and batch_solids.hip keep their text and their instructions, and a batch without openings launches exactly
// what it launched before.
//
// One OPEN CODE of 16 bits per cell, formed on the host (openings.cpp) and read from memory where batch_solids.hip reads
// its code byte: that byte in bits 0..7, which neighbour is open in bits 8..11, bit 12 = the opening is an outflow
// (advect_math.h).  An array of its own; the solids' bytes stay as they are for the kernels that read them.
//
// The step, in the order of batch_solids.hip (the rule of include/sfl.h, items 1 - 7 and 2a):
//   * advection of the velocity as it stands, on every cell; what is stored for a solid cell is (0, 0) and for a fluid
//     inflow cell the member's inflow velocity;
//   * forces in queue order, a record on a solid cell or on an inflow cell skipped: together the same as imposing the
//     inflow and zeroing the solids after the forces, without a pass and a barrier of their own;
//   * with an inflow profile (the kernels named *_profile_*; include/sfl.h "INFLOW PROFILES AND FLUX"): the records of the
//     member's row of the profile's table into the same array, beside the forces;
//   * divergence (divergence_sum_open), solve (sor_open_in_lds: sor_solid_in_lds' loop, only the set-up of k differs),
//     gradient (project_cell_open), dye as ever.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell).
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#include "batch.h"
#include "small_grid_core.h"
#include "stats_kernels.h"

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
namespace {

using namespace small_core;

constexpr int kThreads = SFL_BATCH_THREADS;
static_assert(cells_per_colour<kThreads>() * kThreads == kSmallGridMaxCells / 2, "SFL_BATCH_THREADS must divide 3072");

// the step of one member: every pointer at that member's first cell, its force records (batch_grid.hip member_step)
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

// the open codes of one member (stride 0 = one set for all members) and its inflow velocity
__device__ __forceinline__ const uint16_t *member_codes(const BatchOpenings &o, size_t member) { return o.codes + member * o.member_stride; }
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

// One whole step of the grid `a` describes, its open codes at `codes`; returns the carved LDS (p and d final, for the
// update norm of the *_each kernel).  kProfile: the records of `row` -- unique fluid inflow cells, which the force loop
// never writes -- go into l.v by all threads behind the advection's barrier, beside the forces, and ONE barrier that every
// workgroup reaches stands in front of the divergence instead of the forces' own.
template <bool kProfile = false>
__device__ __forceinline__ Lds open_step(const SmallStep &a, const uint16_t *__restrict__ codes, float2 inflow, char *lds_raw,
                                         ProfileRow row = ProfileRow{nullptr, nullptr, 0})
{
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in);
    float2 *v_out = reinterpret_cast<float2 *>(a.v_out);

    // advect(v_next, v, v, dt, no_slip) on every cell (item 1); an inflow cell holds the inflow (item 2a), a solid one (0, 0)
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float2 u = v_in[c];
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        const float2 r = sample_global_vec2f<true>(v_in, g, s, si, sj);
        const int code = codes[c];
        l.v[c] = !(code & kSolidFluid) ? make_float2(0.0f, 0.0f) : is_inflow_cell(code) ? inflow : r;
    }
    __syncthreads();
    if constexpr (kProfile)   // the profile's part of item 2a
        for (int k = threadIdx.x; k < row.n; k += kThreads) l.v[row.cells[k]] = row.vel[k];
    // drag forces, in queue order: later entries win; a record on a solid or an inflow cell has no effect (items 2, 2a, 3)
    if (a.n_forces > 0) {
        if (threadIdx.x == 0)
            for (int k = 0; k < a.n_forces; ++k) {
                const int i = a.force_cells[2 * k], gj = a.force_cells[2 * k + 1];
                if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                const int code = codes[gj * dim_x + i];
                if (!(code & kSolidFluid) || is_inflow_cell(code)) continue;
                l.v[gj * dim_x + i] = make_float2(a.force_vel[2 * k], a.force_vel[2 * k + 1]);
            }
        if constexpr (!kProfile) __syncthreads();
    }
    if constexpr (kProfile) __syncthreads();   // the records and the forces are visible to the divergence
    // the divergence of a fluid cell; 0.0f in a solid one (item 4)
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int code = codes[c];
        const float sum = divergence_sum_open(l.v + c, dim_x, code);
        const float dv = (code & kSolidFluid) ? sum * a.two_dx_inv : 0.0f;
        l.d[c] = dv;
        a.div[c] = dv;
    }
    // the pressure (item 5; the barrier inside also orders the divergence writes above)
    sor_open_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, a.iters, a.prm);
    // the gradient (item 6), then the dye back-trace with the projected velocity of the cell itself (item 7)
    const uint32_t *col_in = a.col_in;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float pc = l.p[c];
        const float2 u = project_cell_open(l.v[c], l.p + c, dim_x, codes[c], a.two_dx_inv);
        v_out[c] = u;
        a.p[c] = pc;
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        store_uq3(a.col_out, (size_t)c, sample_global_uq3<false>(col_in, g, s, si, sj));
    }
    return l;
}

// poisson_solve of ONE grid with openings: d_in -> p_out (solve_in_lds)
__device__ __forceinline__ Lds open_solve(char *lds_raw, float *p_out, const float *d_in, const uint16_t *__restrict__ codes, int dim_x,
                                          int dim_y, int iters, SorParams prm)
{
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) l.d[c] = d_in[c];
    sor_open_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, iters, prm);   // (its first barrier also covers the copy of d)
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[c] = l.p[c];
    return l;
}

__global__ void SFL_BATCH_BOUNDS
batch_open_step_kernel(BatchStep b, BatchOpenings open)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    open_step(a, member_codes(open, blockIdx.x), member_inflow(open, blockIdx.x), lds_raw);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_step_each_kernel(BatchStep b, BatchOpenings open, const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];   // workgroup-uniform: scalar loads
    const size_t member = (size_t)q.member;      // (the host hands out long members first)
    SmallStep a = member_step(b, member);
    a.dt = q.dt;
    a.two_dx_inv = q.two_dx_inv;
    a.iters = q.iters;
    a.prm = q.prm;
    const uint16_t *codes = member_codes(open, member);
    const Lds l = open_step(a, codes, member_inflow(open, member), lds_raw);
    // (the step's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_open_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

// ... with an inflow profile: the same step, the member's row of the table beside its codes
__global__ void SFL_BATCH_BOUNDS
batch_open_profile_step_kernel(BatchStep b, BatchOpenings open, BatchProfile profile)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    open_step<true>(a, member_codes(open, blockIdx.x), member_inflow(open, blockIdx.x), lds_raw, member_profile(profile, blockIdx.x));
}

__global__ void SFL_BATCH_BOUNDS
batch_open_profile_step_each_kernel(BatchStep b, BatchOpenings open, BatchProfile profile, const BatchMember *__restrict__ members,
                                    float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    a.dt = q.dt;
    a.two_dx_inv = q.two_dx_inv;
    a.iters = q.iters;
    a.prm = q.prm;
    const uint16_t *codes = member_codes(open, member);
    const Lds l = open_step<true>(a, codes, member_inflow(open, member), lds_raw, member_profile(profile, member));
    update_norm_open_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchOpenings open, int dim_x, int dim_y, int iters,
                        SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const size_t base = (size_t)blockIdx.x * (size_t)dim_x * (size_t)dim_y;
    open_solve(lds_raw, p_out + base, d_in + base, member_codes(open, blockIdx.x), dim_x, dim_y, iters, prm);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_solve_each_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchOpenings open, int dim_x, int dim_y,
                             const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t base = (size_t)q.member * (size_t)dim_x * (size_t)dim_y;
    const uint16_t *codes = member_codes(open, (size_t)q.member);
    const Lds l = open_solve(lds_raw, p_out + base, d_in + base, codes, dim_x, dim_y, q.iters, q.prm);
    update_norm_open_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, q.prm.dx, report + q.member);
}

// ---- the velocity statistics of members with openings (batch_solids.hip solid_velocity_stats_kernel) -----------------
// max |v.x|, max |v.y| over all cells and max |divergence| by item 4 of the rule over all cells, as bit patterns into
// records zeroed in front.  blockIdx.y is the member, the workgroups of blockIdx.x share its cells.
constexpr int kStatsThreads = 256;

__global__ void __launch_bounds__(kStatsThreads)
open_velocity_stats_kernel(const float *__restrict__ v, BatchOpenings open, int dim_x, int dim_y, float two_dx_inv,
                           const float *__restrict__ member_two_dx_inv, FlowStatsRecord *__restrict__ out)
{
    const size_t member = blockIdx.y;
    const int cells = dim_x * dim_y;
    const float2 *q = reinterpret_cast<const float2 *>(v) + member * (size_t)cells;
    const uint16_t *codes = member_codes(open, member);
    const float scale = member_two_dx_inv ? member_two_dx_inv[member] : two_dx_inv;
    unsigned m[3] = {0u, 0u, 0u};
    for (int c = blockIdx.x * kStatsThreads + threadIdx.x; c < cells; c += gridDim.x * kStatsThreads) {
        const int code = codes[c];
        const float2 own = q[c];
        const float sum = divergence_sum_open(q + c, dim_x, code);
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

// every step or solve launch of this file: one workgroup per member, 16 B of LDS per cell, granted once per device
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

}  // namespace

hipError_t launch_batch_open_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, int batch)
{
    return launch_members<batch_open_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open);
}

hipError_t launch_batch_open_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, int batch,
                                       const BatchMember *members, float *report)
{
    return launch_members<batch_open_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open, members, report);
}

hipError_t launch_batch_open_profile_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile, int batch)
{
    return launch_members<batch_open_profile_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open, profile);
}

hipError_t launch_batch_open_profile_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                               int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_open_profile_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open, profile, members, report);
}

hipError_t launch_batch_open_solve(hipStream_t s, float *p, const float *d, const BatchOpenings &open, int dim_x, int dim_y,
                                   int batch, int iters, SorParams prm)
{
    return launch_members<batch_open_solve_kernel>(s, dim_x, dim_y, batch, p, d, open, dim_x, dim_y, iters, prm);
}

hipError_t launch_batch_open_solve_each(hipStream_t s, float *p, const float *d, const BatchOpenings &open, int dim_x, int dim_y,
                                        int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_open_solve_each_kernel>(s, dim_x, dim_y, batch, p, d, open, dim_x, dim_y, members, report);
}

hipError_t launch_open_velocity_stats(hipStream_t s, FlowStatsRecord *out, const float *v, const BatchOpenings &open, int dim_x,
                                      int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv)
{
    if (members <= 0) return hipSuccess;
    const int cells = dim_x * dim_y;
    const int per_member = (cells + 4 * kStatsThreads - 1) / (4 * kStatsThreads);   // four cells per thread, at most six workgroups
    for (int first = 0; first < members; first += 65535) {   // (gridDim.y is a 16-bit number)
        const int count = members - first < 65535 ? members - first : 65535;
        BatchOpenings part = open;
        part.codes += (size_t)first * open.member_stride;
        part.inflow += 2 * (size_t)first;
        open_velocity_stats_kernel<<<dim3(per_member, count), kStatsThreads, 0, s>>>(
            v + 2 * (size_t)first * cells, part, dim_x, dim_y, two_dx_inv, member_two_dx_inv ? member_two_dx_inv + first : nullptr,
            out + first);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sfl
