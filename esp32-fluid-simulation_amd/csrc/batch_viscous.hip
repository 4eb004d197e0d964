// batch_viscous.hip -- batch members with a viscosity (gfx950 / MI355X; include/sfl.h "VISCOSITY"): the member step of
// batch_grid.hip and the one of batch_solids.hip with item 3a, the implicit diffusion of the velocity, inserted between the
// forces and the divergence.  Kernels of their own, written again the way batch_solids.hip wrote batch_grid.hip's again:
// the kernels of batch_grid.hip, batch_solids.hip and small_step_body.inc keep their text and their instructions, and a
// batch without a viscosity launches exactly what it launched before.
//
// THE DIFFUSION RUNS IN LDS WITH NO EXTRA BYTES.  carve() places d and p side by side behind the velocity, 8 B per cell,
// and both are dead until item 4: u0 lives there as float2 while u lives in l.v.  A thread owns the same cells of a
// colour in every half-sweep (the ownership of sor_in_lds: position q = thread + k * threads of the colour's row-major
// list) and keeps their index and which neighbours are inside the domain in three registers per colour; a half-sweep
// reads the other colour's cells from l.v and writes its own -- a barrier behind each.  The update is diffuse_tile.h's,
// the one every user shares.
//
// Per-member a, c and sweeps arrive from record `member` of a BatchViscous table -- a workgroup-uniform address, scalar
// loads -- and a member with sweeps == 0 (the host stores that for nu == 0 too) skips the item by a workgroup-uniform
// branch: no bit of it changes.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell);
// profiles/viscosity.txt has the registers.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the header's order.
#include "diffuse_tile.h"
#include "small_grid_core.h"
#include "viscous_kernels.h"

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

__device__ __forceinline__ const uint8_t *member_codes(const BatchSolids &s, size_t member) { return s.codes + member * s.member_stride; }

// Item 3a: `q.sweeps` sweeps on u = l.v, u0 in the 8 B per cell where d and p will live.  l.v is complete (a barrier in
// front); a barrier behind the last half-sweep.  codes: null without solids.
__device__ __forceinline__ void diffuse_in_lds(const Lds &l, const uint8_t *__restrict__ codes, int dim_x, int dim_y, BatchViscous q)
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
            const bool fluid = have && (!codes || (codes[c] & kSolidFluid));
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

// One whole step of the grid `a` describes with item 3a by `q`; kSolids: its code bytes at `codes` and the solids' rule
// (batch_solids.hip solid_step), else the plain member step (small_step_body.inc).  Returns the carved LDS (p and d
// final, for the update norm of the *_each kernels).
template <bool kSolids>
__device__ __forceinline__ Lds viscous_step(const SmallStep &a, const uint8_t *__restrict__ codes, BatchViscous q, char *lds_raw)
{
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in);
    float2 *v_out = reinterpret_cast<float2 *>(a.v_out);

    // advect(v_next, v, v, dt, no_slip) on every cell (item 1); with solids a solid cell keeps (0, 0) (item 3)
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float2 u = v_in[c];
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        const float2 r = sample_global_vec2f<true>(v_in, g, s, si, sj);
        if constexpr (kSolids)
            l.v[c] = (codes[c] & kSolidFluid) ? r : make_float2(0.0f, 0.0f);
        else
            l.v[c] = r;
    }
    __syncthreads();
    // drag forces, in queue order: later entries win; a record on a solid cell has no effect (items 2 and 3)
    if (a.n_forces > 0) {
        if (threadIdx.x == 0)
            for (int k = 0; k < a.n_forces; ++k) {
                const int i = a.force_cells[2 * k], gj = a.force_cells[2 * k + 1];
                if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                if constexpr (kSolids)
                    if (!(codes[gj * dim_x + i] & kSolidFluid)) continue;
                l.v[gj * dim_x + i] = make_float2(a.force_vel[2 * k], a.force_vel[2 * k + 1]);
            }
        __syncthreads();
    }
    // the diffusion (item 3a); skipped whole by a member without one
    if (q.sweeps > 0) diffuse_in_lds(l, kSolids ? codes : nullptr, dim_x, dim_y, q);
    // the divergence (item 4)
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        float dv;
        if constexpr (kSolids) {
            const int code = codes[c];
            const float sum = divergence_sum_solid(l.v + c, dim_x, code);
            dv = (code & kSolidFluid) ? sum * a.two_dx_inv : 0.0f;
        } else {
            const int gj = c / dim_x, i = c - gj * dim_x;
            dv = divergence_sum(l.v + c, dim_x, i, gj, i_max, j_max) * a.two_dx_inv;
        }
        // (d lies where u0 lay: cell c's d is written while another thread may still read its neighbours' velocity, never u0)
        l.d[c] = dv;
        a.div[c] = dv;
    }
    // the pressure (item 5; the barrier inside also orders the divergence writes above)
    if constexpr (kSolids)
        sor_solid_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, a.iters, a.prm);
    else
        sor_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, a.iters, a.prm);
    // the gradient (item 6), then the dye back-trace with the projected velocity of the cell itself (item 7)
    const uint32_t *col_in = a.col_in;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float pc = l.p[c];
        float2 u;
        if constexpr (kSolids)
            u = project_cell_solid(l.v[c], l.p + c, dim_x, codes[c], a.two_dx_inv);
        else
            u = project_cell(l.v[c], l.p + c, dim_x, i, gj, i_max, j_max, a.two_dx_inv);
        v_out[c] = u;
        a.p[c] = pc;
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        store_uq3(a.col_out, (size_t)c, sample_global_uq3<false>(col_in, g, s, si, sj));
    }
    return l;
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_step_kernel(BatchStep b, const BatchViscous *__restrict__ visc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    viscous_step<false>(a, nullptr, visc[blockIdx.x], lds_raw);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_step_each_kernel(BatchStep b, const BatchViscous *__restrict__ visc, const BatchMember *__restrict__ members,
                               float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];   // workgroup-uniform: scalar loads
    const size_t member = (size_t)q.member;      // (the host hands out long members first)
    SmallStep a = member_step(b, member);
    a.dt = q.dt;
    a.two_dx_inv = q.two_dx_inv;
    a.iters = q.iters;
    a.prm = q.prm;
    const Lds l = viscous_step<false>(a, nullptr, visc[member], lds_raw);
    // (the step's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_in_lds<kThreads>(l.p, l.d, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_solid_step_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    viscous_step<true>(a, member_codes(solids, blockIdx.x), visc[blockIdx.x], lds_raw);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_solid_step_each_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc,
                                     const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    a.dt = q.dt;
    a.two_dx_inv = q.two_dx_inv;
    a.iters = q.iters;
    a.prm = q.prm;
    const uint8_t *codes = member_codes(solids, member);
    const Lds l = viscous_step<true>(a, codes, visc[member], lds_raw);
    update_norm_solid_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

// every launch of this file: one workgroup per member, 16 B of LDS per cell, granted once per device
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

hipError_t launch_batch_viscous_step(hipStream_t s, const BatchStep &a, const BatchViscous *visc, int batch)
{
    return launch_members<batch_viscous_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, visc);
}

hipError_t launch_batch_viscous_step_each(hipStream_t s, const BatchStep &a, const BatchViscous *visc, int batch,
                                          const BatchMember *members, float *report)
{
    return launch_members<batch_viscous_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, visc, members, report);
}

hipError_t launch_batch_viscous_solid_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                           int batch)
{
    return launch_members<batch_viscous_solid_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids, visc);
}

hipError_t launch_batch_viscous_solid_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids,
                                                const BatchViscous *visc, int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_viscous_solid_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids, visc, members, report);
}

}  // namespace sfl
