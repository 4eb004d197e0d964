// batch_openings.hip -- batch members with openings on the rim of their grids (gfx950 / MI355X; include/sfl.h "OPENINGS"):
// the step, the pressure solve and the velocity statistics of batch_solids.hip for a batch whose members carry a map of
// inflow and outflow cells, with or without solid cells.  The kernels and launchers alone: their bodies are
// batch_member.h's and small_grid_core.h's, the ones batch_solids.hip instantiates on bytes, instantiated here on open
// codes and with the member's inflow.  Kernels of their own: a batch without openings launches exactly what it did.
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
//   * divergence (divergence_sum_open), solve (sor_coded_in_lds: only the set-up of k knows the outflow), gradient
//     (project_cell_open), dye as ever.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell).
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;

__global__ void SFL_BATCH_BOUNDS
batch_open_step_kernel(BatchStep b, BatchOpenings open)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds(a, member_codes(open, blockIdx.x), lds_raw, member_inflow(open, blockIdx.x));
}

__global__ void SFL_BATCH_BOUNDS
batch_open_step_each_kernel(BatchStep b, BatchOpenings open, const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint16_t *codes = member_codes(open, member);
    const Lds l = step_in_lds(a, codes, lds_raw, member_inflow(open, member));
    // (the step's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

// ... with an inflow profile: the same step, the member's row of the table beside its codes
__global__ void SFL_BATCH_BOUNDS
batch_open_profile_step_kernel(BatchStep b, BatchOpenings open, BatchProfile profile)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds<uint16_t, false, true>(a, member_codes(open, blockIdx.x), lds_raw, member_inflow(open, blockIdx.x), kNoViscosity,
                                       member_profile(profile, blockIdx.x));
}

__global__ void SFL_BATCH_BOUNDS
batch_open_profile_step_each_kernel(BatchStep b, BatchOpenings open, BatchProfile profile, const BatchMember *__restrict__ members,
                                    float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint16_t *codes = member_codes(open, member);
    const Lds l = step_in_lds<uint16_t, false, true>(a, codes, lds_raw, member_inflow(open, member), kNoViscosity,
                                                     member_profile(profile, member));
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchOpenings open, int dim_x, int dim_y, int iters,
                        SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const size_t base = (size_t)blockIdx.x * (size_t)dim_x * (size_t)dim_y;
    coded_solve_in_lds(lds_raw, p_out + base, d_in + base, member_codes(open, blockIdx.x), dim_x, dim_y, iters, prm);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_solve_each_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchOpenings open, int dim_x, int dim_y,
                             const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t base = (size_t)q.member * (size_t)dim_x * (size_t)dim_y;
    const uint16_t *codes = member_codes(open, (size_t)q.member);
    const Lds l = coded_solve_in_lds(lds_raw, p_out + base, d_in + base, codes, dim_x, dim_y, q.iters, q.prm);
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, q.prm.dx, report + q.member);
}

__global__ void __launch_bounds__(kStatsThreads)
open_velocity_stats_kernel(const float *__restrict__ v, BatchOpenings open, int dim_x, int dim_y, float two_dx_inv,
                           const float *__restrict__ member_two_dx_inv, FlowStatsRecord *__restrict__ out)
{
    velocity_stats_of(v, open, dim_x, dim_y, two_dx_inv, member_two_dx_inv, out);
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
    return launch_coded_velocity_stats<open_velocity_stats_kernel>(s, out, v, open, dim_x, dim_y, members, two_dx_inv,
                                                                   member_two_dx_inv);
}

}  // namespace sfl
