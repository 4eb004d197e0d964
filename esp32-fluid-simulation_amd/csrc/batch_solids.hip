// batch_solids.hip -- batch members with solid cells inside their grids (gfx950 / MI355X; include/sfl.h "SOLIDS"): the
// step, the pressure solve and the velocity statistics of batch_grid.hip and flow_stats.hip for a batch whose members
// carry a mask of solid cells.  The kernels and launchers alone: their bodies are batch_member.h's (step_in_lds,
// coded_solve_in_lds, velocity_stats_of) and small_grid_core.h's (sor_coded_in_lds, update_norm_coded_in_lds), shared with
// batch_openings.hip and batch_viscous.hip and instantiated here on bytes.  Kernels of their own beside batch_grid.hip's,
// whose text is small_step_body.inc and keeps its instructions: a batch without solids launches exactly what it did.
//
// One CODE BYTE per cell, formed on the host (solids.cpp) and read from memory: bits 0..3 = W, E, S, N neighbour present
// (inside the domain and fluid), bit 4 = the cell is fluid, a solid cell's byte 0 (advect_math.h).  The bytes stay out of
// LDS -- two members of 61 x 81 share a CU with 2 x 79 056 of its 163 840 bytes, and a byte per cell in LDS would cost the
// second member -- and a mask shared by all members (member stride 0) stays in L2.  The solve's set-up reads the byte of
// every owned cell once, into the registers sor_iteration already keeps (sor_cells_init_coded); its loop is the
// existing one.  The three per-cell passes of a step read it once per cell.
//
// The step, in the order of small_step_body.inc (the rule of include/sfl.h, items 1 - 7):
//   * advection of the velocity as it stands, on every cell; what is stored for a solid cell is (0, 0);
//   * forces in queue order, a record on a solid cell skipped: together the same as zeroing the solids after the forces,
//     without a pass and a barrier of its own;
//   * divergence (divergence_sum_solid), solve (sor_coded_in_lds), gradient (project_cell_solid), dye as ever.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell).
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;

__global__ void SFL_BATCH_BOUNDS
batch_solid_step_kernel(BatchStep b, BatchSolids solids)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds(a, member_codes(solids, blockIdx.x), lds_raw);
}

__global__ void SFL_BATCH_BOUNDS
batch_solid_step_each_kernel(BatchStep b, BatchSolids solids, const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint8_t *codes = member_codes(solids, member);
    const Lds l = step_in_lds(a, codes, lds_raw);
    // (the step's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_solid_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchSolids solids, int dim_x, int dim_y, int iters,
                         SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const size_t base = (size_t)blockIdx.x * (size_t)dim_x * (size_t)dim_y;
    coded_solve_in_lds(lds_raw, p_out + base, d_in + base, member_codes(solids, blockIdx.x), dim_x, dim_y, iters, prm);
}

__global__ void SFL_BATCH_BOUNDS
batch_solid_solve_each_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, BatchSolids solids, int dim_x, int dim_y,
                              const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t base = (size_t)q.member * (size_t)dim_x * (size_t)dim_y;
    const uint8_t *codes = member_codes(solids, (size_t)q.member);
    const Lds l = coded_solve_in_lds(lds_raw, p_out + base, d_in + base, codes, dim_x, dim_y, q.iters, q.prm);
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, dim_x, dim_y, q.prm.dx, report + q.member);
}

__global__ void __launch_bounds__(kStatsThreads)
solid_velocity_stats_kernel(const float *__restrict__ v, BatchSolids solids, int dim_x, int dim_y, float two_dx_inv,
                            const float *__restrict__ member_two_dx_inv, FlowStatsRecord *__restrict__ out)
{
    velocity_stats_of(v, solids, dim_x, dim_y, two_dx_inv, member_two_dx_inv, out);
}

}  // namespace

hipError_t launch_batch_solid_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, int batch)
{
    return launch_members<batch_solid_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids);
}

hipError_t launch_batch_solid_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids, int batch,
                                        const BatchMember *members, float *report)
{
    return launch_members<batch_solid_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids, members, report);
}

hipError_t launch_batch_solid_solve(hipStream_t s, float *p, const float *d, const BatchSolids &solids, int dim_x, int dim_y,
                                    int batch, int iters, SorParams prm)
{
    return launch_members<batch_solid_solve_kernel>(s, dim_x, dim_y, batch, p, d, solids, dim_x, dim_y, iters, prm);
}

hipError_t launch_batch_solid_solve_each(hipStream_t s, float *p, const float *d, const BatchSolids &solids, int dim_x, int dim_y,
                                         int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_solid_solve_each_kernel>(s, dim_x, dim_y, batch, p, d, solids, dim_x, dim_y, members, report);
}

hipError_t launch_solid_velocity_stats(hipStream_t s, FlowStatsRecord *out, const float *v, const BatchSolids &solids, int dim_x,
                                       int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv)
{
    return launch_coded_velocity_stats<solid_velocity_stats_kernel>(s, out, v, solids, dim_x, dim_y, members, two_dx_inv,
                                                                    member_two_dx_inv);
}

}  // namespace sfl
