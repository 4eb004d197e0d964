// batch_viscous.hip -- batch members with a viscosity (gfx950 / MI355X; include/sfl.h "VISCOSITY"): the member step of
// batch_grid.hip and the one of batch_solids.hip with item 3a, the implicit diffusion of the velocity, inserted between the
// forces and the divergence.  The kernels and launchers alone: the step is batch_member.h's step_in_lds with item 3a asked
// for -- without codes (the plain member step) or on the solids' bytes -- and the diffusion its diffuse_in_lds, which runs
// in the 16 B of LDS per cell that a step has anyway.  Kernels of their own: a batch without a viscosity launches exactly
// what it launched before.
//
// Per-member a, c and sweeps arrive from record `member` of a BatchViscous table -- a workgroup-uniform address, scalar
// loads -- and a member with sweeps == 0 (the host stores that for nu == 0 too) skips the item by a workgroup-uniform
// branch: no bit of it changes.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell);
// profiles/viscosity.txt has the registers.
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;

__global__ void SFL_BATCH_BOUNDS
batch_viscous_step_kernel(BatchStep b, const BatchViscous *__restrict__ visc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds<void, true>(a, nullptr, lds_raw, no_inflow(), visc[blockIdx.x]);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_step_each_kernel(BatchStep b, const BatchViscous *__restrict__ visc, const BatchMember *__restrict__ members,
                               float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const Lds l = step_in_lds<void, true>(a, nullptr, lds_raw, no_inflow(), visc[member]);
    // (the step's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_in_lds<kThreads>(l.p, l.d, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_solid_step_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds<uint8_t, true>(a, member_codes(solids, blockIdx.x), lds_raw, no_inflow(), visc[blockIdx.x]);
}

__global__ void SFL_BATCH_BOUNDS
batch_viscous_solid_step_each_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc,
                                     const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint8_t *codes = member_codes(solids, member);
    const Lds l = step_in_lds<uint8_t, true>(a, codes, lds_raw, no_inflow(), visc[member]);
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
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
