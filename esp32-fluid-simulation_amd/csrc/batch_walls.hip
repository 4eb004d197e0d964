// batch_walls.hip -- batch members whose solid cells hold a prescribed velocity (gfx950 / MI355X; include/sfl.h "WALL
// VELOCITIES"): the member step of batch_viscous.hip on the solids' bytes and the one of batch_openings.hip with a profile,
// each with the member's row of the wall table.  The kernels and launchers alone: the step is batch_member.h's step_in_lds
// with kWalls asked for -- the row's records into l.v beside the profile's (the extended item 3, which only item 3a
// reads) and into v_out behind the projection (item 8).  Kernels of their own: a batch without a wall table launches
// exactly what it launched before.
//
// Two cases carry every combination the host admits:
//   * code bytes with kViscous: a batch without viscosity hands in no table of BatchViscous records and every member runs
//     kNoViscosity, whose sweeps == 0 skips item 3a by the workgroup-uniform branch the viscous kernels have anyway;
//   * open codes with kProfile: a batch without a profile hands in no table and every member's row is empty -- a loop that
//     does not run; barriers do not change bits.
// The table's row is read at workgroup-uniform addresses (scalar loads), its records by all threads.
//
// Workgroup shape and occupancy: those of batch_grid.hip (1024 threads, 8 waves per SIMD, 16 B of dynamic LDS per cell);
// profiles/walls.txt has the registers.
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;

__device__ __forceinline__ BatchViscous member_viscosity(const BatchViscous *__restrict__ visc, size_t member)
{
    return visc ? visc[member] : kNoViscosity;
}
__device__ __forceinline__ ProfileRow member_profile_or_none(const BatchProfile &t, size_t member)
{
    return t.offsets ? member_profile(t, member) : ProfileRow{nullptr, nullptr, 0};
}

__global__ void SFL_BATCH_BOUNDS
batch_wall_step_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc, BatchProfile walls)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds<uint8_t, true, false, true>(a, member_codes(solids, blockIdx.x), lds_raw, no_inflow(), member_viscosity(visc, blockIdx.x),
                                            ProfileRow{nullptr, nullptr, 0}, member_profile(walls, blockIdx.x));
}

__global__ void SFL_BATCH_BOUNDS
batch_wall_step_each_kernel(BatchStep b, BatchSolids solids, const BatchViscous *__restrict__ visc, BatchProfile walls,
                            const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint8_t *codes = member_codes(solids, member);
    const Lds l = step_in_lds<uint8_t, true, false, true>(a, codes, lds_raw, no_inflow(), member_viscosity(visc, member),
                                                          ProfileRow{nullptr, nullptr, 0}, member_profile(walls, member));
    // (item 8 only stores to v_out; l.p and l.d are final since the solve's last barrier)
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

__global__ void SFL_BATCH_BOUNDS
batch_open_wall_step_kernel(BatchStep b, BatchOpenings open, BatchProfile profile, BatchProfile walls)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
    step_in_lds<uint16_t, false, true, true>(a, member_codes(open, blockIdx.x), lds_raw, member_inflow(open, blockIdx.x), kNoViscosity,
                                             member_profile_or_none(profile, blockIdx.x), member_profile(walls, blockIdx.x));
}

__global__ void SFL_BATCH_BOUNDS
batch_open_wall_step_each_kernel(BatchStep b, BatchOpenings open, BatchProfile profile, BatchProfile walls,
                                 const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
    const uint16_t *codes = member_codes(open, member);
    const Lds l = step_in_lds<uint16_t, false, true, true>(a, codes, lds_raw, member_inflow(open, member), kNoViscosity,
                                                           member_profile_or_none(profile, member), member_profile(walls, member));
    update_norm_coded_in_lds<kThreads>(l.p, l.d, codes, a.dim_x, a.dim_y, a.prm.dx, report + member);
}

}  // namespace

hipError_t launch_batch_wall_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                  const BatchProfile &walls, int batch)
{
    return launch_members<batch_wall_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids, visc, walls);
}

hipError_t launch_batch_wall_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                       const BatchProfile &walls, int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_wall_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, solids, visc, walls, members, report);
}

hipError_t launch_batch_open_wall_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                       const BatchProfile &walls, int batch)
{
    return launch_members<batch_open_wall_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open, profile, walls);
}

hipError_t launch_batch_open_wall_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                            const BatchProfile &walls, int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_open_wall_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, open, profile, walls, members, report);
}

}  // namespace sfl
