// batch_grid.hip -- many small grids in ONE launch (gfx950 / MI355X): workgroup m runs the whole sim step, or the whole
// pressure solve, of batch member m with that member's fields in its LDS, exactly as small_grid.hip runs one grid.
//
// One small grid keeps one CU busy and leaves the other 255 idle (the sketch's 61 x 81 grid: one workgroup of 1024
// threads).  A batch fills the chip with independent members -- ensembles, parameter studies -- and the dispatcher
// places their workgroups wherever LDS and registers allow; nothing here depends on the order in which workgroups run
// or on the XCD a workgroup lands on.  The arithmetic is small_grid_core.h / small_step_body.inc, the very code of
// small_grid.hip: a member's results are bit for bit those of a context of its shape.
//
// Addressing: a member's base offset (member x cells x element) is computed in 64-bit -- a batch may hold more than 2^32
// bytes of one field -- and offsets inside a member stay 32-bit ints (at most kSmallGridMaxCells cells).
//
// Workgroup shape and occupancy are build knobs (profiles/batch_throughput.txt has the sweep at B = 1024): SFL_BATCH_THREADS
// threads per member, and SFL_BATCH_WAVES_PER_EU > 0 asks the compiler for a register budget that lets that many waves
// share a SIMD (8 with 1024 threads, 4 with 512: two members per CU, which LDS allows for the sketch's 79 KB members in a
// CU's 160 KB; 0 = the compiler's choice).  Shipped: 1024 threads at 8 waves per SIMD -- 64 VGPRs with one spilled to
// scratch, two members per CU -- 1.27x the member-steps/s of the same kernel at 70 VGPRs and one member per CU, whose
// instructions are small_step_kernel's; 512 threads ran slower with either budget.
//
// Per-member parameters (batch_step_each_kernel, batch_solve_each_kernel): the same bodies with dt, dx, iters and omega
// read from record blockIdx.x of a BatchMember array -- a workgroup-uniform address, so the values arrive by scalar loads,
// the iteration loop and its barriers stay scalar-controlled and the register budget above is not touched; members with
// different iteration counts simply leave at different times.  The record names its member: workgroups are handed out
// roughly in blockIdx order, and the host lists the members with the most iterations first, so that no long member
// starts last and sets the launch's end alone (1.46x at B = 1024 with iters spread over 5 .. 80, profiles/batch_params.txt).
// Results do not depend on that order.  These kernels end with the member's update norm
// (update_norm_in_lds): max |p_gs - p| over the final pressure, evaluated from the p and d still in LDS, one float per
// member.  They are kernels of their own, not a template parameter of the two above: the uniform kernels keep their
// instructions.
//
// Stopping at a tolerance (batch_step_until_kernel, batch_solve_until_kernel): the *_each kernels with sor_until_in_lds
// (small_grid_core.h) for their solve -- a check of the update norm in front of every `every`-th iteration, formed from
// the registers of the solve, and the member leaves the loop at the first one that finds the norm <= tol (or a NaN).
// tol and every arrive like the record, by scalar loads of BatchStop blockIdx.x, and the verdict of a check is made
// wave-uniform, so the loop stays scalar-controlled.  The last check is the report; the iterations run go out beside it.
// Kernels of their own again: the six kernels that existed keep their instructions (profiles/batch_until.txt).
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the
// reference's order.  Reference citations are file:line under /root/reference/ESP32-fluid-simulation/.
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;   // (the workgroup's shape, member_step, apply_member, launch_members)

// ---- one whole step of member blockIdx.x, ino:252-287 ---------------------------------------------
__global__ void SFL_BATCH_BOUNDS
batch_step_kernel(BatchStep b)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const SmallStep a = member_step(b, blockIdx.x);
#include "small_step_body.inc"
}

// ---- poisson_solve (poisson.cpp:114-125) of member blockIdx.x ------------------------------------
__global__ void SFL_BATCH_BOUNDS
batch_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y, int iters,
                   SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const size_t base = (size_t)blockIdx.x * (size_t)dim_x * (size_t)dim_y;
    solve_in_lds<kThreads>(lds_raw, p_out + base, d_in + base, dim_x, dim_y, iters, prm);
}

// (the update norm of one member, update_norm_in_lds: small_grid_core.h -- batch_play.hip ends with it too)

// ---- one whole step of member blockIdx.x with that member's parameters, then its update norm ------------------
__global__ void SFL_BATCH_BOUNDS
batch_step_each_kernel(BatchStep b, const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];   // workgroup-uniform: scalar loads
    const size_t member = (size_t)q.member;      // (the host hands out long members first)
    SmallStep a = member_step(b, member);
    apply_member(a, q);
#include "small_step_body.inc"
    // (the body's last loop only reads l.p and l.v; l.p and l.d are final since the solve's last barrier)
    update_norm_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, a.prm.dx, report + member);
}

// ---- poisson_solve of member blockIdx.x with that member's dx, iters and omega, then its update norm ----------
__global__ void SFL_BATCH_BOUNDS
batch_solve_each_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y,
                        const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const size_t base = (size_t)q.member * (size_t)dim_x * (size_t)dim_y;
    solve_in_lds<kThreads>(lds_raw, p_out + base, d_in + base, dim_x, dim_y, q.iters, q.prm);
    const Lds l = carve(lds_raw, dim_x * dim_y);
    update_norm_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, q.prm.dx, report + q.member);
}

// ---- the *_until kernels: the *_each kernels with the solve stopped at a tolerance (sor_until_in_lds) ---------------
// stops[k] belongs to members[k].  What a member leaves besides its fields: report[m] = the update norm of its final
// pressure (the solve's own last check: no walk afterwards) and counts[2 m], counts[2 m + 1] = the iterations of this
// solve and their sum over the launches of one call (`add` = 0 in the call's first launch).  Plain stores by thread 0.
__device__ __forceinline__ void leave_until(const UntilResult &r, size_t member, float *report, int *counts, int add)
{
    if (threadIdx.x == 0) {
        report[member] = __uint_as_float(r.norm_bits);
        counts[2 * member] = r.iters;
        counts[2 * member + 1] = add ? counts[2 * member + 1] + r.iters : r.iters;
    }
}

__global__ void SFL_BATCH_BOUNDS
batch_step_until_kernel(BatchStep b, const BatchMember *__restrict__ members, const BatchStop *__restrict__ stops,
                        float *__restrict__ report, int *__restrict__ counts, int add)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];   // workgroup-uniform: scalar loads
    const BatchStop stop = stops[blockIdx.x];
    const size_t member = (size_t)q.member;
    SmallStep a = member_step(b, member);
    apply_member(a, q);
#define SFL_STEP_SOLVE const UntilResult r = sor_until_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, a.iters, a.prm, stop.tol, stop.every)
#include "small_step_body.inc"
#undef SFL_STEP_SOLVE
    leave_until(r, member, report, counts, add);
}

__global__ void SFL_BATCH_BOUNDS
batch_solve_until_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y,
                         const BatchMember *__restrict__ members, const BatchStop *__restrict__ stops,
                         float *__restrict__ report, int *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const BatchMember q = members[blockIdx.x];
    const BatchStop stop = stops[blockIdx.x];
    const size_t base = (size_t)q.member * (size_t)dim_x * (size_t)dim_y;
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) l.d[c] = d_in[base + c];
    const UntilResult r = sor_until_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, q.iters, q.prm, stop.tol, stop.every);
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[base + c] = l.p[c];
    leave_until(r, (size_t)q.member, report, counts, 0);
}

}  // namespace

hipError_t launch_batch_step(hipStream_t s, const BatchStep &a, int batch)
{
    return launch_members<batch_step_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a);
}

hipError_t launch_batch_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch, int iters,
                              SorParams prm)
{
    return launch_members<batch_solve_kernel>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, iters, prm);
}

hipError_t launch_batch_step_each(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members, float *report)
{
    return launch_members<batch_step_each_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, members, report);
}

hipError_t launch_batch_solve_each(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                   const BatchMember *members, float *report)
{
    return launch_members<batch_solve_each_kernel>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, members, report);
}

hipError_t launch_batch_step_until(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                   const BatchStop *stops, float *report, int *counts, bool add)
{
    return launch_members<batch_step_until_kernel>(s, a.step.dim_x, a.step.dim_y, batch, a, members, stops, report, counts,
                                                   add ? 1 : 0);
}

hipError_t launch_batch_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                    const BatchMember *members, const BatchStop *stops, float *report, int *counts)
{
    return launch_members<batch_solve_until_kernel>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, members, stops, report,
                                                    counts);
}

}  // namespace sfl
