// batch_large.hip -- batches of LARGE members in one launch (gfx950 / MI355X): workgroup k runs the whole sim step, or the
// whole pressure solve, of one member of up to kLargeMemberMaxCells cells (128 x 128, 160 x 120) with 8 B of LDS per cell
// (large_member_core.h: the advected velocity first, the divergence and the pressure afterwards).  The batches of
// sfl_batch_create_large; batch_grid.hip's kernels (16 B per cell, at most 6144 cells) are those of sfl_batch_create and
// are not touched by this file.
//
// One workgroup of 1024 threads per member, one member per CU: up to 158 KB of a CU's 160 KB of LDS, and the register
// budget of four waves per SIMD (128 VGPRs).  Nothing depends on the order in which workgroups run or on where they land;
// a member that follows another on a CU zero-fills its pressure and overwrites the whole region before it reads it.
//
// Six entry points, three kernels of each kind from one templated body: uniform parameters (step_n, poisson_solve),
// per-member parameters with the update norm at the end (*_each), and per-member parameters with the solve stopped at a
// tolerance (*_until).  The records (BatchMember, BatchStop) are read at a workgroup-uniform address: scalar loads.
// Results are, bit for bit, those of a context of the member's shape -- and of batch_grid.hip's kernels at shapes both take.
//
// Addressing: a member's base offset (member x cells x element) is computed in 64-bit; offsets inside a member are
// 32-bit ints.  Numerics contract: -ffp-contract=off, no denormal flushing.
#include "batch_member.h"
#include "large_member_core.h"

namespace sfl {
namespace {

using namespace large_core;
using batch_member::apply_member;   // (the two that do not depend on the bytes of LDS per cell)
using batch_member::member_step;

// what a member leaves besides its fields: report[m] = the update norm of its final pressure (kEach, kUntil) and
// counts[2 m], counts[2 m + 1] = the iterations of this solve and their sum over the launches of one call (kUntil; `add`
// = 0 in the call's first launch).  Plain stores by thread 0.
template <int kMode>
__device__ __forceinline__ void leave(const Solved &r, size_t member, float *report, int *counts, int add)
{
    if (kMode != kUniform && threadIdx.x == 0) {
        report[member] = __uint_as_float(r.norm_bits);
        if (kMode == kUntil) {
            counts[2 * member] = r.iters;
            counts[2 * member + 1] = add ? counts[2 * member + 1] + r.iters : r.iters;
        }
    }
}

// ---- one whole step (ino:252-287) of the member that workgroup blockIdx.x is given ---------------------------------------
// kUniform: member blockIdx.x with the parameters of b.step; members, stops, report, counts unused.  Otherwise record
// blockIdx.x names the member and carries its dt, 1 / (2 dx), iters (kUntil: the cap) and SOR constants; stops[blockIdx.x]
// goes with it (kUntil).
template <int kMode>
__global__ void __launch_bounds__(kThreads)
large_step_kernel(BatchStep b, const BatchMember *__restrict__ members, const BatchStop *__restrict__ stops,
                  float *__restrict__ report, int *__restrict__ counts, int add)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    size_t member = blockIdx.x;
    float tol = -1.0f;
    int every = 1;
    SmallStep a;
    if (kMode == kUniform) {
        a = member_step(b, member);
    } else {
        const BatchMember q = members[blockIdx.x];   // workgroup-uniform: scalar loads
        member = (size_t)q.member;                   // (the host hands out long members first)
        a = member_step(b, member);
        apply_member(a, q);
        if (kMode == kUntil) {
            const BatchStop stop = stops[blockIdx.x];
            tol = stop.tol;
            every = stop.every;
        }
    }
    const Solved r = step_member<kMode>(lds_raw, a, tol, every);
    leave<kMode>(r, member, report, counts, add);
}

// ---- poisson_solve (poisson.cpp:114-125) of the member that workgroup blockIdx.x is given --------------------------------
template <int kMode>
__global__ void __launch_bounds__(kThreads)
large_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y, int iters, SorParams prm,
                   const BatchMember *__restrict__ members, const BatchStop *__restrict__ stops, float *__restrict__ report,
                   int *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    size_t member = blockIdx.x;
    float tol = -1.0f;
    int every = 1;
    if (kMode != kUniform) {
        const BatchMember q = members[blockIdx.x];
        member = (size_t)q.member;
        iters = q.iters;
        prm = q.prm;
        if (kMode == kUntil) {
            const BatchStop stop = stops[blockIdx.x];
            tol = stop.tol;
            every = stop.every;
        }
    }
    const size_t base = member * (size_t)dim_x * (size_t)dim_y;
    const Solved r = solve_member<kMode>(lds_raw, p_out + base, d_in + base, dim_x, dim_y, iters, prm, tol, every);
    leave<kMode>(r, member, report, counts, 0);
}

// every launch of this file: one workgroup per member, 8 B of dynamic LDS per cell; more than 64 KB of it has to be
// granted once per kernel and device
template <auto KERNEL, class... A>
hipError_t launch_members(hipStream_t s, int dim_x, int dim_y, int batch, A... args)
{
    static bool granted[64];
    if (!large_member_fits(dim_x, dim_y)) return hipErrorInvalidValue;   // (the dynamic LDS below, the threads' cells)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!granted[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLargeMemberMaxCells * 8);
        if (e != hipSuccess) return e;
        granted[dev] = true;
    }
    const size_t lds = (size_t)dim_x * dim_y * 8;
    KERNEL<<<batch, kThreads, lds, s>>>(args...);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_large_step(hipStream_t s, const BatchStep &a, int batch)
{
    return launch_members<large_step_kernel<kUniform>>(s, a.step.dim_x, a.step.dim_y, batch, a, nullptr, nullptr, nullptr,
                                                       nullptr, 0);
}

hipError_t launch_batch_large_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch, int iters,
                                    SorParams prm)
{
    return launch_members<large_solve_kernel<kUniform>>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, iters, prm, nullptr,
                                                        nullptr, nullptr, nullptr);
}

hipError_t launch_batch_large_step_each(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                        float *report)
{
    return launch_members<large_step_kernel<kEach>>(s, a.step.dim_x, a.step.dim_y, batch, a, members, nullptr, report,
                                                    nullptr, 0);
}

hipError_t launch_batch_large_solve_each(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                         const BatchMember *members, float *report)
{
    return launch_members<large_solve_kernel<kEach>>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, 0, SorParams{}, members,
                                                     nullptr, report, nullptr);
}

hipError_t launch_batch_large_step_until(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                         const BatchStop *stops, float *report, int *counts, bool add)
{
    return launch_members<large_step_kernel<kUntil>>(s, a.step.dim_x, a.step.dim_y, batch, a, members, stops, report, counts,
                                                     add ? 1 : 0);
}

hipError_t launch_batch_large_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                          const BatchMember *members, const BatchStop *stops, float *report, int *counts)
{
    return launch_members<large_solve_kernel<kUntil>>(s, dim_x, dim_y, batch, p, d, dim_x, dim_y, 0, SorParams{}, members,
                                                      stops, report, counts);
}

}  // namespace sfl
