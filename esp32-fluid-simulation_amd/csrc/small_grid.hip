// small_grid.hip -- the whole sim step, or the whole pressure solve, of a SMALL grid in one launch of
// one workgroup (gfx950 / MI355X).
//
// The sketch's own grid is 61 x 81 cells (ino:12-14): 20 KB of velocity + pressure + divergence.  With
// one kernel per operator and one per few colour passes a step of that size is six to ten dependent
// launches of ~5 us each and the GPU idles in between (profiles/r02_experiments_without_gain.txt: a
// hipGraph does not help, the latency is on the GPU side).  Here ONE workgroup of 1024 threads keeps
// the advected velocity, the divergence and the pressure of the whole grid in its CU's LDS (16 B per
// cell: up to 6144 cells = 96 KB) and runs advection -> forces -> divergence -> the red-black SOR
// iterations (a workgroup barrier between colour passes) -> projection -> dye advection back to back.
// The arithmetic is that of the one-thread-per-cell kernels (stencil_kernels.hip, advect_math.h),
// expression by expression: same bits.  The device code itself lives in small_grid_core.h, which batch_grid.hip
// shares (one grid per workgroup, many grids per launch).
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the
// reference's order.  Reference citations are file:line under /root/reference/ESP32-fluid-simulation/.
#include "small_grid_core.h"
#include "until_kernels.h"

namespace sfl {
namespace {

using namespace small_core;

constexpr int kThreads = 1024;
constexpr int kCellsPerColour = cells_per_colour<kThreads>();

// ---- poisson_solve (poisson.cpp:114-125) alone ---------------------------------------------------
__global__ void __launch_bounds__(kThreads)
small_solve_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y, int iters,
                   SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    solve_in_lds<kThreads>(lds_raw, p_out, d_in, dim_x, dim_y, iters, prm);
}

// ---- `iters` more iterations on the pressure p_io holds (sfl_poisson_continue), in place ----------------------------
// A kernel of its own, as the one below: small_solve_kernel and small_step_kernel keep their instructions.
__global__ void __launch_bounds__(kThreads)
small_solve_warm_kernel(float *__restrict__ p_io, const float *__restrict__ d_in, int dim_x, int dim_y, int iters,
                        SorParams prm)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        l.d[c] = d_in[c];
        l.p[c] = p_io[c];
    }
    __syncthreads();
    sor_warm_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, iters, prm);   // (every pass ends behind a barrier)
    for (int c = threadIdx.x; c < cells; c += kThreads) p_io[c] = l.p[c];
}

// ---- the solve from zero stopped at a tolerance (sfl_poisson_solve_until): batch_solve_until_kernel for one grid ------
__global__ void __launch_bounds__(kThreads)
small_solve_until_kernel(float *__restrict__ p_out, const float *__restrict__ d_in, int dim_x, int dim_y, int cap,
                         SorParams prm, float tol, int every, unsigned *__restrict__ result)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    for (int c = threadIdx.x; c < cells; c += kThreads) l.d[c] = d_in[c];
    const UntilResult r = sor_until_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, cap, prm, tol, every);
    for (int c = threadIdx.x; c < cells; c += kThreads) p_out[c] = l.p[c];
    if (threadIdx.x == 0) {
        result[0] = r.norm_bits;
        result[1] = (unsigned)r.iters;
    }
}

// ---- one whole step, ino:252-287 -------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
small_step_kernel(SmallStep a)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#include "small_step_body.inc"
}

}  // namespace

bool small_grid_fits(int dim_x, int dim_y)
{
    return (int64_t)dim_x * dim_y <= kSmallGridMaxCells && (int64_t)dim_y * ((dim_x + 1) / 2) <= kCellsPerColour * kThreads;
}

hipError_t launch_small_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int iters, SorParams prm)
{
    static bool granted[64];
    const size_t lds = (size_t)dim_x * dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(small_solve_kernel), granted);
    if (e != hipSuccess) return e;
    small_solve_kernel<<<1, kThreads, lds, s>>>(p, d, dim_x, dim_y, iters, prm);
    return hipGetLastError();
}

hipError_t launch_small_solve_warm(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int iters, SorParams prm)
{
    static bool granted[64];
    const size_t lds = (size_t)dim_x * dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(small_solve_warm_kernel), granted);
    if (e != hipSuccess) return e;
    small_solve_warm_kernel<<<1, kThreads, lds, s>>>(p, d, dim_x, dim_y, iters, prm);
    return hipGetLastError();
}

hipError_t launch_small_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int cap, SorParams prm,
                                    float tol, int every, unsigned *result)
{
    static bool granted[64];
    const size_t lds = (size_t)dim_x * dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(small_solve_until_kernel), granted);
    if (e != hipSuccess) return e;
    small_solve_until_kernel<<<1, kThreads, lds, s>>>(p, d, dim_x, dim_y, cap, prm, tol, every, result);
    return hipGetLastError();
}

hipError_t launch_small_step(hipStream_t s, const SmallStep &a)
{
    static bool granted[64];
    const size_t lds = (size_t)a.dim_x * a.dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(small_step_kernel), granted);
    if (e != hipSuccess) return e;
    small_step_kernel<<<1, kThreads, lds, s>>>(a);
    return hipGetLastError();
}

}  // namespace sfl
