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
// Numerics contract: -ffp-contract=off, every operation individually rounded in the
// reference's order.  Reference citations are file:line under /root/reference/ESP32-fluid-simulation/.
#include "batch.h"
#include "small_grid_core.h"

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
// every workgroup size must own the same cells of one colour in total as small_grid.hip's 1024 threads: the batch
// accepts exactly the shapes small_grid_fits accepts
static_assert(cells_per_colour<kThreads>() * kThreads == kSmallGridMaxCells / 2, "SFL_BATCH_THREADS must divide 3072");

// ---- one whole step of member blockIdx.x, ino:252-287 ---------------------------------------------
__global__ void SFL_BATCH_BOUNDS
batch_step_kernel(BatchStep b)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const size_t member = blockIdx.x;
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

}  // namespace

hipError_t launch_batch_step(hipStream_t s, const BatchStep &a, int batch)
{
    static bool granted[64];
    const size_t lds = (size_t)a.step.dim_x * a.step.dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(batch_step_kernel), granted);
    if (e != hipSuccess) return e;
    batch_step_kernel<<<batch, kThreads, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_batch_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch, int iters,
                              SorParams prm)
{
    static bool granted[64];
    const size_t lds = (size_t)dim_x * dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(batch_solve_kernel), granted);
    if (e != hipSuccess) return e;
    batch_solve_kernel<<<batch, kThreads, lds, s>>>(p, d, dim_x, dim_y, iters, prm);
    return hipGetLastError();
}

}  // namespace sfl
