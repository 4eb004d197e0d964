// batch_play.hip -- `steps` consecutive sim steps of every member of a batch in ONE launch (gfx950 / MI355X): workgroup m
// runs member m through all of them and keeps its velocity in LDS from one step to the next.  batch_grid.hip's step
// kernels end the launch after every step: per member and step at 61 x 81 they read the velocity from memory by gathers
// (39 KB), write velocity, divergence and pressure back (79 KB) and cross a launch boundary, for values the same
// workgroup needs again at once.  That needs every force of those steps before the launch: the timeline of
// include/sfl.h (sfl_batch_queue_forces_at), staged as one CSR table with a row per (step, member) (batch.cpp).
//
// LDS: the 16 B per cell of batch_grid.hip as two regions A and B of 8 B per cell whose roles swap every step
// (large_member_core.h plays the same trick within one step).  In step k, with S the region that holds the step's
// source velocity and D the other one:
//
//   1  advect S -> D              a gather, so it cannot be in place; LDS reads through an LDS-typed pointer
//      BARRIER                    D is complete, nobody reads S any more
//   2  forces into D (thread 0)   BARRIER, where the member has records in this step
//   3  divergence of D -> d       d and p live in S, which is dead: d = the first half of S, p the second
//   4  solve: p = 0 | BARRIER | red-black SOR on p (a barrier behind every colour pass): small_grid_core.h sor_in_lds
//   5  per cell: D[c] <- D[c] - grad p (project_cell reads only the cell's own velocity: in place), the dye back-trace
//      with it
//      BARRIER                    D is the source of step k + 1; p and d may be overwritten
//
// Memory: the velocity is read once, before step 0, and velocity, divergence and pressure are stored in the last step
// only -- nothing can observe them in between.  The dye stays in memory and ping-pongs between col_in and col_out inside
// the kernel (the host swaps its pointers by the parity of `steps`).  Dye written in step k is gathered by OTHER threads
// of the same workgroup in step k + 1, and the buffer step k gathered from is overwritten in step k + 1: the
// __syncthreads() that ends phase 5 stands between the two and orders them at workgroup scope (a release of the
// workgroup's global stores in front of the barrier, an acquire behind it).  No workgroup reads another's dye, so nothing
// wider is needed.
//
// Parameters come per member from BatchMember records as in batch_grid.hip's *_each kernels (scalar loads; the host lists
// the members with the most iterations first), or once for all from the launch's arguments (members == nullptr).  With
// records the kernel ends with the member's update norm, taken from the p and d the last solve left in LDS.
// Workgroup shape and register budget are batch_grid.hip's.  The arithmetic is small_grid_core.h / advect_math.h, each
// stencil written once: every field ends up bit for bit where `steps` launches of batch_step[_each]_kernel leave it.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#include "batch_member.h"

namespace sfl {
namespace {

using namespace batch_member;   // (the workgroup's shape, apply_member)

__global__ void SFL_BATCH_BOUNDS
batch_play_kernel(BatchPlay b, int batch, const BatchMember *__restrict__ members, float *__restrict__ report)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    SmallStep a = b.step;
    size_t member = blockIdx.x;
    if (members) {   // workgroup-uniform: scalar loads
        const BatchMember q = members[blockIdx.x];
        member = (size_t)q.member;
        apply_member(a, q);
    }
    const size_t base = member * (size_t)a.dim_x * (size_t)a.dim_y;   // 64-bit: cells before this member
    float2 *const lds_v = reinterpret_cast<float2 *>(lds_raw);   // region A at cell 0, region B at cell `cells`
    uint32_t *col_src = const_cast<uint32_t *>(a.col_in) + 3 * base, *col_dst = a.col_out + 3 * base;

    {   // the velocity the launch starts from -> region A
        const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in) + base;
        for (int c = threadIdx.x; c < a.dim_x * a.dim_y; c += kThreads) lds_v[c] = v_in[c];
    }
    __syncthreads();

    for (int k = 0; k < b.steps; ++k) {
        const bool last = k + 1 == b.steps;
        // The shape, as far as the compiler can tell, is another one in every step: what a step derives from it (the
        // solve's cells, masks and constants above all) is then formed in that step, as in a launch per step, and not
        // hoisted in front of the loop and kept alive -- spilled -- across every phase of every step.
        int dim_x = a.dim_x, dim_y = a.dim_y;
        asm volatile("" : "+s"(dim_x), "+s"(dim_y));
        const int cells = dim_x * dim_y, i_max = dim_x - 1, j_max = dim_y - 1;
        const Slab g{dim_x, dim_y, 0, dim_y};
        const int s_at = (k & 1) ? cells : 0;
        const float2 *vs = lds_v + s_at;             // S: the source velocity
        float2 *vd = lds_v + (cells - s_at);         // D: advected, then projected
        float *d = reinterpret_cast<float *>(lds_v + s_at), *p = d + cells;   // in S, once it is dead

        // 1  advect(v_next, v, v, dt, no_slip): ino:252-256, advect.h:78-84
        lds_cfloat *vs_lds = (lds_cfloat *)(lds_raw + (size_t)s_at * 8);
        for (int c = threadIdx.x; c < cells; c += kThreads) {
            const int gj = c / dim_x, i = c - gj * dim_x;
            const float2 u = vs[c];
            const float si = (float)i - u.x * a.dt;
            const float sj = (float)gj - u.y * a.dt;
            const SrcPos s = classify(si, sj, dim_x, dim_y);
            vd[c] = sample_lds_vec2f<true>(vs_lds, g, s, si, sj);
        }
        __syncthreads();
        // 2  drag forces of this step, in queue order: later entries win (ino:264-269)
        int f0 = 0, f1 = 0;
        if (b.force_rows && k < b.rows) {   // this member's row of step k
            const int *row = b.force_rows + (size_t)k * (size_t)batch;
            f0 = row[member];
            f1 = row[member + 1];
        }
        if (f1 > f0) {
            if (threadIdx.x == 0)
                for (int f = f0; f < f1; ++f) {
                    const int i = a.force_cells[2 * (size_t)f], gj = a.force_cells[2 * (size_t)f + 1];
                    if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                    vd[gj * dim_x + i] = make_float2(a.force_vel[2 * (size_t)f], a.force_vel[2 * (size_t)f + 1]);
                }
            __syncthreads();
        }
        // 3  calculate_divergence: ino:274, finitediff.cpp:9-39
        for (int c = threadIdx.x; c < cells; c += kThreads) {
            const int gj = c / dim_x, i = c - gj * dim_x;
            const float dv = divergence_sum(vd + c, dim_x, i, gj, i_max, j_max) * a.two_dx_inv;
            d[c] = dv;
            if (last) a.div[base + c] = dv;
        }
        // 4  poisson_solve: ino:275 (the barrier inside also orders the divergence writes above)
        sor_in_lds<kThreads>(p, d, dim_x, dim_y, a.iters, a.prm);
        // 5  subtract_gradient (ino:276, finitediff.cpp:41-82) in place, then the dye back-trace with the projected
        //    velocity of the cell itself (ino:281-287, advect.h:81)
        for (int c = threadIdx.x; c < cells; c += kThreads) {
            const int gj = c / dim_x, i = c - gj * dim_x;
            const float pc = p[c];
            const float2 u = project_cell(vd[c], p + c, dim_x, i, gj, i_max, j_max, a.two_dx_inv);
            vd[c] = u;
            if (last) {
                reinterpret_cast<float2 *>(a.v_out)[base + c] = u;
                a.p[base + c] = pc;
            }
            const float si = (float)i - u.x * a.dt;
            const float sj = (float)gj - u.y * a.dt;
            const SrcPos s = classify(si, sj, dim_x, dim_y);
            store_uq3(col_dst, (size_t)c, sample_global_uq3<false>(col_src, g, s, si, sj));
        }
        if (last) {
            // (the loop above only reads p; p and d are final since the solve's last barrier)
            if (report) update_norm_in_lds<kThreads>(p, d, dim_x, dim_y, a.prm.dx, report + member);
        } else {
            uint32_t *const t = col_src;
            col_src = col_dst;
            col_dst = t;
            __syncthreads();   // D -> S of the next step; the dye of this step -> the gathers of the next (see the top)
        }
    }
}

}  // namespace

hipError_t launch_batch_play(hipStream_t s, const BatchPlay &a, int batch, const BatchMember *members, float *report)
{
    static bool granted[64];
    const size_t lds = (size_t)a.step.dim_x * a.step.dim_y * 16;
    hipError_t e = allow_small_grid_lds(reinterpret_cast<const void *>(batch_play_kernel), granted);
    if (e != hipSuccess) return e;
    batch_play_kernel<<<batch, kThreads, lds, s>>>(a, batch, members, members ? report : nullptr);
    return hipGetLastError();
}

}  // namespace sfl
