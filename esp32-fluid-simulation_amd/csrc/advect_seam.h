// advect_seam.h -- the kernel that joins two sim steps inside sfl_step_n (SFL_OPT_STEP_SEAMS): subtract_gradient + dye advection of
// step k and velocity advection + divergence of step k + 1 in one pass over memory.  Included by advect_tiled.hip (it uses that file's
// tile geometry, windows and sampling helpers); reference: ESP32-fluid-simulation.ino:249-289, finitediff.cpp:9-82, advect.h:24-85.
#pragma once

// ---- the seam between two steps -------------------------------------------------------------------------------
// Inside sfl_step_n the last kernel of step k (subtract_gradient + dye advection, ino:276 + ino:281-287) and the first
// kernel of step k + 1 (velocity advection + divergence, ino:252-256 + ino:274) are ONE kernel: the projected velocity of
// step k is the field step k + 1 advects, and apart from the dye's back-trace nobody else ever reads it -- so it is
// produced in LDS, on the window the advection needs (the pressure window is one cell wider), used by both halves and
// never written to memory: 8 B per cell less to write, the 74 x 42 window per tile less to read back.  Same arithmetic
// in the same order as the two kernels above (a back-trace that leaves a window projects the texels it needs on the fly
// from memory: the same expressions, so the same bits); whole-domain contexts.
constexpr int kPX = kDX + 2, kPY = kDY + 2;   // pressure window

// sample() (advect.h:37-72) of the PROJECTED velocity, texels projected on the fly from v and p in memory
template <bool NO_SLIP>
__device__ __forceinline__ float2 sample_global_projected(const float2 *v, const float *p, const Slab &g, const SrcPos &s,
                                                          float si, float sj, float two_dx_inv)
{
    const int i_max = g.dim_x - 1, j_max = g.gdim_y - 1;
    return sample_vec2f<NO_SLIP>(s, si, sj, g.dim_x, g.gdim_y, [&](int a, int b) {
        const int i = s.ci + a, gj = s.cj + b;
        return project_cell(v[lcell(g, i, gj)], i, gj, i_max, j_max, two_dx_inv,
                            [&](int pi, int pj) { return p[lcell(g, pi, pj)]; });
    });
}

// 512 threads; the register allocator leaves room for 6 waves per SIMD = three blocks per CU (80 VGPRs; two blocks at the 86 it
// would take by itself: 836 against 780 us; four blocks at 64 VGPRs spill: 1390 us)
#ifndef SEAM_THREADS
#define SEAM_THREADS 512
#endif
constexpr int kThreadsSeam = SEAM_THREADS;
template <int THREADS>
__global__ void __launch_bounds__(THREADS, 6)
seam_tiled_kernel(uint32_t *__restrict__ next_col, const uint32_t *col, float2 *__restrict__ next_v,
                  float *__restrict__ div, const float2 *v, const float *pressure, Slab g, TileGrid tg, float dt,
                  float two_dx_inv)
{
    constexpr int kWaves = THREADS / 64, kRows = kTY / kWaves;
    constexpr int kPlane = kSY * kSX;
    static_assert(kRing <= THREADS, "one ring cell per thread");
    constexpr int kWords = kPX * kPY + 2 * kDX * kDY;   // pressure window + velocity window, in 4-byte words
    static_assert(3 * kPlane <= kWords && kVX * kVY * 2 <= kWords, "one LDS buffer, tenants in turn");
    // ONE buffer (38.2 KB: four blocks per CU), used in turn by the pressure window + the projected velocity window of step
    // k, the dye window, and the advected velocities of step k + 1; what has to survive a change of tenant waits in
    // registers (the dye texels while the velocity is projected and advected, the advected cells while the dye is).
    __shared__ uint32_t lds[kWords];
    float *lds_p = reinterpret_cast<float *>(lds);
    float2 *lds_v = reinterpret_cast<float2 *>(lds + kPX * kPY);
    static_assert((kPX * kPY) % 2 == 0, "the velocity window starts 8-byte aligned");
    int tx, ty;
    if (!tile_of_block(tg, tx, ty)) return;
    const int x0 = tx * kTX, y0 = ty * kTY;
    const int i_max = g.dim_x - 1, j_max = g.gdim_y - 1;
    const Window wv = window_of<kRD>(x0, y0, g, 0, g.gdim_y);
    const Window wc = window_of<kR>(x0, y0, g, 0, g.gdim_y);
    const Window wp = window_of<kRD + 1>(x0, y0, g, 0, g.gdim_y);   // the pressure window is one cell wider than the velocity window
    {   // every load of the block in flight before the first LDS write
        float2 got_v[staged(kDX * kDY, THREADS)];
        float got_p[staged(kPX * kPY, THREADS)];
        stage_loads<kPX, kPY, THREADS>(got_p, wp, g, [&](size_t c) { return pressure[c]; });
        stage_loads<kDX, kDY, THREADS>(got_v, wv, g, [&](size_t c) { return v[c]; });
        stage_writes<kPX, kPY, THREADS>(lds_p, got_p);
        __syncthreads();
        // ino:276 on the velocity window: every thread projects the cells it loaded, pressure from LDS (five scattered loads
        // per window cell from memory cost 300 of the kernel's 970 us: profiles/r04_step_seam.txt)
#pragma unroll
        for (int k = 0; k < staged(kDX * kDY, THREADS); ++k) {
            const int e = threadIdx.x + k * THREADS;
            if (e >= kDX * kDY) break;
            float2 u = got_v[k];
            if (window_has<kDX>(wv, e)) {
                const int r = e / kDX, cx = e - r * kDX;
                u = project_cell(u, lds_p + (r + 1) * kPX + (cx + 1), kPX, wv.sx0 + cx, wv.sy0 + r, i_max, j_max, two_dx_inv);
            }
            lds_v[e] = u;
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = x0 + lane;
    const bool column = i < g.dim_x;
    // ino:252-256 of step k + 1: the projected velocity advects itself (no-slip), tile and the ring around it
    auto advected = [&](int ai, int agj) -> float2 {
        const float2 u = lds_v[(agj - wv.sy0) * kDX + (ai - wv.sx0)];
        const float si = (float)ai - u.x * dt;
        const float sj = (float)agj - u.y * dt;
        const SrcPos s = classify(si, sj, g.dim_x, g.gdim_y);
        return sample_window_vec2f<kDX>(lds_v, wv, s,
                                        [&] { return sample_global_projected<true>(v, pressure, g, s, si, sj, two_dx_inv); });
    };
    float2 mine[kRows], own[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int gj = y0 + wave + kWaves * r;
        mine[r] = own[r] = float2{0.0f, 0.0f};
        if (column && gj < g.gdim_y) {
            own[r] = lds_v[(gj - wv.sy0) * kDX + (i - wv.sx0)];   // the dye's back-trace below needs it
            mine[r] = advected(i, gj);
            next_v[lcell(g, i, gj)] = mine[r];
        }
    }
    const RingCell rc = ring_cell(threadIdx.x, x0, y0, g);
    float2 around = float2{0.0f, 0.0f};
    if (rc.inside) around = advected(rc.i, rc.gj);
    // The dye window is not needed before this point, and its 18 registers per thread are what pushed the kernel over the
    // 80 VGPRs that let three blocks share a CU: with every load of the block up front it spilled 9 registers (16 B of
    // scratch per thread = the 203 MB of writes nobody could explain in profiles/r04_sim_step_summary.txt).  Its loads are
    // issued HERE; the other two blocks of the CU cover their latency.
    uq3 got_c[staged(kSX * kSY, THREADS)];
    stage_loads<kSX, kSY, THREADS>(got_c, wc, g, [&](size_t c) { return load_uq3(col, c); });
    __syncthreads();   // everybody is done with the velocity window: the dye window moves in
    stage_writes<kSX, kSY, THREADS>(lds, got_c);
    __syncthreads();
    // ino:281-287: the dye of step k, back-traced with the cell's own projected velocity (free-slip)
    if (column) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int gj = y0 + wave + kWaves * r;
            if (gj >= g.gdim_y) break;
            const float2 u = own[r];
            const float si = (float)i - u.x * dt;
            const float sj = (float)gj - u.y * dt;
            const SrcPos s = classify(si, sj, g.dim_x, g.gdim_y);
            store_uq3(next_col, lcell(g, i, gj), sample_window_uq3<false, kSX, kSY>(lds, wc, col, g, s, si, sj));
        }
    }
    __syncthreads();   // everybody is done with the dye window: the advected velocities move in
    // ino:274 of step k + 1 (finitediff.cpp:9-39)
    divergence_of_parked<THREADS>(div, reinterpret_cast<float2 *>(lds), mine, rc, around, g, x0, y0, two_dx_inv);
}
