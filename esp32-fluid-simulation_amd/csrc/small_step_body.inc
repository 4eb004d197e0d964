// small_step_body.inc -- the body of the one-workgroup step kernels (ino:252-287), included INSIDE a kernel by small_grid.hip
// (small_step_kernel: one grid per launch) and batch_grid.hip (one grid per workgroup).  What the including kernel has
// in scope: `a`, the SmallStep of its grid (every pointer at that grid's first cell), `lds_raw`, its dynamic LDS (16 B
// per cell), `kThreads`, its workgroup size, and sfl::small_core (small_grid_core.h).  A text, not a function: with the
// body inlined from a function the compiler schedules small_step_kernel differently, and its instructions must not
// change with this sharing (the same instructions, in the same order, as before batch_grid.hip existed).
// Offsets inside the grid are 32-bit ints (at most kSmallGridMaxCells cells).
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y;
    const Lds l = carve(lds_raw, cells);
    const Slab g{dim_x, dim_y, 0, dim_y};
    const float2 *v_in = reinterpret_cast<const float2 *>(a.v_in);
    float2 *v_out = reinterpret_cast<float2 *>(a.v_out);

    // advect(v_next, v, v, dt, no_slip): ino:252-256, advect.h:78-84
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float2 u = v_in[c];
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        l.v[c] = sample_global_vec2f<true>(v_in, g, s, si, sj);
    }
    __syncthreads();
    // drag forces, in queue order: later entries win (ino:264-269)
    if (a.n_forces > 0) {
        if (threadIdx.x == 0)
            for (int k = 0; k < a.n_forces; ++k) {
                const int i = a.force_cells[2 * k], gj = a.force_cells[2 * k + 1];
                if (i < 0 || i >= dim_x || gj < 0 || gj >= dim_y) continue;
                l.v[gj * dim_x + i] = make_float2(a.force_vel[2 * k], a.force_vel[2 * k + 1]);
            }
        __syncthreads();
    }
    // calculate_divergence: ino:274, finitediff.cpp:9-39
    const int i_max = dim_x - 1, j_max = dim_y - 1;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float dv = divergence_sum(l.v + c, dim_x, i, gj, i_max, j_max) * a.two_dx_inv;
        l.d[c] = dv;
        a.div[c] = dv;
    }
    // poisson_solve: ino:275 (the barrier inside also orders the divergence writes above).  A kernel whose solve is
    // another one names it in SFL_STEP_SOLVE before it includes this text (batch_grid.hip: the solve to a tolerance)
#ifdef SFL_STEP_SOLVE
    SFL_STEP_SOLVE;
#else
    sor_in_lds<kThreads>(l.p, l.d, dim_x, dim_y, a.iters, a.prm);
#endif
    // subtract_gradient (ino:276, finitediff.cpp:41-82), then the dye back-trace with the projected velocity of
    // the cell itself (ino:281-287, advect.h:81) -- per cell, no barrier needed in between
    const uint32_t *col_in = a.col_in;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int gj = c / dim_x, i = c - gj * dim_x;
        const float pc = l.p[c];
        const float2 u = project_cell(l.v[c], l.p + c, dim_x, i, gj, i_max, j_max, a.two_dx_inv);
        v_out[c] = u;
        a.p[c] = pc;
        const float si = (float)i - u.x * a.dt;
        const float sj = (float)gj - u.y * a.dt;
        const SrcPos s = classify(si, sj, dim_x, dim_y);
        store_uq3(a.col_out, (size_t)c, sample_global_uq3<false>(col_in, g, s, si, sj));
    }
