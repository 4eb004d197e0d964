/*
 * sfl.h -- C ABI of the MI355X-native stable-fluids hot path ("sfl").
 *
 * This is the drop-in boundary for the sim-task arithmetic of
 * colonelwatch/ESP32-fluid-simulation.  Every entry point is `extern "C"`, takes
 * plain pointers / sizes / scalars and returns an int status (0 = SFL_OK, <0 = error,
 * text via sfl_last_error()).  The reference's own functions return void and check
 * nothing; the C++ drop-in headers in include/sfl/ keep those
 * exact signatures on top of this ABI.
 *
 * Citations are file:line under /root/reference/ESP32-fluid-simulation/.
 *
 * Data layout (identical to the reference, operations.h:7-9): element (i, j) of a
 * dim_x * dim_y field at index dim_x*j + i, i fastest.  Velocity = interleaved
 * {x, y} float32 (Vector2<float>, vector.h:4-57, 8 B); dye = interleaved {x, y, z}
 * uint32 raw values (Vector3<UQ32>, vector.h:63-122 + uq32.h:8-16, 12 B);
 * pressure / divergence = float32.
 *
 * Four groups of entry points:
 *   1. host-pointer drop-ins  sfl_host_*      the reference signatures + status; upload,
 *                                             run the HIP kernels, download (parity / porting aid)
 *   2. solver contexts        sfl_create ...  device-resident fields for one GPU's row slab of
 *                                             the domain, operators, RCCL halo exchange
 *   3. utilities              version, errors, device query, slab partition arithmetic
 *   4. batches                sfl_batch_*     many independent small grids of one shape on one
 *                                             device, stepped by one launch
 *
 * There is NO CPU fallback anywhere behind this header: without a usable GPU every
 * compute entry point fails with SFL_ERR_HIP.
 */
#ifndef SFL_H
#define SFL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFL_API __attribute__((visibility("default")))

#define SFL_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------------- */
#define SFL_OK 0
#define SFL_ERR_INVALID (-1) /* bad argument: NULL, dim < 2, iters < 0, aliasing rule broken   */
#define SFL_ERR_HIP (-2)     /* HIP runtime / no device / kernel launch failure               */
#define SFL_ERR_RCCL (-3)    /* RCCL failure                                                  */
#define SFL_ERR_NOMEM (-4)   /* device or host allocation failed                              */
#define SFL_ERR_STATE (-5)   /* call not valid in this context state (e.g. comm not attached) */
#define SFL_ERR_HALO (-6)    /* a back-trace left the slab's advect halo (multi-GPU only)     */

/* ---- field identifiers of a context ----------------------------------------------- */
#define SFL_FIELD_VELOCITY 0   /* Vector2<float>  velocity_field (ino:54)                    */
#define SFL_FIELD_COLOR 1      /* Vector3<UQ32>   color_field    (ino:55)                    */
#define SFL_FIELD_DIVERGENCE 2 /* float           div_v          (ino:272)                   */
#define SFL_FIELD_PRESSURE 3   /* float           p              (ino:273)                   */

/* ---- tunables (sfl_set_option / sfl_get_option) ------------------------------------------ */
#define SFL_OPT_SOR_KERNEL 0      /* 0 = auto, 1 = one launch per colour pass (baseline kernel),
                                     2 = fused multi-pass streaming kernel.  Both give the reference's
                                     bits on every input (unless SFL_OPT_SOR_FOLD is set)          */
#define SFL_OPT_SOR_FUSE 1        /* colour passes fused per launch by kernel 2: even, 2..16, or
                                     0 = auto (16 on slabs of >= 12 M cells, 10 from 3 M, else 8) */
#define SFL_OPT_ADVECT_HALO 2     /* slabs: rows of the advected field exchanged per side.  0 (default) =
                                     automatic, correct for any velocity: sfl_step sizes the velocity
                                     advection's halo from the reach measured at the end of the previous
                                     step (the same velocity, the same dt: exact), runs the dye advection
                                     on that reach plus a margin and checks it AFTER the step -- a flag and
                                     the true reach travel to the host asynchronously and are examined by
                                     the next call on the context, which repeats the dye advection alone
                                     (from the untouched old buffer) if a back-trace left the guess; no
                                     host round trip inside a step.  The stand-alone sfl_advect_* operators
                                     and a step after the velocity was written from outside measure first
                                     (one host round trip); beyond 64 rows the field is gathered on every
                                     GPU.  1..64 = fixed: a back-trace that leaves them is reported as
                                     SFL_ERR_HALO by sfl_synchronize                                      */
#define SFL_OPT_SOR_ROWS 3        /* output rows per wave tile of kernel 2 (0 = auto)            */
#define SFL_OPT_TRANSPORT 4       /* READ ONLY: 0 = none (whole domain / not attached yet),
                                     1 = RCCL (sfl_comm_attach), 2 = in-process (sfl_group_link),
                                     3 = emulated (sfl_comm_emulate: timing only), 4 = emulated with RCCL
                                     messages to the rank itself (sfl_comm_emulate_rccl: timing only) */
#define SFL_OPT_SOR_LANE_CELLS 5  /* cells per lane of kernel 2: 0 = auto or 2 (the only flavour
                                     left: round 1's packed 4-cell tiles were never faster)        */
#define SFL_OPT_SOR_HALO 6        /* rows of p a superstep's halo makes valid on a slab (kernel 2): 0 =
                                     auto, else fuse..160; larger = fewer, larger exchanges, more recomputed
                                     ghost rows; from 2 x fuse on, exchanges behind events are issued one launch
                                     early (sfl_plan_poisson).  Auto starts from 64 rows on slabs of >= 1024 rows
                                     (32 on thinner ones) and moves to another depth when a model of the solve --
                                     redundant rows against exchanges at their MEASURED cost,
                                     SFL_OPT_MEASURED_WIRE_US -- names another candidate: the first 12 solves of a
                                     kind (same iterations, fuse depth, schedule) then run on the candidates in
                                     turn between pairs of events, the 13th waits for them (one host
                                     hipEventSynchronize) and keeps the fastest (SFL_OPT_LAST_HALO reads what a
                                     solve used).  Same bits at every depth; a caller who times fewer than 13
                                     solves of a kind times the exploration -- or sets a depth                */
#define SFL_OPT_FUSE_PROJECTION 7 /* sfl_step only: 1 (default) = subtract_gradient is applied
                                     inside the dye-advection kernel (one pass over v), 0 = two
                                     kernels                                                     */

#define SFL_OPT_ADVECT_KERNEL 9   /* advection, divergence and gradient kernels: 0 = auto, 1 = one
                                     thread per cell reading its neighbours / texels from memory,
                                     2 = the window of a 64 x 32-cell tile staged in LDS (auto = 2
                                     from 16384 cells per launch); same results                  */
#define SFL_OPT_FUSE_DIVERGENCE 10 /* sfl_step only: 1 (default) = on a whole-domain context with no
                                     queued forces and advection kernel 2, the velocity advection
                                     and calculate_divergence run as one kernel (the advected tile
                                     is differenced in LDS); 0 = two kernels                       */
#define SFL_OPT_SMALL_GRID 11      /* 1 (default) = on a whole-domain context of at most 6144 cells
                                     whose kernel options are all automatic, sfl_poisson_solve and
                                     sfl_step run as ONE launch of one workgroup with the fields in
                                     LDS (the sketch's 61 x 81 grid: one launch instead of six to
                                     ten); 0 = the general kernels                                 */
#define SFL_OPT_EMULATE_WIRE_US 12 /* sfl_comm_emulate / sfl_comm_emulate_rccl only (measurement aid): every emulated halo message is held
                                     back by this many microseconds on the exchange stream before its copy
                                     starts -- the latency of a real xGMI send / receive that a self-copy does
                                     not have; 0 (default) .. 10000                                   */
#define SFL_OPT_STEP_SEAMS 14      /* sfl_step_n on a whole-domain context with the tile kernels: 1 (default) = between two steps
                                     subtract_gradient + dye advection of one and velocity advection + divergence of the
                                     next run as ONE kernel (the projected velocity in between is never written to memory);
                                     0 = n times sfl_step.  Same results either way                              */
#define SFL_OPT_LAST_EARLY_ROWS 17 /* READ ONLY: slabs on the automatic advection halo: L > 0 when the last sfl_step kept the velocity
                                     advection of the rows further than L from both cuts that it had queued BEFORE reading the
                                     previous step's report (they need no halo; the report says whether that held); 0 = the step
                                     advected everything after the report                                            */

#define SFL_OPT_HALO_TIMEOUT_MS 18  /* limit of a wait INSIDE a launch or on the exchange stream (SFL_OPT_EXCHANGE_SCHEDULE = 3),
                                     milliseconds: 0 (default) = the transport's own: 2 s where every party is this process
                                     (virtual ranks, emulated ranks), 300 s on RCCL ranks -- a peer process may simply be late
                                     (I/O, a garbage collection), and what used to be an event wait must not become an error */
#define SFL_OPT_EXCHANGE_SCHEDULE 19 /* slabs, kernel 2: how a solve orders its halo exchanges -- ONE option for what rounds 2 - 5 spread over
                                     SFL_OPT_SOR_OVERLAP (8), SFL_OPT_SOR_ARRIVAL (13) and SFL_OPT_SOR_CHAIN (15; the chained launch was
                                     retired in round 6), whose numbers are no longer accepted.  All schedules give the same bits.
                                     SET: 0 (default) = automatic: 3 on virtual and emulated ranks, 2 on RCCL ranks whose peers are
                                          other processes (a launch that waits inside the kernel is only as safe as its peer is
                                          punctual, and the scheme has not run on more than one GPU yet: tools/first_multi_gpu.sh);
                                          2 wherever the context's compute and exchange stream were found NOT to run side by side
                                          (measured once, at attach / first solve; RCCL ranks agree on it collectively);
                                       1 = in line: every launch whole, every exchange awaited on the compute stream;
                                       2 = one launch early, behind cross-stream events (round 3): a superstep's halo travels on the
                                          exchange stream while the owned rows of that launch are relaxed, its ghost rows are relaxed
                                          behind the message, the launch after waits whole (halo >= 2 x fuse; shallower halos and the
                                          right-hand side's exchange are awaited in line);
                                       3 = in time, counted on the device (sfl_plan_poisson kernel 3): the halo is exchanged after the
                                          launch that produces it; that launch runs the tiles whose rows the message carries at the
                                          top priority, writes through, and counts them; the message leaves on that count while the
                                          rest of the launch is still running; the next launch is queued at once and only its tiles
                                          next to a cut wait, INSIDE the launch, for a count of arrived messages.  A wait that outlasts
                                          SFL_OPT_HALO_TIMEOUT_MS gives up; sfl_synchronize reports it, sfl_download and the next
                                          operator on the context fail instead of handing out / building on an invalid field.
                                     GET: what the next solve will do: 0 = nothing to order (whole domain, no transport, the baseline
                                          kernel), else 1 / 2 / 3 with the automatic choice and the streams' verdict resolved        */
#define SFL_OPT_MEASURED_WIRE_US 20  /* READ ONLY: slabs with a transport: microseconds one halo exchange of this context costs before
                                     its first byte moves (launches, protocol, wire), measured -- not assumed -- with
                                     back-to-back exchanges of p at two depths when the transport was attached (RCCL ranks:
                                     the maximum over the ranks) or in front of the first solve (virtual / emulated ranks: the
                                     copy, and SFL_OPT_EMULATE_WIRE_US if set); -1 = nothing to measure, or not measured yet
                                     (the query itself never measures: that is a collective of the ranks and belongs to a solve).  The automatic halo depth of a
                                     solve (SFL_OPT_SOR_HALO = 0) is chosen from it: deeper halos = fewer exchanges, more rows
                                     relaxed redundantly                                                             */
#define SFL_OPT_LAST_HALO 21         /* READ ONLY: halo depth (rows of p per superstep) of the last solve's plan on this slab  */
#define SFL_OPT_SOR_FOLD 22          /* kernel 2's interior relaxation, poisson.cpp:107-111.  0 (default) = as the reference writes it,
                                     (1 - omega) * p + omega * (-0.25f * t), t = dx * d - sum: every product rounded on its own, the
                                     reference's bits on EVERY input.  1 = (1 - omega) * p + (-0.25f * omega) * t: one product less (7
                                     instead of 8 vector instructions per cell and pass, measured +2.4 .. 3 % cell-iters/s at 8192^2).
                                     The same bits wherever every operand of t (dx * d and the four neighbours' p) is zero or at least
                                     2^-124 = 4.7e-38 in magnitude -- dense fields.  Where one is a nonzero number below that -- the
                                     decaying front of a sparsely forced solution in a quiescent region reaches that range after ~63
                                     iterations: the sketch's own scenario -- the reference rounds -0.25f * t to a denormal first and
                                     the folded product can differ by one unit of 2^-149.  After ONE solve only cells of that front
                                     differ (absolute differences <= ~1e-40).  Over repeated sim steps the difference climbs the scales
                                     of a field that holds every magnitude down to the denormals, and pressure and velocity end up with
                                     ordinary rounding noise against the reference (units in the last place of each value; 1e-8 of the
                                     field's maximum after three steps at 80 iterations) -- inside north_star's 1e-5, but not the
                                     reference's bits.  Opt in only if that is acceptable; the boundary cells keep both products
                                     either way (tests/test_gpu_parity.py test_quiescent_*)                        */

typedef struct sfl_context sfl_context;
typedef struct sfl_batch sfl_batch;

/* =====================================================================================
 * 3. utilities
 * ===================================================================================== */
SFL_API int sfl_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
SFL_API const char *sfl_last_error(void);
/* Number of visible HIP devices (0 and SFL_ERR_HIP when there is none). */
SFL_API int sfl_device_count(int *count);
/* Name / CU count / memory of a device; any out pointer may be NULL. */
SFL_API int sfl_device_info(int device, char *name, size_t name_cap, int *compute_units,
                            size_t *total_mem_bytes);

/* Row-slab partition of dim_y rows over nranks: rank g owns global rows
 * [dim_y*g/nranks, dim_y*(g+1)/nranks).  Pure arithmetic, no GPU needed.                */
SFL_API int sfl_slab_rows(int dim_y, int nranks, int rank, int *row_begin, int *row_end);

/* One step of a rank's program (sfl_plan_poisson): either a halo exchange with both
 * neighbouring slabs or a compute launch.  Row ranges are GLOBAL rows.                        */
typedef struct sfl_plan_step {
    int32_t kind;         /* SFL_STEP_*                                                       */
    int32_t field;        /* EXCHANGE: SFL_FIELD_* whose halo rows are refreshed              */
    int32_t rows;         /* EXCHANGE: rows per side (sent from / received next to the owned
                             block); 0 on compute steps                                       */
    int32_t g_begin;      /* compute: first output row (may extend into the ghost rows).
                             EXCHANGE: depth of the first row exchanged, counted from the cut
                             (0 = the rows next to it): each rank sends its owned rows at depth
                             [g_begin, g_begin + rows) and receives the neighbour's into the ghost
                             rows at the same depth; the ghost rows nearer the cut are still valid */
    int32_t g_end;        /* compute: one past the last output row                            */
    int32_t nsweeps;      /* SOR: colour passes executed by this launch.  Pass j (1-based)
                             covers rows [g_begin-(nsweeps-j), g_end+(nsweeps-j)) clipped to
                             the domain, i.e. halo rows are recomputed redundantly so that
                             the output rows are exact                                        */
    int32_t first_colour; /* SOR: colour of pass 1 (0 = even (i+j), poisson.cpp:22)           */
    int32_t from_zero;    /* SOR: p is implicitly zero on entry (poisson.cpp:117-119)         */
} sfl_plan_step;

#define SFL_STEP_EXCHANGE 1 /* refresh `rows` ghost rows per side of `field`                   */
#define SFL_STEP_SOR 2      /* nsweeps colour passes -> output rows [g_begin, g_end)           */
#define SFL_STEP_ZERO 3     /* zero-fill p on every local row (baseline kernel only)           */

/* Program of one poisson_solve on slab `rank` of `nranks`: kernel = 1 (one colour pass per
 * launch, 1-row exchange before every pass but the first) or 2 (fused: `fuse` passes per
 * launch; launches are grouped into supersteps of at most `halo` passes in total, with ONE
 * exchange of p per superstep but the first -- ghost rows are recomputed redundantly in
 * between -- plus one exchange of the right-hand side up front).
 * halo is clamped to >= fuse; halo == fuse exchanges before every launch.
 * halo >= 2 * fuse: EARLY exchanges.  The exchange of a superstep is issued one launch early,
 * before the LAST launch of the previous superstep, while the ghost rows are still valid as deep
 * as that launch needs for the owned rows (EXCHANGE.g_begin = its nsweeps, rows = halo - nsweeps);
 * that launch's output extends `what the next superstep needs` into the ghost rows, i.e. its passes
 * are repeated on the received rows.  An executor may run the owned rows of that launch while the
 * message travels and the ghost rows behind it (csrc/sor_executor.cpp run_poisson_early does).
 * Writes at most `cap` steps, returns the total in *n_steps.  Pure arithmetic, no GPU needed;
 * the GPU executor walks exactly this program.                                               */
SFL_API int sfl_plan_poisson(int dim_y, int nranks, int rank, int iters, int fuse, int kernel,
                             int halo, sfl_plan_step *steps, int cap, int *n_steps);
/* kernel = 3: kernel 2's launches with IN-TIME exchanges at every halo depth -- never early: the exchange of a superstep
 * follows the launch that produces its rows (SFL_OPT_EXCHANGE_SCHEDULE = 3; with a tail every superstep holds halo - tail passes and its
 * exchange skips the `tail` ghost rows the launch before left exact).                                                    */
/* The same with a TAIL: `tail` ghost rows of p are still exact when the solve ends (every launch of an
 * early-exchange plan then extends that much further into the ghost rows; ignored -- as 0 -- by the other
 * plans).  sfl_step on slabs asks for 1, the row subtract_gradient (finitediff.cpp:41-82) reads beyond a
 * cut, and so needs no exchange of p between the solve and the projection.                          */
SFL_API int sfl_plan_poisson_tail(int dim_y, int nranks, int rank, int iters, int fuse, int kernel,
                                  int halo, int tail, sfl_plan_step *steps, int cap, int *n_steps);

/* Pass plan of one poisson_solve: 2*iters half-sweeps are executed as `*n_passes` launches of
 * at most `fuse` half-sweeps each (the last one may be shorter); passes[k] receives the
 * number of half-sweeps of launch k when passes != NULL (capacity cap).  How these launches
 * interleave with halo exchanges on a slab is sfl_plan_poisson's business.  Pure arithmetic,
 * no GPU needed.                                                                            */
SFL_API int sfl_sor_pass_plan(int iters, int fuse, int *n_passes, int *passes, int cap);

/* =====================================================================================
 * 1. host-pointer drop-ins: the reference's operator signatures + int status.
 *    Pointers are HOST memory; each call uploads, runs the HIP kernels on `device 0`
 *    (or SFL_DEVICE from the environment) and downloads.  Intended for parity tests and as
 *    the first step of a port; production callers keep fields on the device (group 2).
 * ===================================================================================== */

/* advect<Vector2<float>, float>   advect.h:74-85 (sample :24-72).  next_p must not alias p;
 * p may alias vel (self-advection, ino:253).                                               */
SFL_API int sfl_host_advect_vec2f(float *next_p, const float *p, const float *vel, int dim_x,
                                  int dim_y, float dt, int no_slip);
/* advect<Vector3<UQ32>, float>    advect.h:74-85 with uq32.h:13,15 (ino:282)               */
SFL_API int sfl_host_advect_vec3uq32(uint32_t *next_p, const uint32_t *p, const float *vel,
                                     int dim_x, int dim_y, float dt, int no_slip);
/* advect<T, float>                advect.h:74-85 for EVERY element type the reference's headers can express:
 * T = `channels` (1..3) consecutive 32-bit channels of one `kind` -- float, Vector2<float>, Vector3<float>
 * (SFL_CHANNEL_F32) or UQ32, Vector2<UQ32>, Vector3<UQ32> (SFL_CHANNEL_UQ32; vector.h:4-126, uq32.h:8-16).
 * sample() (advect.h:24-72) acts channel by channel on all of them; the sketch's two instantiations
 * (2 x f32, 3 x uq32) take the same kernels as the two entry points above.                     */
#define SFL_CHANNEL_F32 0
#define SFL_CHANNEL_UQ32 1
SFL_API int sfl_host_advect_channels(void *next_p, const void *p, const float *vel, int dim_x, int dim_y,
                                     float dt, int no_slip, int channels, int kind);
/* calculate_divergence            finitediff.h:6-7, finitediff.cpp:9-39                     */
SFL_API int sfl_host_calculate_divergence(float *div, const float *v, int dim_x, int dim_y,
                                          float dx);
/* subtract_gradient (in place)    finitediff.h:9-10, finitediff.cpp:41-82                   */
SFL_API int sfl_host_subtract_gradient(float *v, const float *p, int dim_x, int dim_y, float dx);
/* poisson_solve                   poisson.h:4-5, poisson.cpp:114-125                        */
SFL_API int sfl_host_poisson_solve(float *p, const float *div, int dim_x, int dim_y, float dx,
                                   int iters, float omega);
/* The operators above never retain caller pointers (as the reference: finitediff.cpp:36,78-79,
 * poisson.cpp:120 keep their contexts on the stack).  For grids of up to 2^26 cells (8192^2) they do keep
 * their device-side working context with the calling thread between calls, so that a loop() of
 * five operators per frame (ino:252-287) does not set up streams and buffers five times per
 * frame; this releases it (optional; also replaced whenever the grid shape changes).          */
SFL_API int sfl_host_release(void);

/* =====================================================================================
 * 2. solver contexts: one context = one GPU's row slab, fields resident in HBM.
 * ===================================================================================== */

/* Whole domain on one device (rank 0 of 1). */
SFL_API int sfl_create(sfl_context **out, int device, int dim_x, int dim_y);
/* Limits: dim_x, dim_y >= 2; at most 2^30 cells per domain and 2^28 cells (owned + 128 ghost rows
 * on a slab) per context -- the kernels address a context's arrays with 32-bit byte offsets;
 * larger domains need more slabs.  Violations return SFL_ERR_INVALID before any GPU is touched.  */
/* Row slab `rank` of `nranks` (sfl_slab_rows) of a dim_x * dim_y domain on `device`.
 * Neighbouring slabs exchange halos through RCCL once sfl_comm_attach() has run, or through
 * in-process copies when the contexts were joined with sfl_group_link().                    */
SFL_API int sfl_create_slab(sfl_context **out, int device, int dim_x, int dim_y, int rank,
                            int nranks);
SFL_API int sfl_destroy(sfl_context *ctx);

/* Options of contexts joined by sfl_group_link are group-wide (setting one member sets all; linking
 * aligns the members with slab 0).  RCCL ranks are separate processes: set the same values on each. */
SFL_API int sfl_set_option(sfl_context *ctx, int option, int value);
SFL_API int sfl_get_option(sfl_context *ctx, int option, int *value);

/* Geometry of this context's slab: global rows [row_begin, row_end). */
SFL_API int sfl_slab_of(sfl_context *ctx, int *row_begin, int *row_end, int *rank, int *nranks);

/* --- RCCL bootstrap: rank 0 creates the id, the launcher distributes the bytes (e.g.
 *     torch.distributed broadcast), every rank attaches.  id_bytes = 128.                  */
SFL_API int sfl_comm_unique_id(void *id_out, size_t id_bytes);
SFL_API int sfl_comm_attach(sfl_context *ctx, const void *id, size_t id_bytes);
/* Collective over the attached communicator (called by sfl_comm_attach itself; call it again after changing
 * options): all-gathers domain, group size and every option the solve's program depends on, and fails with
 * SFL_ERR_STATE on the ranks that differ from any other -- mismatched programs would otherwise hang in a
 * send / receive or exchange the wrong rows.  Synchronises the context's streams.                       */
SFL_API int sfl_comm_check_options(sfl_context *ctx);
/* RCCL bring-up check for boxes with a single GPU (a communicator cannot hold two ranks of one
 * device): inside one ncclGroup, send the first `rows` owned rows of the divergence field to
 * this rank itself and receive them into the first `rows` owned rows of the pressure field --
 * the same pointer / count / stream arithmetic as a neighbour halo exchange.                  */
SFL_API int sfl_comm_loopback(sfl_context *ctx, int rows);
/* Measurement aid for boxes with fewer GPUs than ranks: this slab context runs ITS rank's program alone.
 * Every halo message it would send is copied -- same size, same stream, same ordering events -- into the
 * ghost rows it would receive into, so launches, copies and their overlap are exactly the rank's own while
 * the values next to the cuts are meaningless (never use the results).  SFL_OPT_TRANSPORT reads 3.
 * bench.py --emulate-rank R --of N reports the time of one solve on such a context.                 */
SFL_API int sfl_comm_emulate(sfl_context *ctx);
/* The same rank program with RCCL ITSELF as the transport: a one-rank communicator is created for the context and every halo
 * message becomes a real ncclSend / ncclRecv of this rank to itself, issued through the very code path a rank of a real
 * communicator takes (one ncclGroup per exchange on the exchange stream, the sender count in front of it and the arrival
 * count behind it when exchanges are counted on the device); the step's reductions over the ranks run as ncclAllReduce on
 * that communicator.  What one GPU can show of the multi-GPU path: RCCL's own kernels beside the solve's launches, their
 * launch latency, their stream semantics.  SFL_OPT_TRANSPORT reads 4; values next to the cuts are meaningless.
 * bench.py --emulate-rank R --of N --via-rccl.                                                                     */
SFL_API int sfl_comm_emulate_rccl(sfl_context *ctx);
/* In-process transport between virtual ranks living on ONE device (bring-up / tests):
 * ctxs[r] must be slab r of nranks == n, all created on the same device.                   */
SFL_API int sfl_group_link(sfl_context **ctxs, int n);

/* --- field I/O: the OWNED rows of this slab, host <-> device, synchronous.
 *     `host` holds (row_end-row_begin) * dim_x elements of the field's element type.       */
SFL_API int sfl_upload(sfl_context *ctx, int field, const void *host, size_t bytes);
SFL_API int sfl_download(sfl_context *ctx, int field, void *host, size_t bytes);
/* Device pointer of the first OWNED row of the field's CURRENT buffer (zero-copy interop; the
 * context keeps ownership).  The pointer is writable, so the query counts as a write from outside (as
 * sfl_upload does): on slabs the next operator exchanges / measures again instead of trusting ghost rows
 * and back-trace reaches it knew before.  Velocity, colour and pressure are ping-ponged between two buffers by
 * the operators that rewrite them (advect: ino:255,286; the fused SOR launches), so the pointer
 * is valid only until the next operator that writes that field -- sfl_step writes all of them:
 * query again after every such call (the query costs nothing).  Asynchronous work may still be
 * pending: sfl_synchronize() before reading through the pointer from another stream.           */
SFL_API int sfl_field_device_ptr(sfl_context *ctx, int field, void **dev_ptr);

/* --- operators on the resident fields, asynchronous on the context's stream.
 *     On a slab each call performs the halo exchanges it needs.  All ranks of a group must
 *     issue the same calls in the same order (they contain matched send/recv pairs).        */
/* velocity <- advect(velocity, velocity, dt, no_slip)       ino:252-256 */
SFL_API int sfl_advect_velocity(sfl_context *ctx, float dt, int no_slip);
/* colour   <- advect(colour, velocity, dt, no_slip)         ino:281-287 */
SFL_API int sfl_advect_color(sfl_context *ctx, float dt, int no_slip);
/* divergence <- calculate_divergence(velocity, dx)          ino:274     */
SFL_API int sfl_calculate_divergence(sfl_context *ctx, float dx);
/* pressure <- poisson_solve(divergence, dx, iters, omega)   ino:275     */
SFL_API int sfl_poisson_solve(sfl_context *ctx, float dx, int iters, float omega);
/* velocity <- subtract_gradient(velocity, pressure, dx)     ino:276     */
SFL_API int sfl_subtract_gradient(sfl_context *ctx, float dx);
/* --- how far the pressure is from converged, and solves that go on from it ("how many iterations does this omega
 *     need?" on a context of any size).  WHOLE-DOMAIN contexts only: a slab gets SFL_ERR_STATE.  The definitions are
 *     the batches' (group 4: sfl_batch_residual, sfl_member_stop), word for word.                                    */
/* Update norm of the context's CURRENT pressure and divergence: *norm = max over all cells c of |p_gs(c) - p(c)|,
 * where p_gs(c) = k(c) * (dx * d(c) - sum(c)) is the value a plain Gauss-Seidel update would put into the cell: sum(c) =
 * the neighbours that exist, added in the order W, E, S (row j - 1), N (row j + 1), k = -1/2, -1/3, -1/4 for 2, 3, 4
 * neighbours; float32, every operation rounded on its own; both colours read from the same p, nothing is updated.  If
 * any |p_gs - p| is a NaN the result is a NaN.  The value does not depend on how the device reduces it: reproducible
 * bit for bit.  Cost: ONE streaming pass over p and d (8 bytes per cell) and one round trip to the host: on an MI355X
 * 0.13 ms at 8192 x 8192, the time of about six iterations of the solve there (profiles/context_until.txt).  ctx or
 * norm NULL return SFL_ERR_INVALID.  Synchronous.                                                                     */
SFL_API int sfl_residual(sfl_context *ctx, float dx, float *norm);
/* `iters` MORE red-black iterations starting from the pressure the context holds, not from zero.  After
 * sfl_poisson_solve(dx, a, omega), sfl_poisson_continue(dx, b, omega) leaves, bit for bit, poisson_solve(divergence, dx,
 * a + b, omega); after an sfl_upload of the pressure it iterates from that field.  iters == 0 does nothing; iters < 0
 * returns SFL_ERR_INVALID.  Asynchronous.                                                                            */
SFL_API int sfl_poisson_continue(sfl_context *ctx, float dx, int iters, float omega);
/* pressure <- the solve from zero stopped by the rule of sfl_member_stop.  `iters` is the cap K.  With u_k the update
 * norm (sfl_residual) of the pressure after k iterations, u_0 taken on p = 0, the solve stops at the smallest k in {0,
 * every, 2 * every, ...} with k < K for which u_k <= tol (IEEE float comparison) or u_k is a NaN, else at K.  The
 * pressure left is, bit for bit, poisson_solve(divergence, dx, k, omega).  *iterations = k, *norm = u_k of that pressure
 * (always evaluated, also at the cap); either out pointer may be NULL.  tol = +inf stops at k = 0: p = 0.  tol < 0 never
 * stops and makes no checks: the call is sfl_poisson_solve plus one final norm.  iters < 0, every < 1 or a NaN tol
 * return SFL_ERR_INVALID before any GPU work.  sfl_last_solve_info afterwards counts the solve's launches, not the checks'.
 *   Choosing `every`: a check costs one pass over p and d and one round trip to the host.  Measured on an MI355X
 * (profiles/context_until.txt): 0.13 ms at 8192 x 8192, where an iteration of the fused solve takes 0.023 ms -- a check
 * costs what about six iterations cost (the norm kernel alone: 0.58 of a 16-pass launch); at 2048 x 2048 0.03 ms,
 * nearly nine iterations.  Over a solve of 80 iterations the checks add 81 % at every = 8, 45 % at 16 and 24 % at 40.
 * A large `every` costs at most every - 1 iterations past the first k that would have passed, a small one costs a
 * check per `every` iterations: choose every >= 16 for production (32 .. 40 keeps the checks near a fifth of the
 * solve's time), small values for studies of the convergence itself.  Grids of at most 6144 cells run the whole rule inside
 * one launch, where a check is cheap (profiles/batch_until.txt).  Synchronous.                                        */
SFL_API int sfl_poisson_solve_until(sfl_context *ctx, float dx, int iters, float omega, float tol, int every,
                                    int32_t *iterations, float *norm);
/* --- what the FLOW looks like, without a download (20 bytes per cell): how fast it is, how divergence-free the velocity
 *     is, how much dye there is.  WHOLE-DOMAIN contexts only: a slab gets SFL_ERR_STATE.  The batches' calls (group 4:
 *     sfl_batch_flow_stats) report the same record per member, by the same definitions.                              */
#define SFL_STATS_VELOCITY 1   /* max_abs_vx, max_abs_vy, max_abs_div : one pass over v, 8 B per cell  */
#define SFL_STATS_DYE      2   /* dye_sum[3]                          : one pass over the dye, 12 B per cell */
struct sfl_flow_stats {
    float    max_abs_vx, max_abs_vy;   /* max over all cells of |v.x|, |v.y|                                   */
    float    max_abs_div;              /* max over all cells of |calculate_divergence(v, dx)(c)|               */
    uint32_t what;                     /* the SFL_STATS_* bits this record holds; the other members are 0      */
    uint64_t dye_sum[3];               /* sum over all cells of the raw UQ32 value of each channel, exact      */
};                                     /* 40 bytes: offsets 0, 4, 8, 12, 16.  Written `struct sfl_flow_stats`: the
                                          call below has the name, and C keeps only struct tags apart from functions */
/* Statistics of the context's CURRENT velocity and dye: the fields sfl_download would hand out at this moment -- after
 * sfl_step_n with its fused step boundaries, after the one-workgroup path, after an sfl_upload; a fresh context reports
 * zeros.  The call READS ONLY: no field changes (the context's divergence field included: nothing is written to it),
 * nothing counts as written from outside, no ghost row or back-trace reach the context knew is forgotten.
 *   max_abs_div: the divergence is calculate_divergence(v, dx) of the reference, operation for operation
 * (finitediff.cpp:9-39): inside, (-v.x(i-1, j) + v.x(i+1, j)) + (-v.y(i, j-1) + v.y(i, j+1)) (div_expr_fast, :29); on the
 * perimeter the terms added one by one to 0.0f in the order W, E, S, N with a missing neighbour's velocity taken as minus
 * the cell's own (div_expr_safe, :15-20); both times 1.0f / (2.0f * dx) (:36); float32, every operation rounded on its
 * own.  Taken on the velocity a step leaves -- projected by subtract_gradient -- it is the physical figure of merit of
 * iters, omega and tol; the update norm (sfl_residual) is only a proxy for it.
 *   The three maxima are taken as the update norm's is: the maximum over the bit patterns of |x| as unsigned integers.
 * Finite values and +inf order as floats do; any NaN wins, so a diverged field never reports a finite number (which NaN
 * is reported is not defined); |-0.0f| reports +0.0f.
 *   dye_sum: 64-bit integer sums of the raw uint32 values, the whole UQ32 range counting (values at and above 2^31
 * included), exact for every input: 2^28 cells per context x 2^32 per value stay below 2^60.  Semi-Lagrangian advection
 * does not conserve the dye; dye_sum against the step number shows how much it loses.
 *   None of the figures depends on how the device tiles or reduces: reproducible bit for bit, and bit for bit what numpy
 * gives on the downloaded fields.
 *   max_abs_vx is the back-trace figure: the next advection traces cell c back by v.x(c) * dt columns (advect.h:78-80),
 * float rounding is monotone and symmetric in sign, so max over c of |v.x(c) * dt| == |max_abs_vx * dt| bit for bit (and
 * likewise for y and rows): the longest back-trace of a step with any dt follows from one call -- what to choose dt by,
 * and the figure a slab's automatic advection halo (SFL_OPT_ADVECT_HALO: 64 rows, then a gather) depends on.
 *   what: a non-empty subset of the SFL_STATS_* bits, else SFL_ERR_INVALID; with SFL_STATS_DYE alone dx is ignored.  ctx
 * or out NULL return SFL_ERR_INVALID.  All of these are refused before any GPU work.  Synchronous: one launch per pass
 * asked for, one copy of the 40 bytes, one wait; nothing is allocated per call.
 *   Cost: one streaming pass per bit: not measured yet.                                                              */
SFL_API int sfl_flow_stats(sfl_context *ctx, int what, float dx, struct sfl_flow_stats *out);
/* --- how far two sets of fields are apart, without a download (20 bytes per cell and side): the distance of a's
 *     velocity, dye and pressure from b's, and whether they are the same bits.  WHOLE-DOMAIN contexts only: a slab
 *     gets SFL_ERR_STATE.  The batches' call (group 4: sfl_batch_distance) reports the same record per member.        */
#define SFL_DIST_VELOCITY 1   /* max_abs_dvx, max_abs_dvy, velocity_cells_differ  : one pass, 8 B per cell and side  */
#define SFL_DIST_DYE      2   /* max_abs_ddye, sum_abs_ddye, dye_cells_differ     : one pass, 12 B per cell and side */
#define SFL_DIST_PRESSURE 4   /* max_abs_dp, pressure_cells_differ                : one pass, 4 B per cell and side  */
struct sfl_field_distance {
    float    max_abs_dvx, max_abs_dvy;  /* max over cells of |a.v.x - b.v.x|, |a.v.y - b.v.y|            */
    float    max_abs_dp;                /* max over cells of |a.p - b.p|                                  */
    uint32_t what;                      /* the SFL_DIST_* bits this record holds; the other members are 0 */
    uint32_t velocity_cells_differ;     /* cells whose velocity differs in the BITS of either component   */
    uint32_t dye_cells_differ;          /* cells whose dye differs in any channel                         */
    uint32_t pressure_cells_differ;     /* cells whose pressure differs in its bits                       */
    uint32_t max_abs_ddye[3];           /* per channel: max over cells of |a - b| of the raw UQ32 values  */
    uint64_t sum_abs_ddye[3];           /* per channel: sum over cells of that, exact                     */
};                                      /* 64 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 40              */
/* The distance of a's CURRENT fields from b's: the fields sfl_download would hand out at this moment (settled as
 * sfl_flow_stats settles them; the pressure is the one sfl_download(SFL_FIELD_PRESSURE) copies).  The call READS ONLY,
 * on both sides, as sfl_flow_stats does.
 *   Floats (velocity, pressure): a - b is ONE float32 subtraction per cell and component; the maximum is taken over the
 * bit patterns of |a - b| as unsigned integers, as the maxima of sfl_flow_stats are.  Finite values and +inf order as
 * floats do; any NaN wins (which NaN is reported is not defined).  inf - inf is a NaN: two fields that hold the SAME inf
 * in a cell report a NaN distance and zero cells differing.  |+0 - -0| reports +0.0f while the cell counts as differing.
 *   *_cells_differ compare BITS: the same NaN payload on both sides is equal, +0 against -0 differs; a cell counts once
 * however many of its words differ.  All three counts zero <=> the fields asked for are identical bits: the library's
 * "bit for bit" (a member against a context, step_n against n steps, a twin run) as one device-side call.
 *   Dye: |a - b| is taken on the raw uint32 values, max(a, b) - min(a, b), no float involved, the whole UQ32 range
 * counting.  The sums are 64-bit and exact: 2^28 cells x 2^32 stay below 2^60.
 *   None of the figures depends on how the device tiles or reduces: bit for bit what numpy gives on the downloads.
 *   Refused with SFL_ERR_INVALID before any GPU work, in this order: `what` empty or with other bits; a, b or out NULL;
 * then a slab (SFL_ERR_STATE); then two contexts of different shape or on different devices.  a == b is allowed (all
 * zeros, or NaNs where a field holds an inf or a NaN).  Synchronous: the call waits for b's stream, makes one launch
 * per bit on a's stream, one copy of the 64 bytes and one wait; nothing is allocated per call (a's records are
 * allocated at its first call).
 *   Cost: two streaming reads per bit (profiles/ensemble.txt).                                                      */
SFL_API int sfl_distance(sfl_context *a, sfl_context *b, int what, struct sfl_field_distance *out);
/* next_p <- advect(p, velocity, dt, no_slip) for a field of the CALLER's, resident on the context's device
 * (advect.h:74-85; element = `channels` x `kind` as for sfl_host_advect_channels): further quantities carried by
 * the flow -- a temperature, a second dye -- without a round trip through the host.  Whole-domain contexts only;
 * next_p_dev must not alias p_dev; asynchronous on the context's stream (sfl_synchronize before reading).   */
SFL_API int sfl_advect_external(sfl_context *ctx, void *next_p_dev, const void *p_dev, int channels, int kind,
                                float dt, int no_slip);
/* One sim step in the order of ino:252-287: advect velocity (no-slip), [apply queued
 * forces], divergence, poisson_solve, subtract_gradient, advect colour (free-slip).         */
SFL_API int sfl_step(sfl_context *ctx, float dt, float dx, int iters, float omega);
/* n sim steps, exactly as n calls of sfl_step (the sim task's loop, ino:249-289, calls the step back to back); queued
 * forces go into the steps they were queued for (the timeline rule below: sfl_queue_forces queues for the FIRST step).
 * Knowing the next step lets the library fuse across the step boundary (SFL_OPT_STEP_SEAMS): a step with records runs
 * its advection, its forces and its divergence unfused, the others take the fused kernel.  n == 0 does nothing.     */
SFL_API int sfl_step_n(sfl_context *ctx, int n, float dt, float dx, int iters, float omega);
/* Queue point forces applied by the next sfl_step between the velocity advection and the
 * divergence (ino:264-269): velocity[index(cells[2k], cells[2k+1])] = (vel[2k], vel[2k+1])
 * in SIMULATION coordinates (the sketch's x/y swap is the caller's business), GLOBAL cell
 * indices.  On slabs EVERY rank queues the SAME list: a rank applies the cells that fall into
 * its rows and into the ghost row next to each cut, which sfl_step keeps exact instead of
 * exchanging it again (a list that differs between ranks gives a wrong divergence at the cuts).   */
SFL_API int sfl_queue_forces(sfl_context *ctx, const int *cells_ij, const float *vel_xy, int n);
/* The same in the sketch's own terms: `struct drag` as the touch task queues it (ino:45-48: Vector2<uint16_t>
 * coords, Vector2<float> velocity, GRAPHICS coordinates) with the transform loop() applies to it (ino:264-269):
 * cell = index(coords.y, coords.x), velocity = (velocity.y, velocity.x).  sizeof(sfl_drag) == sizeof(struct drag)
 * == 12, same member order: a drag_queue message can be passed as it is.  Coordinates outside the domain are
 * refused (SFL_ERR_INVALID, nothing queued); the sketch would write out of bounds.                        */
typedef struct sfl_drag {
    uint16_t coord_x, coord_y; /* msg.coords.x, msg.coords.y     */
    float vel_x, vel_y;        /* msg.velocity.x, msg.velocity.y */
} sfl_drag;
SFL_API int sfl_queue_drags(sfl_context *ctx, const sfl_drag *msgs, int n);
/* --- THE TIMELINE RULE: forces queued for step `step` of the steps to come, so that one sfl_step_n replays a whole
 *     recorded stroke (the sketch's loop() drains its drag_queue in every iteration, ino:264-269).  It holds for a
 *     context and, with "within each member", for a batch (group 4):
 *   - `step` counts the steps still to come.  0 is the next step any step call runs.  A record for step s is applied in
 *     that step between the velocity advection and the divergence.
 *   - Within one step, records are applied in the order of the calls that queued them (the last write wins).  For a
 *     batch that order holds within each member.
 *   - sfl_queue_forces, sfl_queue_drags and sfl_batch_queue_forces are the _at calls with step = 0, interleaved with
 *     them in call order.
 *   - A step call of n steps consumes the records of steps [0, n).  Later records move down by n.  This applies to
 *     sfl_step (n = 1), sfl_step_n, sfl_batch_step_n, sfl_batch_step_n_each and sfl_batch_step_n_until.  n == 0 consumes
 *     nothing.
 *   - Solves, uploads, setup and render calls neither consume nor shift.
 *   - A step call that is refused leaves the timeline exactly as it was.  Refusals are an argument check, or the
 *     recorder's SFL_ERR_STATE when the call would complete more frames than are free.
 *   - step < 0 and NULL pointers with n > 0 return SFL_ERR_INVALID and queue nothing.  So does a member outside the
 *     batch, and, for drags, a coordinate outside the domain.  The message names the first offender.  Cells outside the
 *     domain in sfl_[batch_]queue_forces_at are skipped at application.  All of it is checked before any GPU is touched.
 *   - On slabs every rank queues the same timeline (sfl_queue_forces above: the same list on every rank, per step).   */
SFL_API int sfl_queue_forces_at(sfl_context *ctx, int step, const int *cells_ij, const float *vel_xy, int n);
SFL_API int sfl_queue_drags_at(sfl_context *ctx, int step, const sfl_drag *msgs, int n);
/* What the timeline holds: *records = the records of all steps, *last_step = the last step that has one (-1 when the
 * timeline is empty).  Either out pointer may be NULL.  No GPU is touched.                                          */
SFL_API int sfl_forces_pending(sfl_context *ctx, int *records, int *last_step);
/* Empties the timeline (of every rank of an in-process group): no step consumes what was queued before.            */
SFL_API int sfl_forget_forces(sfl_context *ctx);

/* --- initial condition of the sketch (setup(), ino:196-241): velocity = 0; dye = three
 *     120-degree sectors around the centre chosen by atan2f, then the sketch's two in-place
 *     sequential 1-2-1 blur passes in UQ32.  The sketch pushes UINT32_MAX through float -> uint32
 *     conversions that are undefined in C++; they SATURATE here (as on the ESP32).  Whole-domain
 *     contexts only; asynchronous on the context's stream.                                   */
SFL_API int sfl_setup_sketch_fields(sfl_context *ctx);

/* --- dye visualiser (the arithmetic of the sketch's draw task, ino:116-176): every cell block
 *     is up-scaled `scaling` x `scaling` by the sketch's incremental lerps, narrowed to UQ32 and
 *     packed to RGB565 (byte-swapped like ino:173 when byteswap != 0).  `host_image` receives
 *     scaling*(dim_x-1) rows of scaling*(dim_y-1) uint16 pixels: the sim's i axis runs down the
 *     screen, j across (ino:164,180).  Whole-domain contexts only; synchronous.               */
SFL_API int sfl_render_rgb565(sfl_context *ctx, int scaling, int byteswap, uint16_t *host_image,
                              size_t bytes);

/* --- synchronisation / timing on the context's stream ---------------------------------- */
SFL_API int sfl_synchronize(sfl_context *ctx);
/* HIP-event stopwatch on the compute stream: start, run work, stop -> elapsed ms (blocks
 * until the stop event has completed).                                                     */
SFL_API int sfl_timer_start(sfl_context *ctx);
SFL_API int sfl_timer_stop(sfl_context *ctx, float *elapsed_ms);
/* Launch statistics of the last sfl_poisson_solve (sfl_poisson_continue, sfl_poisson_solve_until) on this context: kernel launches, halo
 * exchanges, half-sweeps fused per launch.  Any out pointer may be NULL.                    */
SFL_API int sfl_last_solve_info(sfl_context *ctx, int *launches, int *exchanges, int *fuse);

/* =====================================================================================
 * 4. batches: B independent whole-domain simulations of one dim_x * dim_y grid on one
 *    device (ensembles, parameter studies).  One launch steps every member, one workgroup
 *    per member with its fields in LDS.  After any sequence of batch calls member m holds,
 *    bit for bit, what a whole-domain context of the same shape holds after the same calls
 *    made with member m's data and member m's forces.
 *    Two kinds of batch, made by two constructors and alike in every other call:
 *    sfl_batch_create       members of at most 6144 cells, 16 B of LDS per cell (velocity,
 *                           divergence and pressure side by side): two members share a CU
 *                           at the sketch's 61 x 81;
 *    sfl_batch_create_large members of at most 20224 cells (128 x 128, 160 x 120), 8 B of
 *                           LDS per cell: the same bytes hold the advected velocity first
 *                           and the divergence and the pressure afterwards.  One member per
 *                           CU; speed not measured yet (profiles/batch_large.txt).
 * ===================================================================================== */

/* Limits: the shapes the one-workgroup path of a context takes (SFL_OPT_SMALL_GRID): dim_x, dim_y >= 2, at most
 * 6144 cells and at most 3072 cells of one colour (dim_y * ceil(dim_x / 2)); batch >= 1 and batch * dim_x * dim_y
 * <= 2^31 - 1.  Violations return SFL_ERR_INVALID before any GPU is touched; a failed allocation returns
 * SFL_ERR_NOMEM.  Every field is zero after create.                                               */
SFL_API int sfl_batch_create(sfl_batch **out, int device, int dim_x, int dim_y, int batch);
/* A batch of LARGE members: every sfl_batch_* call below takes it, with the same semantics, argument checks, staleness
 * rules and messages, and member m holds the same bits as a context of its shape.  Such a batch always runs the
 * large-member kernels, whatever its shape (a 2 x 2 or a 61 x 81 too: the layout can be priced against sfl_batch_create
 * at a shape both take).  Limits: dim_x, dim_y >= 2; at most SFL_BATCH_LARGE_MAX_CELLS cells; at most 10240 cells of one
 * colour (dim_y * ceil(dim_x / 2): ten per thread of a member's 1024); batch >= 1 and batch * dim_x * dim_y <= 2^31 - 1.
 * Violations return SFL_ERR_INVALID before any GPU is touched; a failed allocation returns SFL_ERR_NOMEM.  Every field
 * is zero after create.                                                                                               */
#define SFL_BATCH_LARGE_MAX_CELLS 20224   /* (163840 - 2048) / 8: p and d of one member in one CU's LDS, 2 KB kept for the kernels' static words */
SFL_API int sfl_batch_create_large(sfl_batch **out, int device, int dim_x, int dim_y, int batch);
/* *large = 1 for a batch made by sfl_batch_create_large, else 0.                                   */
SFL_API int sfl_batch_is_large(sfl_batch *b, int *large);
SFL_API int sfl_batch_destroy(sfl_batch *b);
/* Any out pointer may be NULL. */
SFL_API int sfl_batch_shape(sfl_batch *b, int *dim_x, int *dim_y, int *batch);
/* --- field I/O of members [first, first + count), synchronous.  Fields are the SFL_FIELD_* of a context with their
 *     element types, stored member-major: member m starts at element m * dim_x * dim_y and is laid out as a context's
 *     field.  bytes must be exactly count * dim_x * dim_y * element size.                          */
SFL_API int sfl_batch_upload(sfl_batch *b, int field, int first, int count, const void *host, size_t bytes);
SFL_API int sfl_batch_download(sfl_batch *b, int field, int first, int count, void *host, size_t bytes);
/* Device pointer of member 0 of the field's CURRENT buffer.  Velocity and colour ping-pong between two buffers as on a
 * context: the pointer is valid until the next step.                                             */
SFL_API int sfl_batch_field_device_ptr(sfl_batch *b, int field, void **dev_ptr);
/* Queue n point forces: record k sets velocity[member members[k], cell (cells_ij[2k], cells_ij[2k+1])] =
 * (vel_xy[2k], vel_xy[2k+1]) in the next step, between the velocity advection and the divergence (ino:264-269), in
 * queue order within each member (the last write wins).  Cells outside the domain are skipped; a member outside
 * [0, batch) fails the call with SFL_ERR_INVALID and queues nothing.                                */
SFL_API int sfl_batch_queue_forces(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n);
/* The same for step `step` of the steps to come, what the timeline holds, and forgetting it: the timeline rule of
 * group 3 (sfl_queue_forces_at), word for word; sfl_batch_queue_forces is step = 0.  The whole timeline is staged on the
 * device once per change, not once per step.  A call of sfl_batch_step_n or sfl_batch_step_n_each on a batch of
 * sfl_batch_create with n >= 2 and a record in some step of [1, n) runs its steps in ONE launch with every member's
 * velocity kept in LDS from step to step (between two frames, where a recorder is on); the results are the same bits.  */
SFL_API int sfl_batch_queue_forces_at(sfl_batch *b, int step, const int *members, const int *cells_ij,
                                      const float *vel_xy, int n);
SFL_API int sfl_batch_forces_pending(sfl_batch *b, int *records, int *last_step);
SFL_API int sfl_batch_forget_forces(sfl_batch *b);
/* n sim steps of every member, as sfl_step_n (queued forces go into the steps they were queued for, those of
 * sfl_batch_queue_forces into the first step: the timeline rule; n == 0 does nothing).  dt, dx,
 * iters and omega are the same for every member (sfl_batch_step_n_each: one set per member).  Asynchronous on the
 * batch's stream.                                                                                 */
SFL_API int sfl_batch_step_n(sfl_batch *b, int n, float dt, float dx, int iters, float omega);
/* pressure <- poisson_solve(divergence, dx, iters, omega) of every member.  Asynchronous.          */
SFL_API int sfl_batch_poisson_solve(sfl_batch *b, float dx, int iters, float omega);

/* --- per-member parameters and the update norm (parameter studies: one member per parameter point) ---------------- */
/* parameters of ONE member: what sfl_batch_step_n takes once for all of them */
typedef struct sfl_member_params {
    float dt, dx, omega;
    int32_t iters;
} sfl_member_params;                       /* 16 bytes */
/* n sim steps; member m runs every one of them with params[m] (an array of `batch` records, HOST memory, read before
 * the call returns).  Otherwise exactly sfl_batch_step_n: queued forces go into their steps (the timeline rule), n == 0 does nothing
 * (beyond checking its arguments), asynchronous.  Member m ends up, bit for bit, where a context of the same shape
 * ends up after sfl_step_n(ctx, n, params[m].dt, params[m].dx, params[m].iters, params[m].omega) with member m's data
 * and forces.  b or params NULL, n < 0 or any params[m].iters < 0 return SFL_ERR_INVALID (the message names the first
 * such member) before anything is launched or the force queue is touched; the floats are not checked, as
 * sfl_batch_step_n checks none.  Members with different iters finish at different times (the library starts those with
 * the most first, whatever their place in the batch); nothing else differs.                          */
SFL_API int sfl_batch_step_n_each(sfl_batch *b, int n, const sfl_member_params *params);
/* pressure <- poisson_solve(divergence, params[m].dx, params[m].iters, params[m].omega) of every member (dt is
 * ignored).  Asynchronous.                                                                          */
SFL_API int sfl_batch_poisson_solve_each(sfl_batch *b, const sfl_member_params *params);
/* The update norm of members [first, first + count) as the last *_each or *_until call left it: one float per member.
 * Synchronous.  bytes must be count * 4.
 *   The update norm of a member with pressure p, divergence d and its own dx is  max over all cells c of
 * |g(c) - p(c)|, where g(c) = k(c) * (dx * d(c) - sum(c)) is the value a plain Gauss-Seidel update would put into the
 * cell (poisson.cpp's p_gs): sum(c) = the neighbours that exist, added in the order W, E, S (row j - 1), N (row j + 1),
 * k = -1/2, -1/3, -1/4 for 2, 3, 4 neighbours; float32, every operation rounded on its own.  It is evaluated on the
 * FINAL pressure of the call (after sfl_batch_step_n_each(n): of the last step's solve, i.e. of the divergence and
 * pressure sfl_batch_download hands out afterwards), both colours, no cell updated in between -- the distance of p
 * from the fixed point of its iteration, in units of p.  If any |g - p| is a NaN the report is a NaN: a diverged member
 * never reports a finite number.  The value does not depend on how the device reduces it: reproducible bit for bit.
 *   Every *_each and *_until call (n > 0) writes the report of every member.  sfl_batch_step_n (n > 0), sfl_batch_poisson_solve and
 * an sfl_batch_upload of the divergence or the pressure make it stale, and a fresh batch has none: SFL_ERR_STATE.  */
SFL_API int sfl_batch_residual(sfl_batch *b, int first, int count, float *host, size_t bytes);
/* --- the same, each member's pressure solve stopped at a tolerance ("how many iterations does this omega need?") --- */
/* when ONE member's solve stops: the second record of a member in the *_until calls */
typedef struct sfl_member_stop {
    float tol;                             /* stop at the first check with update norm <= tol; < 0: never */
    int32_t every;                         /* a check in front of every `every`-th iteration, >= 1 */
} sfl_member_stop;                         /* 8 bytes */
/* The rule.  Member m has params[m] = {dt, dx, omega, iters} and stops[m] = {tol, every}; iters is now the CAP K.  Let
 * u_k be the update norm of the member's pressure after k iterations of its solve -- sfl_batch_residual's definition
 * below, word for word: both colours, nothing updated in between -- with u_0 taken on p = 0.  The solve stops at the
 * smallest k in {0, every, 2 * every, ...} with k < K for which u_k <= tol (IEEE float comparison) or u_k is a NaN (a
 * diverged member ends at the first check that sees the NaN); otherwise at k = K.  The pressure left is that of exactly
 * k iterations: bit for bit poisson_solve(divergence, dx, k, omega) of the reference, which has no such test of its
 * own.  The update norm reported (sfl_batch_residual) is u_k of that final pressure, the iteration count reported
 * (sfl_batch_iterations) is k.
 *   A negative tol never stops a member, not even at a NaN: the call is then the *_each call, bit for bit, report
 * included, and every count is the cap.  tol = +inf stops at k = 0: p = 0.  every < 1, a NaN tol or iters < 0 return
 * SFL_ERR_INVALID (the message names the first such member) before anything is launched or the force queue is
 * touched, as b, params or stops NULL and n < 0 do.  Members are started by cap, the largest first.          */
/* sfl_batch_step_n_each with the solve of every step run by the rule (queued forces go into their steps, the timeline rule; n == 0
 * launches nothing and leaves the reports as they were).  Asynchronous; params and stops are arrays of `batch` records
 * in HOST memory, read before the call returns.                                                       */
SFL_API int sfl_batch_step_n_until(sfl_batch *b, int n, const sfl_member_params *params, const sfl_member_stop *stops);
/* pressure of every member <- its solve by the rule on its divergence (dt is ignored).  Asynchronous.  */
SFL_API int sfl_batch_poisson_solve_until(sfl_batch *b, const sfl_member_params *params, const sfl_member_stop *stops);
/* The iterations of members [first, first + count) as the last *_until call left them, two ints per member: those of
 * the member's last solve (the one sfl_batch_residual reports on), then their sum over the n steps of that call (after
 * sfl_batch_poisson_solve_until: the same number twice).  Synchronous.  bytes must be count * 8.  Valid only after an
 * *_until call (n > 0): whatever makes sfl_batch_residual stale makes this stale, and so does an *_each call --
 * SFL_ERR_STATE, and the message says to call sfl_batch_step_n_until or sfl_batch_poisson_solve_until.    */
SFL_API int sfl_batch_iterations(sfl_batch *b, int first, int count, int32_t *host, size_t bytes);
/* --- the flow statistics of members [first, first + count): one sfl_flow_stats record per member (group 2,
 *     sfl_flow_stats: the definitions, word for word), of the member's CURRENT velocity and dye -- what sfl_batch_download
 *     would hand out -- with the divergence scaled by dx.  A member reports, bit for bit, what a context holding the
 *     same fields reports.  Every member's record is evaluated by ONE launch per pass asked for, whatever the range;
 *     [first, first + count) is copied out.  Reads only: the reports of sfl_batch_residual and sfl_batch_iterations do
 *     not go stale.  Synchronous; the device and pinned records are allocated once per batch, nothing per call.
 *     `what` empty or with other bits, b or host NULL, bytes != count * 40 and a range that is not inside the batch
 *     return SFL_ERR_INVALID before any GPU work.                                                                  */
SFL_API int sfl_batch_flow_stats(sfl_batch *b, int what, float dx, int first, int count,
                                 struct sfl_flow_stats *host, size_t bytes);
/* The same with member m's divergence scaled by params[m].dx: params is an array of `batch` records (HOST memory, read
 * before the call returns; NULL returns SFL_ERR_INVALID), whose other members are ignored.                            */
SFL_API int sfl_batch_flow_stats_each(sfl_batch *b, int what, const sfl_member_params *params,
                                      int first, int count, struct sfl_flow_stats *host, size_t bytes);
/* --- the distance of members [first, first + count) of b from a reference: one sfl_field_distance record per member
 *     (group 2, sfl_distance: the definitions, word for word), of the members' CURRENT velocity, dye and pressure --
 *     what sfl_batch_download would hand out.  Record k is member first + k of b against member ref_member of `ref`;
 *     with ref_member == -1 it is against member first + k of `ref`: the pairwise form, for twins.  ref == NULL means
 *     b itself.  `ref` may be the other kind of batch (sfl_batch_create_large against sfl_batch_create); it must have
 *     b's dim_x and dim_y and sit on b's device.  A member's record is, bit for bit, what sfl_distance reports for two
 *     contexts holding those fields.  ONE launch per bit whatever the range; the call waits for ref's stream first.
 *     Reads only, on both sides: the reports of sfl_batch_residual and sfl_batch_iterations do not go stale, the
 *     timeline of queued forces and the recorder are untouched.  Synchronous; the device and pinned records are
 *     allocated once per batch, nothing per call.  count == 0 does nothing.
 *       Refused with SFL_ERR_INVALID before any GPU work, in this order: `what` empty or with other bits; count < 0 or
 *     bytes != count * 64 (the message names the bytes expected); b or host NULL; a range that is not inside b,
 *     ref_member outside [-1, ref's batch), a pairwise range that is not inside ref; a ref of another shape or on
 *     another device.                                                                                               */
SFL_API int sfl_batch_distance(sfl_batch *b, int what, sfl_batch *ref, int ref_member, int first, int count,
                               struct sfl_field_distance *host, size_t bytes);
/* --- the per-cell envelope of the dye over members: the mean picture of an ensemble and the picture of where its
 *     members disagree, without downloading B fields ---------------------------------------------------------------- */
#define SFL_ENV_MEAN   0   /* floor(sum over the members / count), 64-bit integer arithmetic */
#define SFL_ENV_MIN    1
#define SFL_ENV_MAX    2
#define SFL_ENV_SPREAD 3   /* max - min */
/* Take the four fields, per cell and channel, over the CURRENT dye of members [first, first + count), count >= 1 --
 * the dye sfl_batch_download would hand out if the stream were drained here.  All four are exact integers on the raw
 * UQ32 values (the sum of up to 2^31 members x 2^32 stays below 2^63): no float, no tolerance, nothing depends on the
 * order of reduction; bit for bit numpy's min, max and sum(uint64) // count over the members.  They are a SNAPSHOT kept
 * on the device with the batch, four dye-typed fields of dim_x * dim_y * 3 words: later steps do not change them, the
 * next call replaces them.  The members' fields are only read.  Asynchronous on the batch's stream: the call can sit
 * between two step calls without a host wait.  The buffers are allocated at the first call and freed by
 * sfl_batch_destroy.  b NULL, count < 1 and a range that is not inside the batch return SFL_ERR_INVALID before any GPU
 * work and leave an earlier snapshot as it was.                                                                      */
SFL_API int sfl_batch_envelope(sfl_batch *b, int first, int count);
/* The range the snapshot holds; count 0: none has been taken yet.  Either out pointer may be NULL.  Never waits.      */
SFL_API int sfl_batch_envelope_info(sfl_batch *b, int *first, int *count);
/* Copy field `which` (SFL_ENV_*) of the snapshot out, laid out as one context's dye: dim_x * dim_y * 3 uint32.
 * Synchronous.  Refused in this order: `which` outside 0..3, bytes != dim_x * dim_y * 12, b or host NULL
 * (SFL_ERR_INVALID), then no snapshot yet (SFL_ERR_STATE).                                                           */
SFL_API int sfl_batch_envelope_download(sfl_batch *b, int which, uint32_t *host, size_t bytes);
/* Draw field `which` of the snapshot: the image is, bit for bit, what sfl_render_rgb565 writes for a context whose dye
 * is that field (H = scaling * (dim_x - 1) rows of W = scaling * (dim_y - 1) uint16).  Synchronous.  Refused in this
 * order: `which` outside 0..3, scaling outside 1..64, bytes != H * W * 2, b or host_image NULL (SFL_ERR_INVALID), then
 * no snapshot yet (SFL_ERR_STATE).                                                                                   */
SFL_API int sfl_batch_envelope_render(sfl_batch *b, int which, int scaling, int byteswap, uint16_t *host_image,
                                      size_t bytes);
/* sfl_setup_sketch_fields for every member (the saturating definition included).  Asynchronous.    */
SFL_API int sfl_batch_setup_sketch_fields(sfl_batch *b);
/* sfl_render_rgb565 of one member's dye.  Synchronous.                                            */
SFL_API int sfl_batch_render_rgb565(sfl_batch *b, int member, int scaling, int byteswap, uint16_t *host_image,
                                    size_t bytes);
/* --- the frames of many members: the draw task of a whole batch in ONE launch (one workgroup per tile of cell blocks of
 *     one member, the tile's corner texels staged in LDS), and a recorder that renders while the batch steps ----------- */
/* The images of members [first, first + count) of the CURRENT dye, member-major: image k (H = scaling * (dim_x - 1) rows
 * of W = scaling * (dim_y - 1) uint16, i down the screen and j across, as sfl_render_rgb565) starts at pixel k * H * W
 * and is, bit for bit, what sfl_batch_render_rgb565(b, first + k, scaling, byteswap, ...) writes.  One launch and one
 * device-to-host copy whatever count is; the device buffer stays with the batch and grows when needed.  Synchronous.
 * count == 0 does nothing.  b NULL, host_images NULL (count > 0), scaling outside 1..64, a range that is not inside the
 * batch and bytes != count * H * W * 2 return SFL_ERR_INVALID before any GPU work.                                      */
SFL_API int sfl_batch_render_members(sfl_batch *b, int first, int count, int scaling, int byteswap,
                                     uint16_t *host_images, size_t bytes);
/* Start recording: `capacity` frames of members [first, first + count) at this scaling and byte order are allocated on
 * the device and the recorder's step count is set to 0.  From now on every step of sfl_batch_step_n, sfl_batch_step_n_each
 * and sfl_batch_step_n_until counts, across calls, and after the step that makes the count a multiple of `every`, frame
 * count / every - 1 is rendered from the dye that step left -- the dye sfl_batch_download would hand out if the call ended
 * there.  The render is one launch on the batch's stream between the step launches: the step calls stay asynchronous and
 * the host never waits.  Nothing else about the step calls changes: every field keeps its bits, sfl_batch_residual and
 * sfl_batch_iterations keep their validity, queued forces still go into their steps.  sfl_batch_poisson_solve*,
 * uploads and sfl_batch_setup_sketch_fields neither count nor record.
 *   A step call whose n steps would complete more frames than are free is refused as a whole with SFL_ERR_STATE (the
 * message names sfl_batch_record_read and sfl_batch_record_start), after the call's own argument checks and before
 * anything is launched: fields, force queue, reports and step count stay untouched.  The recorder fills up at a frame
 * boundary, so a caller who reads the frames and calls sfl_batch_record_start again whenever it is full keeps the phase.
 *   Called while recording, it starts afresh: the frames are dropped, the count is 0 again, and the device buffer is
 * reallocated only if it must grow.  b NULL, every < 1, capacity < 1 (or so large that the frames' bytes do not fit a
 * size_t), scaling outside 1..64, count < 1 and a range that
 * is not inside the batch return SFL_ERR_INVALID before any GPU work and leave a running recording as it was; a failed
 * allocation returns SFL_ERR_NOMEM and leaves the batch not recording.  One frame may exceed 4 GiB.                    */
SFL_API int sfl_batch_record_start(sfl_batch *b, int every, int first, int count, int scaling, int byteswap, int capacity);
/* Stop recording and free the frames (sfl_batch_destroy frees them too).  Stopping a batch that is not recording is
 * SFL_OK.  Afterwards steps record nothing and sfl_batch_record_read returns SFL_ERR_STATE.                             */
SFL_API int sfl_batch_record_stop(sfl_batch *b);
/* Frames written so far, the capacity, and the steps counted since sfl_batch_record_start.  Any out pointer may be NULL.
 * For a batch that is not recording all three are 0 and the call returns SFL_OK.  Never waits.                          */
SFL_API int sfl_batch_record_info(sfl_batch *b, int *frames, int *capacity, int64_t *steps);
/* Copy members [first, first + count) of frame `frame` out, member-major as sfl_batch_render_members lays them out.  The
 * numbers are the batch's member numbers and must lie inside the recorded range.  Frames are not consumed.  Synchronous.
 * Not recording: SFL_ERR_STATE.  b NULL, host NULL (count > 0), frame outside [0, frames written), a range that is not
 * inside the recorded one and bytes != count * H * W * 2 return SFL_ERR_INVALID before any GPU work.                    */
SFL_API int sfl_batch_record_read(sfl_batch *b, int frame, int first, int count, uint16_t *host, size_t bytes);
/* --- TRACERS: points that move with the flow, and probes of the fields at positions that are no cell centres, without
 *     a download.  A context (group 2; WHOLE-DOMAIN contexts only: a slab gets SFL_ERR_STATE) holds one set of n tracers;
 *     a batch (sfl_batch_tracers_*) holds K tracers per member, laid out [member][k][2].
 *   A position (x, y) is two floats in GRID coordinates: x along i (the fast axis) and y along j, exactly the coordinates
 * sample(p, i, j, dim_x, dim_y, no_slip) of sfl/advect.h takes; cell (i, j) has its centre at (i, j).
 *   ADVANCE by dt: u = sample<Vector2<float>>(velocity, x, y, dim_x, dim_y, true) on the velocity the context or member
 * holds at that moment, then x' = x + u.x * dt, y' = y + u.y * dt: per component one rounded product and one rounded sum,
 * no FMA.  no_slip is true, as the reference samples the velocity (ino:253): a tracer more than half a cell outside a
 * wall samples zero and stops.
 *   SAMPLE: at every tracer sample<T> of ONE field, bit for bit the header's: SFL_FIELD_VELOCITY as Vector2<float> (8
 * bytes per tracer), SFL_FIELD_PRESSURE and SFL_FIELD_DIVERGENCE as float (4), SFL_FIELD_COLOR as Vector3<UQ32> (12, the
 * raw values; narrowed to UQ32 exactly where the reference narrows).  The caller chooses no_slip.
 *   NaN: a tracer with a NaN coordinate is never sampled: an advance leaves BOTH its coordinates as they are, a sample
 * writes NaN for the float fields and 0 for the dye.  +-inf and huge finite coordinates are ordinary positions outside
 * the domain and take sample's wall branches.  A NaN velocity makes a position NaN; it then stays.
 *   FOLLOWING: a set made with follow != 0 is advanced after every step of every step call (sfl_step, sfl_step_n; a
 * batch: sfl_batch_step_n, _each, _until), with that step's dt (a batch's _each and _until calls: each member's own) and
 * that step's projected velocity -- the tracers move as the dye does.  sfl_step_n(n) with a following set == n x
 * (sfl_step; sfl_tracers_advance(dt)), bit for bit in the positions and in every field.  The advance is one launch on
 * the context's or batch's stream behind the step's: the step calls stay as asynchronous as they are.  A step call reads
 * each step's projected velocity from memory, so with a following set sfl_step_n runs WITHOUT the fused step boundaries
 * of SFL_OPT_STEP_SEAMS (which never store it), and a batch's call with records in its later steps runs one launch per
 * step instead of one for all: the fields keep their bits, the call costs what n single steps cost.  Without a
 * following set every call launches exactly what it launched before there were tracers.
 *   TRAILS: after sfl_tracers_trail_start, every advance (followed or sfl_tracers_advance) counts, and after every
 * `every`-th the positions are also written to the next of `capacity` slots in device memory (by the advance's own
 * launch), read out afterwards.  A call whose advances would complete more slots than are free is refused WHOLE with
 * SFL_ERR_STATE, after its argument checks and before anything is staged or launched: fields, positions, timeline and
 * counts stay untouched.
 *   Every refusal below is made before any GPU work and carries its own message (sfl_last_error).  capacity of a
 * position buffer counts FLOATS.                                                                                        */
/* Attach n tracers at xy[2 k], xy[2 k + 1] (copied; synchronous), replacing the set the context holds and ending its
 * trail.  n == 0 removes the set (xy may be NULL).  ctx NULL, xy NULL with n > 0: SFL_ERR_INVALID; a slab: SFL_ERR_STATE. */
SFL_API int sfl_tracers_set(sfl_context *ctx, const float *xy, size_t n, int follow);
/* *n = the tracers attached (0: none).  NULL arguments: SFL_ERR_INVALID.                                                */
SFL_API int sfl_tracers_count(sfl_context *ctx, size_t *n);
/* The positions now (synchronous).  capacity < 2 n floats, NULL arguments: SFL_ERR_INVALID; no set: SFL_ERR_STATE.       */
SFL_API int sfl_tracers_download(sfl_context *ctx, float *xy, size_t capacity);
/* One advance by dt on the current velocity (asynchronous).  No set: SFL_ERR_STATE; a full trail: SFL_ERR_STATE.         */
SFL_API int sfl_tracers_advance(sfl_context *ctx, float dt);
/* sample<T> of `field` (SFL_FIELD_*) at every tracer, n elements in tracer order (synchronous; reads only).  An unknown
 * field, capacity_bytes < n elements, NULL arguments: SFL_ERR_INVALID; no set: SFL_ERR_STATE.                           */
SFL_API int sfl_tracers_sample(sfl_context *ctx, int field, int no_slip, void *out, size_t capacity_bytes);
/* Start a trail of `capacity` slots, one after every `every`-th advance; the count of advances starts at 0.  Called with
 * a trail running, it starts afresh.  every < 1, capacity < 1 (or slots whose bytes do not fit a size_t), ctx NULL:
 * SFL_ERR_INVALID; no set attached: SFL_ERR_STATE.                                                                      */
SFL_API int sfl_tracers_trail_start(sfl_context *ctx, int every, int capacity);
/* Stop the trail and free its slots (sfl_tracers_set and sfl_destroy do too).  Without a trail: SFL_OK.                  */
SFL_API int sfl_tracers_trail_stop(sfl_context *ctx);
/* Slots written so far, the capacity, the advances counted since the start; all 0 without a trail.  Out pointers may be
 * NULL.  Never waits.                                                                                                   */
SFL_API int sfl_tracers_trail_info(sfl_context *ctx, int *written, int *capacity, int64_t *advances);
/* Slots [first_slot, first_slot + slots) into xy, slot-major, each slot n positions (synchronous; not consumed).  A
 * range that is not inside the slots written, capacity < slots * 2 n floats, NULL arguments: SFL_ERR_INVALID; no trail:
 * SFL_ERR_STATE.                                                                                                        */
SFL_API int sfl_tracers_trail_read(sfl_context *ctx, int first_slot, int slots, float *xy, size_t capacity);
/* The same for a batch of either kind: k tracers per member, xy and every slot laid out [member][k][2], samples
 * [member][k][element]; capacities count the floats (bytes) of ALL members.  sfl_batch_tracers_advance moves every
 * member by the one dt.  *k of sfl_batch_tracers_count is the number per member.                                         */
SFL_API int sfl_batch_tracers_set(sfl_batch *b, const float *xy, size_t k, int follow);
SFL_API int sfl_batch_tracers_count(sfl_batch *b, size_t *k);
SFL_API int sfl_batch_tracers_download(sfl_batch *b, float *xy, size_t capacity);
SFL_API int sfl_batch_tracers_advance(sfl_batch *b, float dt);
SFL_API int sfl_batch_tracers_sample(sfl_batch *b, int field, int no_slip, void *out, size_t capacity_bytes);
SFL_API int sfl_batch_tracers_trail_start(sfl_batch *b, int every, int capacity);
SFL_API int sfl_batch_tracers_trail_stop(sfl_batch *b);
SFL_API int sfl_batch_tracers_trail_info(sfl_batch *b, int *written, int *capacity, int64_t *advances);
SFL_API int sfl_batch_tracers_trail_read(sfl_batch *b, int first_slot, int slots, float *xy, size_t capacity);
/* --- VIEWS: the flow itself as pictures -- speed, vorticity, pressure and divergence, without a download.  A view is a
 *     scalar field derived from the velocity or the pressure, mapped through a palette to one Vector3<UQ32> texel per
 *     grid node and drawn by the draw task's own chain.  A view image is, BY DEFINITION, sfl_batch_render_rgb565 of a
 *     member whose dye is the view's node colours, bit for bit.  Whole-domain contexts (a slab: SFL_ERR_STATE) and
 *     batches of either kind.  Every call reads only, runs on the object's stream behind whatever was launched before,
 *     and is synchronous only where it copies to the host.
 *   THE FOUR SCALARS are float32, every product, sum and quotient rounded on its own, node (i, j) at dim_x * j + i; all
 * four use k = 1.0f / (2.0f * dx), formed as calculate_divergence forms it:
 *     SFL_VIEW_SPEED       sqrtf(vx * vx + vy * vy), correctly rounded, denormals kept; dx plays no part.
 *     SFL_VIEW_VORTICITY   ((E - W) - (N - S)) * k in this order for EVERY node (there is no separate edge order), E, W =
 *                          vy at (i + 1, j) and (i - 1, j), N, S = vx at (i, j + 1) and (i, j - 1); a neighbour outside
 *                          the domain is MINUS THE NODE'S OWN component, the ghost rule of calculate_divergence's edge
 *                          expression ("ghost velocity is negative").  This is a definition stated here, not a result of
 *                          the reference, which has no vorticity.
 *     SFL_VIEW_PRESSURE    the pressure the object holds: what sfl_download(SFL_FIELD_PRESSURE) copies.
 *     SFL_VIEW_DIVERGENCE  calculate_divergence(v, dx) bit for bit, edge nodes included, computed from the velocity the
 *                          object holds now; nothing is stored (SFL_FIELD_DIVERGENCE keeps what the last step left).
 *   SCALAR -> TEXEL: with r = 1.0f / (hi - lo) and t = (s - lo) * r: if s or t is NaN the texel is nan_colour.  Otherwise
 * t is clamped to [0, 1] (+-inf included), x = t * (float)(stops - 1), n = min((int)x, stops - 2), f = x - (float)n and
 * each channel = uq_narrow(a + (b - a) * f) with a, b = uq_widen of stops n and n + 1.  The texel is this narrowed
 * uint32; the draw widens it again, exactly as it widens dye.
 *   No stop and no nan_colour channel may exceed SFL_VIEW_MAX_COLOUR = 0xFC000000.  That value still gives RGB565 its
 * full 5 / 6 / 5 bits, and it keeps every intermediate of the palette's lerp and of the draw's walks inside [0, 2^32),
 * where narrowing is defined: the nearest excluded value, 0xFF000000, is 5 * 10^7 away, and a chain of 63 additions errs
 * by about 10^4.  Saturation of UQ32 is not defined by this interface.
 *   Refused with SFL_ERR_INVALID before any GPU work, each with its own message: `what` outside 0..3, stops outside
 * 2..256, colours NULL, hi - lo (in float) not finite or not > 0, dx not finite or not > 0, a stop or nan_colour channel
 * above SFL_VIEW_MAX_COLOUR; NULL objects and buffers, a byte count that is not the result's, a member range that is not
 * inside the batch.  A context is settled as sfl_flow_stats settles it.                                                 */
#define SFL_VIEW_SPEED 0
#define SFL_VIEW_VORTICITY 1
#define SFL_VIEW_PRESSURE 2
#define SFL_VIEW_DIVERGENCE 3
#define SFL_VIEW_MAX_STOPS 256
#define SFL_VIEW_MAX_COLOUR 0xFC000000u
/* 40 bytes on every supported target: what 0, dx 4, lo 8, hi 12, stops 16, nan_colour 20, colours 32.                  */
struct sfl_view {
    int32_t what;            /* SFL_VIEW_*                                                          */
    float dx;                /* grid spacing of vorticity and divergence (ignored by the other two, but checked)         */
    float lo, hi;            /* the scalars mapped to the first and the last stop                    */
    int32_t stops;           /* 2 .. SFL_VIEW_MAX_STOPS                                             */
    uint32_t nan_colour[3];  /* the texel of a NaN, raw UQ32                                        */
    const uint32_t *colours; /* stops x 3 raw UQ32 values; read during the call only                */
};
/* The scalar field(s): dim_x * dim_y floats (a batch: of members [first, first + count), member-major); bytes must be
 * exactly that.  dx as in struct sfl_view.  count == 0 does nothing.  Synchronous.                                      */
SFL_API int sfl_view_scalar(sfl_context *ctx, int what, float dx, float *host, size_t bytes);
SFL_API int sfl_batch_view_scalar(sfl_batch *b, int what, float dx, int first, int count, float *host, size_t bytes);
/* The node colours, 3 words per node, laid out as SFL_FIELD_COLOR: for a caller's own renderer.  Synchronous.            */
SFL_API int sfl_view_texels(sfl_context *ctx, const struct sfl_view *view, uint32_t *host, size_t bytes);
SFL_API int sfl_batch_view_texels(sfl_batch *b, const struct sfl_view *view, int first, int count, uint32_t *host,
                                  size_t bytes);
/* The images.  Image shape, the scaling's range 1..64, the byte-count check and count == 0 are those of
 * sfl_render_rgb565 / sfl_batch_render_members.  One launch whatever count is: the node colours are formed in LDS in
 * front of the draw and never stored.  A context's image of more than 2^31 - 1 pixels is refused (SFL_ERR_INVALID): the
 * kernel's offsets inside one image are 32-bit.  Synchronous.                                                           */
SFL_API int sfl_view_render(sfl_context *ctx, const struct sfl_view *view, int scaling, int byteswap,
                            uint16_t *host_image, size_t bytes);
SFL_API int sfl_batch_view_render_members(sfl_batch *b, const struct sfl_view *view, int first, int count, int scaling,
                                          int byteswap, uint16_t *host_images, size_t bytes);
/* What the recorder draws from the next frame on: this view, or the dye (view NULL).  SFL_ERR_STATE unless a recording is
 * on; sfl_batch_record_start and sfl_batch_record_stop reset it to the dye, and a recording that never calls it behaves
 * exactly as before.  The view is copied, palette included, to a device buffer the batch owns and frees: the caller's
 * memory is not read after the call returns.  Asynchronous: the copy runs on the batch's stream behind the frames
 * already launched.  Frames keep their size: sfl_batch_record_info and sfl_batch_record_read do not change.  A view frame
 * shows the velocity and the pressure the step that completed it left.                                                  */
SFL_API int sfl_batch_record_view(sfl_batch *b, const struct sfl_view *view);
/* --- HISTORIES: the flow statistics of every k-th step, recorded while stepping.  A history is `capacity` samples in
 *     device memory; after every `every`-th step of any step call, ONE launch on the context's or batch's stream writes
 *     one 64-byte record per recorded member from the fields that step left.  The step calls stay asynchronous and the
 *     host never waits; the records are read out afterwards.  Batches of either kind, and whole-domain contexts (group 2;
 *     a slab gets SFL_ERR_STATE).
 *   THE RECORD.  Every figure is one the calls above already define, word for word:
 *     max_abs_vx, max_abs_vy, max_abs_div, what, dye_sum   struct sfl_flow_stats (sfl_flow_stats: the definitions) of
 *                   the velocity and the dye the step left, with what = SFL_STATS_VELOCITY | SFL_STATS_DYE and the
 *                   divergence scaled by the step's dx: the first 40 bytes ARE a struct sfl_flow_stats;
 *     update_norm   sfl_batch_residual's (sfl_residual's) definition on the pressure and the divergence the step left,
 *                   with the step's dx.  A uniform sfl_batch_step_n leaves no valid sfl_batch_residual report; the
 *                   history evaluates the norm all the same, from the pressure and divergence in memory;
 *     iterations    of that step's solve: iters, or under sfl_batch_step_n_until the k the rule (sfl_member_stop)
 *                   stopped the member at -- the first word of sfl_batch_iterations if the call ended with that step;
 *     step          the history's step count when the sample was taken: every, 2 * every, ...;
 *     dt, dx        that step's: the call's, or the member's own in the *_each and *_until calls.
 *   A record equals, bit for bit, what sfl_batch_flow_stats[_each], sfl_batch_residual and sfl_batch_iterations (a
 * context: sfl_flow_stats, sfl_residual) return when called right after the same step.  Maxima over bit patterns and
 * integer sums do not depend on the order of reduction: no tolerance anywhere.
 *   COUNTING.  Every step of sfl_batch_step_n, sfl_batch_step_n_each and sfl_batch_step_n_until counts, across calls
 * (a context: every step of sfl_step and sfl_step_n).  Solves, uploads and setup_sketch_fields neither count nor sample.
 * A step call whose steps would complete more samples than are free is refused WHOLE with SFL_ERR_STATE, after the
 * call's own argument checks and before anything is staged or launched: fields, timeline, reports, frames and every
 * count stay untouched.  The history fills up at a sample boundary, so a caller who reads the samples and starts the
 * history again whenever it is full keeps the phase.
 *   WHAT A HISTORY CHANGES.  Nothing about any result: all fields keep their bits, sfl_batch_residual and
 * sfl_batch_iterations keep their validity, queued forces go into their steps, a recorder and following tracers run as
 * they do.  It changes which launches a call makes: a batch call that would run several steps in one launch (a timeline
 * with records in its later steps, small members) is cut into launches that end at the steps whose sample is due -- with
 * a recorder on as well, at either's due steps -- and sfl_step_n on a context runs WITHOUT the fused step boundaries of
 * SFL_OPT_STEP_SEAMS, as with a following set of tracers: a seam never stores the velocity a sample reads.  Without a
 * history on, every call launches exactly what it launched before there were histories.
 *   Cost: one launch per sample reading 28 bytes per cell and member (a batch; a context: the two passes of
 * sfl_flow_stats and the pass of sfl_residual).  Measured on an MI355X (profiles/history.txt), a sample after EVERY
 * step: 61 x 81 x 1024 members at 20 iterations, +30 us per sample beside a step of 125 us; 128 x 128 x 256 large members,
 * +28 us beside a step of 168 us.  The loop of synchronous calls a history replaces -- step_n_until(1), flow_stats,
 * residual, iterations -- took 292 us per step where the one call with a history takes 201.  Choose `every` accordingly.
 *   Every refusal below is made before any GPU work, carries its own message (sfl_last_error) and leaves a running
 * history as it was.                                                                                                    */
struct sfl_history_record {
    float    max_abs_vx, max_abs_vy, max_abs_div;
    uint32_t what;
    uint64_t dye_sum[3];
    float    update_norm;
    int32_t  iterations;
    int64_t  step;
    float    dt, dx;
};                                     /* 64 bytes: offsets 0, 4, 8, 12, 16, 40, 44, 48, 56, 60 */
/* Start a history of members [first, first + count): `capacity` samples of count records are allocated on the device
 * and the history's step count is set to 0.  Called while a history is on, it starts afresh: the samples are dropped,
 * the count is 0 again, and the device buffer is reallocated only if it must grow.  b NULL, every < 1, capacity < 1 (or
 * so large that the samples' bytes do not fit a size_t), count < 1 and a range that is not inside the batch return
 * SFL_ERR_INVALID; a failed allocation returns SFL_ERR_NOMEM and leaves the batch without a history.                    */
SFL_API int sfl_batch_history_start(sfl_batch *b, int every, int first, int count, int capacity);
/* Stop the history and free the samples (sfl_batch_destroy frees them too).  Without a history: SFL_OK.                  */
SFL_API int sfl_batch_history_stop(sfl_batch *b);
/* Samples written so far, the capacity, and the steps counted since the start; all 0 without a history.  Any out
 * pointer may be NULL.  Never waits.                                                                                    */
SFL_API int sfl_batch_history_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps);
/* Copy members [first, first + count) of samples [first_sample, first_sample + samples) out, sample-major: record
 * [s][m] at host[s * count + m].  The numbers are the batch's member numbers and must lie inside the recorded range.
 * Samples are not consumed.  Synchronous.  No history: SFL_ERR_STATE.  b NULL, host NULL (bytes > 0), first_sample or
 * samples < 0, a sample range that is not inside the samples written, count < 1, a member range that is not inside the
 * recorded one and bytes != samples * count * 64 return SFL_ERR_INVALID.                                                */
SFL_API int sfl_batch_history_read(sfl_batch *b, int first_sample, int samples, int first, int count,
                                   struct sfl_history_record *host, size_t bytes);
/* The same for a whole-domain context: one record per sample, bytes == samples * 64.  A sample is the passes of
 * sfl_flow_stats and sfl_residual launched on the context's stream and pointed at the record; the words the host knows
 * (what, iterations, step, dt, dx) are merged in when the records are read.                                             */
SFL_API int sfl_history_start(sfl_context *ctx, int every, int capacity);
SFL_API int sfl_history_stop(sfl_context *ctx);
SFL_API int sfl_history_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps);
SFL_API int sfl_history_read(sfl_context *ctx, int first_sample, int samples, struct sfl_history_record *host,
                             size_t bytes);
/* --- SOLIDS: solid cells inside the grid of a batch member.  A mask marks cells as solid; every other cell is fluid.  The
 *     rule below extends the reference's wall rule inward -- a solid neighbour is one more reason for a neighbour to be
 *     absent -- and is a definition stated here, like the vorticity's: the reference knows no wall but the rim of its grid.
 *     A neighbour of a cell is PRESENT when it is inside the domain and fluid.  With no solid cell the rule's step is
 *     sfl_batch_step_n's bit for bit; a grid whose outer ring is solid computes in its inner cells, bit for bit, the
 *     divergence, the solve and the gradient of the plain grid of those inner cells (the ring shifts (i, j) by (1, 1): the
 *     colouring is kept), and so a whole step at dt = 0.
 *   ONE STEP, in the order of sfl_step:
 *     1. velocity advection  unchanged, advect(..., no_slip) on EVERY cell, reading the velocity as it stands: no special
 *                            sampling near a solid.  Solid nodes hold zero velocity; the bilinear gather decays towards them.
 *     2. forces              in queue order, unchanged.
 *     3. zero the solids     after 1 and 2 the velocity of every solid cell is (0, 0): a force record on a solid cell has no
 *                            effect.
 *     4. divergence          of a fluid cell with all four neighbours present ((-W.x + E.x) + (-S.y + N.y)) * k; otherwise
 *                            0.0f plus the four terms in the order W, E, S, N, then * k, an absent neighbour's term being the
 *                            cell's own component with the ghost's sign: own.x for W, -own.x for E, own.y for S, -own.y for
 *                            N.  k = 1.0f / (2.0f * dx).  A solid cell's divergence is 0.0f.
 *     5. pressure            p = 0 everywhere; solid cells are never updated and never read.  A fluid cell relaxes as in
 *                            sfl_poisson_solve with `present` counting its present neighbours: the sum is
 *                            (((z + W) + E) + S) + N with -0.0f for an absent neighbour, z = -0.0f iff present == 4, else
 *                            +0.0f; p_gs = k * (dx * d - sum) with k = -0.25f, (float)(-1.0 / 3.0), -0.5f, -1.0f for present
 *                            = 4, 3, 2, 1 and k = 0.0f for present == 0 (a fluid cell walled in on all sides: the one case no
 *                            plain grid can produce); p = (1 - omega) * p + omega * p_gs.  The colour of a cell is (i + j) & 1
 *                            of the domain's coordinates, even first.
 *     6. gradient            of a fluid cell: an absent neighbour's pressure is the cell's own.  A solid cell's velocity stays
 *                            (0, 0), its pressure 0.
 *     7. dye                 unchanged, on every cell, with the projected velocity: a solid cell traces back to itself and
 *                            keeps its colour (less the UQ32 round trip of the first step).  Paint obstacles by uploading dye.
 *   TWO DIAGNOSTICS follow the rule.  The update norm of the _each calls (sfl_batch_residual) is the maximum over FLUID cells
 * of |p_gs - p| with the k, z and sum of item 5; a member without a fluid cell reports 0.0f.  max_abs_div of
 * sfl_batch_flow_stats[_each] is the maximum over all cells of item 4's divergence of the velocity held.
 *   WHICH CALLS HONOUR SOLIDS: sfl_batch_step_n, sfl_batch_step_n_each, sfl_batch_poisson_solve,
 * sfl_batch_poisson_solve_each and sfl_batch_flow_stats[_each], on a batch made by sfl_batch_create.  While solids are set a
 * step call runs one launch per step, as with following tracers, also where it would have replayed a timeline in one launch;
 * the results are the same either way.  Everything that forms neither a divergence nor a pressure works unchanged: render,
 * recorder, envelope, distance, tracers, and the speed, vorticity and pressure views -- the vorticity view reads the zero
 * velocity of solid cells through its ordinary stencil.
 *   REFUSED WHOLE with SFL_ERR_STATE, each with its own message: sfl_batch_set_solids on a batch of sfl_batch_create_large;
 * sfl_batch_step_n_until and sfl_batch_poisson_solve_until, sfl_batch_history_start and SFL_VIEW_DIVERGENCE (the view calls
 * and sfl_batch_record_view) while solids are set; sfl_batch_set_solids with a mask while a history is on or the recorder
 * draws the divergence view.  A call's own argument checks come first, and nothing is staged or launched by a refused call. */
/* Set the solids: mask = dim_y * dim_x bytes shared by all members (per_member 0), or batch * dim_y * dim_x bytes, member-
 * major (per_member 1); cell (i, j) at dim_x * j + i, nonzero = solid.  The mask is read during the call only.  mask NULL
 * clears the solids: the batch then launches exactly what it launched before they were set.  No field is touched -- a
 * velocity or a pressure already held by a cell that becomes solid goes with the next step (items 3 and 5).  Synchronous.
 * b NULL and per_member outside 0..1 return SFL_ERR_INVALID.                                                             */
SFL_API int sfl_batch_set_solids(sfl_batch *b, const uint8_t *mask, int per_member);
/* Whether solids are set, and whether per member.  Either out pointer may be NULL.  Never waits.                         */
SFL_API int sfl_batch_solids_info(sfl_batch *b, int *set, int *per_member);
/* The masks of members [first, first + count) as bytes 0 / 1, member-major (a shared mask: repeated; no solids: zeros);
 * bytes must be count * dim_y * dim_x.  Synchronous.                                                                     */
SFL_API int sfl_batch_solids_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes);
/* --- SOLIDS OF A CONTEXT: the same solid cells inside the grid of a whole-domain context, at any grid size.  The rule is the
 *     one of "SOLIDS" above, items 1 to 7, unchanged: one step of a context with solids set computes, bit for bit, what one
 *     step of a batch member of the same shape with the same mask computes, and with no solid cell in the mask what the
 *     context computes without one.
 *   WHICH CALLS HONOUR SOLIDS while a mask is set:
 *     sfl_step, sfl_step_n      items 1 to 7 as ONE UNFUSED SEQUENCE per step: the velocity advection and the forces as ever,
 *                               the divergence by item 4 (the same pass stores (0, 0) into the solid cells' velocity, item 3),
 *                               the solve by item 5, the gradient by item 6, the dye advection as ever.  No step seams
 *                               (SFL_OPT_STEP_SEAMS), no fused advection + divergence or projection, and no one-launch step of
 *                               a small grid (SFL_OPT_SMALL_GRID): those kernels derive their walls from coordinates.
 *     sfl_calculate_divergence  item 4 on the velocity held.  An absent neighbour is never read, so what the solid cells'
 *                               velocity holds does not matter; it is not touched.
 *     sfl_poisson_solve         item 5, from p = 0.
 *     sfl_poisson_continue      item 5's iterations on the pressure held.
 *     sfl_subtract_gradient     item 6; writes (0, 0) into solid cells.
 *     sfl_residual              the masked update norm: the maximum over the fluid cells, 0.0f when there is none.
 *     sfl_poisson_solve_until   the rule of that call as a loop on the host over the two calls above, on grids of every size.
 *     sfl_flow_stats            max_abs_div by item 4; the other figures as ever.
 *     sfl_history_*             a sample's max_abs_div and update_norm are what sfl_flow_stats and sfl_residual return after
 *                               the same step, so they follow the rule too.
 *   The masked solve runs ceil(iters / 8) launches of a kernel of its own between the pressure and its ping-pong partner
 * (sfl_last_solve_info reports them).  That kernel knows only the rule's arithmetic: SFL_OPT_SOR_FOLD, SFL_OPT_SOR_KERNEL,
 * SFL_OPT_SOR_FUSE and SFL_OPT_SOR_ROWS have no effect while solids are set.
 *   UNCHANGED: sfl_advect_velocity and sfl_advect_color called on their own, upload and download, render, sfl_distance,
 * tracers, and the speed, vorticity and pressure views.
 *   REFUSED WHOLE with SFL_ERR_STATE, each with its own message and with nothing staged or launched: sfl_set_solids with a
 * mask on a slab (nranks != 1) or on a context that has a transport attached; sfl_comm_attach, sfl_comm_emulate,
 * sfl_comm_emulate_rccl and sfl_group_link while solids are set; SFL_VIEW_DIVERGENCE through sfl_view_scalar, sfl_view_texels
 * and sfl_view_render while solids are set.  A call's own argument checks come first.                                      */
/* Set the solids: mask = dim_y * dim_x bytes, cell (i, j) at dim_x * j + i, nonzero = solid; read during the call only.
 * mask NULL clears the solids: the context then launches exactly what it launched before they were set -- the one-launch
 * step of a small grid, the fused kernels and the step seams included.  No field is touched -- a velocity or a pressure
 * already held by a cell that becomes solid goes with the next step (items 3 and 5).  Synchronous.  ctx NULL returns
 * SFL_ERR_INVALID.                                                                                                         */
SFL_API int sfl_set_solids(sfl_context *ctx, const uint8_t *mask);
/* Whether solids are set, and how many cells of the mask are solid (0 when none is set).  Either out pointer may be NULL.
 * Never waits.                                                                                                             */
SFL_API int sfl_solids_info(sfl_context *ctx, int *set, int64_t *solid_cells);
/* The mask as bytes 0 / 1 (no solids: zeros); bytes must be dim_y * dim_x.  Synchronous.                                   */
SFL_API int sfl_solids_download(sfl_context *ctx, uint8_t *host, size_t bytes);
/* --- LOADS: how hard the flow pushes on solid bodies -- the pressure force on every body, as figures (sfl_batch_loads,
 *     sfl_loads) and as curves recorded while stepping (sfl_batch_loads_start, sfl_loads_start), without a download.  The rule
 *     below is a definition stated here, like the vorticity's and the solids': the reference knows no bodies.  It is the
 *     PRESSURE load only -- no viscous and no momentum-flux part -- and there is no torque.
 *   FACES.  A wet face is a pair (fluid cell F, solid cell S) where S is one of F's four neighbours, S is INSIDE THE DOMAIN
 * and S belongs to a body.  The rim of the grid is not a body and has no faces.
 *   BODIES.  Without labels every solid cell is body 1 and `bodies` is 1.  sfl_batch_set_bodies / sfl_set_bodies give one byte
 * per cell: 0 = in no body (a channel wall that is not wanted in the drag), 1..bodies = that body, bodies <= SFL_MAX_BODIES.
 * A label counts only where the cell is solid at the time of the sample; labels and masks are independent of each other,
 * either may be set first, and either may be shared by all members or per member.
 *   THE RECORD, per body, over its wet faces, from the pressure held (p of the face is the pressure of its FLUID cell):
 *     nonfinite   the number of faces whose pressure is NaN or +-Inf; those faces take no further part;
 *     max_abs_p   the maximum of |p| over the remaining faces; 0.0f when there is none;
 *     exp2        q = floor(log2(max_abs_p)) - 32, denormals included: frexp((double)max_abs_p)'s exponent - 1 - 32; q = 0 when
 *                 max_abs_p == 0;
 *     a face's term  t = (int64_t)trunc(ldexp((double)p, -q)): exact in double, |t| < 2^33; the largest face keeps all of its
 *                 24 bits, and a face is truncated only below 2^-32 of the largest;
 *     fx          the sum of t over the faces whose fluid cell lies WEST of its solid cell minus the sum over those whose
 *                 fluid cell lies EAST of it; fy the same with SOUTH and NORTH: pressure pushes the body away from the fluid;
 *     faces[4]    the numbers of faces whose fluid cell lies W, E, S, N of the solid cell; faces[0] is the frontal area
 *                 of a flow in +x.
 *   A context holds at most 2^28 cells, hence fewer than 2^30 faces, and |sum| < 2^30 * 2^33 = 2^63: fx and fy never overflow.
 *   The load in pressure times cell widths is fx * 2^exp2 (fy * 2^exp2); the caller multiplies by dx.  All zeros mean a body
 * without a face, or no solids set.  Integer sums, maxima over bit patterns and counts do not depend on the order of
 * reduction: every field of every record is, bit for bit, what the rule computes from the downloaded pressure, mask and
 * labels, and a context and a batch member of the same shape, mask, labels and pressure report the same bytes.
 *   THE RECORDER follows the histories' rules unchanged: after every `every`-th step of ANY step call -- counted across calls
 * -- one launch on the stream (a context: two) writes count * bodies records from the fields that step left; the step calls
 * stay asynchronous; a step call whose steps would complete more samples than are free is refused WHOLE with SFL_ERR_STATE
 * before anything is staged or launched; a restart keeps the buffer; sample s belongs to step (s + 1) * every since the
 * start.  A sample taken while no solids are set is zero records (a batch's one-launch replay of a timeline only runs
 * without solids: the samples that fall inside it are zeros).  A loads recorder changes no result and, unlike a history, not
 * even which step launches a call makes; with none on, every call launches exactly what it launched before there were loads.
 *   Admission as everywhere: a call's own argument checks come first, then the state refusals, each with its own message;
 * a refused call stages and launches nothing.  (The tangential viscous force on the same bodies: "FRICTION", below.)        */
#define SFL_MAX_BODIES 16
struct sfl_body_load {
    int64_t  fx, fy;
    int32_t  exp2;
    float    max_abs_p;
    uint32_t faces[4];
    uint32_t nonfinite, reserved;
};                                     /* 48 bytes: offsets 0, 8, 16, 20, 24, 40, 44 */
/* Label the bodies: labels = dim_y * dim_x bytes shared by all members (per_member 0) or batch * dim_y * dim_x bytes, member-
 * major (per_member 1), cell (i, j) at dim_x * j + i; read during the call only.  labels NULL goes back to "every solid cell
 * is body 1" (bodies is then 1, whatever is passed).  Batches of either kind.  Synchronous.  b NULL, per_member outside 0..1,
 * bodies outside 1..SFL_MAX_BODIES and a label > bodies (the message names the first such cell) return SFL_ERR_INVALID; while
 * the loads recorder is on the call is refused with SFL_ERR_STATE: the layout of its samples depends on `bodies`.           */
SFL_API int sfl_batch_set_bodies(sfl_batch *b, const uint8_t *labels, int per_member, int bodies);
/* The number of bodies, whether labels are set, and whether per member.  Any out pointer may be NULL.  Never waits.        */
SFL_API int sfl_batch_bodies_info(sfl_batch *b, int *bodies, int *labelled, int *per_member);
/* The labels of members [first, first + count), member-major (shared labels: repeated; no labels: every byte 1); bytes must
 * be count * dim_y * dim_x.  Synchronous.                                                                                  */
SFL_API int sfl_batch_bodies_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes);
/* The loads of members [first, first + count) from the pressure held: count * bodies records, member-major (record of body k
 * of member m at host[(m - first) * bodies + k - 1]); bytes must be count * bodies * 48.  One launch, synchronous; changes
 * no field.  A batch without solids set reports zero records without a launch.                                             */
SFL_API int sfl_batch_loads(sfl_batch *b, int first, int count, struct sfl_body_load *host, size_t bytes);
/* Start the recorder for members [first, first + count): `capacity` samples of count * bodies records are allocated on the
 * device and the step count is set to 0.  Called while it is on, it starts afresh; the buffer is reallocated only if it must
 * grow.  b NULL, every < 1, capacity < 1 (or too large for a size_t), count < 1 and a range outside the batch return
 * SFL_ERR_INVALID; a failed allocation returns SFL_ERR_NOMEM and leaves the batch without a recorder.                      */
SFL_API int sfl_batch_loads_start(sfl_batch *b, int every, int first, int count, int capacity);
/* Stop the recorder and free its samples (sfl_batch_destroy frees them too).  Without one: SFL_OK.                         */
SFL_API int sfl_batch_loads_stop(sfl_batch *b);
/* Samples written so far, the capacity, the steps counted since the start (all 0 without a recorder) and the number of
 * bodies.  Any out pointer may be NULL.  Never waits.                                                                      */
SFL_API int sfl_batch_loads_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies);
/* Copy samples [first_sample, first_sample + samples) out whole, sample-major: the record of body k of recorded member m of
 * sample s at host[(s * count + m) * bodies + k - 1]; bytes must be samples * count * bodies * 48.  Not consumed.
 * Synchronous.  No recorder: SFL_ERR_STATE.                                                                                */
SFL_API int sfl_batch_loads_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_load *host, size_t bytes);
/* The same for a whole-domain context: `bodies` records per sample.  A slab and a context with a transport attached get
 * SFL_ERR_STATE, as from sfl_set_solids.  A sample is two streaming passes over the code bytes, the maximum and then the
 * sums, behind a memset of the sample's records, all on the context's stream.                                              */
SFL_API int sfl_set_bodies(sfl_context *ctx, const uint8_t *labels, int bodies);
SFL_API int sfl_bodies_info(sfl_context *ctx, int *bodies, int *labelled);
SFL_API int sfl_bodies_download(sfl_context *ctx, uint8_t *host, size_t bytes);
SFL_API int sfl_loads(sfl_context *ctx, struct sfl_body_load *host, size_t bytes);
SFL_API int sfl_loads_start(sfl_context *ctx, int every, int capacity);
SFL_API int sfl_loads_stop(sfl_context *ctx);
SFL_API int sfl_loads_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies);
SFL_API int sfl_loads_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_load *host, size_t bytes);
/* --- VISCOSITY: an implicit diffusion of the velocity between the forces and the divergence, opt-in, per member in a batch and
 *     on whole-domain contexts of any size.  The reference knows no viscosity: the arithmetic below is a definition stated
 *     here, like the vorticity's, the solids' and the loads'.  It is anchored on the reference through nu = 0, which gives the
 *     existing step bit for bit.
 *   ITEM 3a OF A STEP.  It runs behind items 1 to 3 of "SOLIDS" (velocity advection, forces, solids zeroed) and in front of
 * item 4 (divergence); in a step without solids, between the forces and the divergence.
 *   SKIPPED WHOLE for a member or a context whose nu == 0.0f or whose sweeps == 0: nothing is computed and no bit changes (a
 * zero coefficient would turn a -0.0f into +0.0f).
 *   COEFFICIENTS.  a = (nu * dt) / (dx * dx) and c = 1.0f / (1.0f + 4.0f * a), both float32, every operation rounded on its
 * own; formed once on the host per call, or per member in the _each call with that member's dt and dx.
 *   THE SWEEPS.  u0 is the velocity that items 1 to 3 left; u starts as u0.  `sweeps` times: first colour 0 -- (i + j) & 1 == 0
 * in domain coordinates --, then colour 1; for every FLUID cell of the colour and for each component q of x, y:
 *     u.q = (u0.q + a * (((W.q + E.q) + S.q) + N.q)) * c
 * A neighbour OUTSIDE THE DOMAIN contributes -u.q, the cell's own component as it stands before this update, negated: the
 * no-slip ghost, zero velocity half a cell beyond the rim node, as in sample() of advect.h.  A SOLID neighbour inside the
 * domain is read as what it holds -- after item 3 that is (0, 0): the node-based wall that item 1 already uses.  Solid cells
 * are never updated.  A colour's cell reads only itself and the other colour: the result does not depend on the order of
 * execution.  Compiled with -ffp-contract=off, as everything.
 *   WHICH CALLS HONOUR VISCOSITY.  Batches of sfl_batch_create: sfl_batch_step_n and sfl_batch_step_n_each, with and without
 * solids set.  While viscosity is set a step call runs one launch per step, as with solids; it does not replay a timeline in
 * one launch.  A batch with viscosity set whose members all have nu = 0 runs the viscous kernels and gives the plain batch's
 * bits.  Everything that only reads fields works unchanged: render, recorder, envelope, distance, tracers, views,
 * sfl_batch_flow_stats, histories and loads.  Whole-domain contexts of any size: sfl_step and sfl_step_n run ONE UNFUSED
 * SEQUENCE per step -- the velocity advection, the forces, the diffusion (with solids set its first launch reads the solid
 * cells' velocity as (0, 0) and stores it so: item 3), then the divergence, the solve, the gradient and the dye advection
 * as the calls of their own run them, by the solids' rule where a mask is set.  No step seams, no fused kernels, no
 * one-launch step of a small grid.  sfl_diffuse_velocity is item 3a as an operator of its own.  The diffusion of a context
 * is blocked in time: ceil(sweeps / 8) launches; more than 8 sweeps need a third velocity-sized buffer, allocated at the
 * first such call (a failed allocation returns SFL_ERR_NOMEM), fewer allocate nothing.
 *   REFUSED WHOLE with SFL_ERR_STATE, each with its own message and with nothing staged or launched: sfl_batch_set_viscosity
 * on a batch of sfl_batch_create_large (its 8 B of LDS per cell leave no room for u0); sfl_batch_step_n_until while
 * viscosity is set; sfl_set_viscosity and sfl_diffuse_velocity with nu > 0 on a slab (nranks != 1) or on a context that has a
 * transport attached; sfl_comm_attach, sfl_comm_emulate, sfl_comm_emulate_rccl and sfl_group_link while viscosity is set.  A
 * call's own argument checks come first: SFL_ERR_INVALID for a NULL handle, a negative or NaN nu (a batch: the message names
 * the first such member), sweeps < 0, per_member outside 0..1 and wrong download sizes.
 *   NOT THERE: viscosity on the batches of sfl_batch_create_large, in the _until calls and on slabs; a viscous part of the
 * loads; diffusion of the dye.                                                                                             */
/* Set the viscosity of a whole-domain context: from now on sfl_step and sfl_step_n run item 3a with this nu and `sweeps`
 * sweeps.  nu == 0 or sweeps == 0 clears it: every call then launches exactly what it launched before.  Never waits.       */
SFL_API int sfl_set_viscosity(sfl_context *ctx, float nu, int sweeps);
/* What is set (0.0f and 0 when nothing is).  Either out pointer may be NULL.  Never waits.                                 */
SFL_API int sfl_viscosity_info(sfl_context *ctx, float *nu, int *sweeps);
/* Item 3a on the velocity held, beside sfl_calculate_divergence and its siblings: its own arguments, nothing needs to be
 * set.  Honours the context's solids where set (a solid cell is not updated and is read as what it holds; nothing is
 * zeroed).  Touches neither the pressure nor the divergence.  nu == 0 or sweeps == 0 launch nothing.  Asynchronous.        */
SFL_API int sfl_diffuse_velocity(sfl_context *ctx, float nu, float dt, float dx, int sweeps);
/* Set the viscosity of a batch: nu = one float for all members (per_member 0) or `batch` floats (per_member 1), read during
 * the call only.  nu NULL clears it: the batch then launches exactly what it launched before.  Never waits.                */
SFL_API int sfl_batch_set_viscosity(sfl_batch *b, const float *nu, int per_member, int sweeps);
/* Whether viscosity is set, whether per member, and the sweeps.  Any out pointer may be NULL.  Never waits.                */
SFL_API int sfl_batch_viscosity_info(sfl_batch *b, int *set, int *per_member, int *sweeps);
/* nu of members [first, first + count) (a shared nu: repeated; none set: zeros); bytes must be count * 4.  Never waits.    */
SFL_API int sfl_batch_viscosity_download(sfl_batch *b, int first, int count, float *host, size_t bytes);
/* --- OPENINGS: inflow and outflow cells on the rim of the grid of a batch member, so that a flow enters on one side and
 *     leaves on another instead of circulating in a closed box.  The reference knows no opening: the rule below is a
 *     definition stated here, like the solids', the loads' and the viscosity's.  It is anchored on what exists: a map
 *     without an opening gives the bits of "SOLIDS", and with no solid cell either those of sfl_batch_step_n.
 *   THE MAP.  One byte per cell: 0 = closed, SFL_OPEN_INFLOW, SFL_OPEN_OUTFLOW.  A nonzero byte is allowed only on a rim cell
 * that is no corner: such a cell has exactly one neighbour outside the domain, and that side is the opening's.  An opening
 * counts only where the cell is fluid at the time, as a body label counts only where the cell is solid; maps and masks are
 * independent of each other, either may be set first, and either may be shared by all members or per member.
 *   THE INFLOW VELOCITY is one (x, y) for all members or one per member -- one batch is then a sweep over the tunnel speed.
 * It must be finite.  sfl_batch_set_inflow changes it without restaging the map.
 *   THE RULE extends items 1 to 7 of "SOLIDS".  An OPEN neighbour is the outside neighbour of a fluid cell whose byte is
 * nonzero; it is absent in the solids' sense.
 *     2a. inflow            after the forces every fluid inflow cell holds the inflow velocity, both components: a force
 *                           record on an inflow cell has no effect.  Then item 3 as ever.
 *     4. divergence         a cell with an open neighbour takes the safe form, 0.0f plus the four terms in the order W, E, S,
 *                           N.  The open neighbour's term is the cell's own component with the sign OPPOSITE to a wall's:
 *                           -own.x for W, +own.x for E, -own.y for S, +own.y for N -- the ghost moves with the cell and the
 *                           flow passes.  Both kinds.
 *     5. pressure           n = present + 1 if the open neighbour is an OUTFLOW, else n = present.  k comes from n by the
 *                           table of "SOLIDS" (n = 4: -0.25f).  z stays -0.0f iff all four neighbours are present, so it is
 *                           +0.0f here, and the open neighbour contributes -0.0f to the sum as an absent one does.  An outflow
 *                           is a ghost pressure of zero that counts as a neighbour; an inflow is a wall to the pressure.  The
 *                           update norm uses the same k.
 *     6. gradient           an outflow neighbour's pressure is +0.0f; an inflow neighbour's is the cell's own.
 *   Items 1, 3 and 7 are unchanged.  The free-slip dye clamps at the rim, so an inflow cell's colour enters with the flow.
 *   An inflow without any outflow is accepted: the Neumann problem is then incompatible and the solve drifts.
 *   WHICH CALLS HONOUR OPENINGS, on a batch made by sfl_batch_create, with and without solids set: sfl_batch_step_n and
 * sfl_batch_step_n_each (one launch per step, as with solids), sfl_batch_poisson_solve[_each], sfl_batch_flow_stats[_each]
 * (max_abs_div follows item 4) and sfl_batch_residual.  Item 2a runs only in the step calls.  With openings and no mask the
 * library forms the codes of an all-fluid grid itself; sfl_batch_solids_info still reports "not set".  Loads, render,
 * recorder, envelope, distance, tracers and the speed, vorticity and pressure views work unchanged.
 *   REFUSED WHOLE with SFL_ERR_STATE, each with its own message and with nothing staged or launched: sfl_batch_set_openings
 * with a map on a batch of sfl_batch_create_large, while a history is on, while the recorder draws the divergence view and
 * while viscosity is set; sfl_batch_step_n_until, sfl_batch_poisson_solve_until, sfl_batch_history_start,
 * SFL_VIEW_DIVERGENCE and sfl_batch_set_viscosity with a nu while openings are set.  A call's own argument checks come first:
 * SFL_ERR_INVALID for a NULL handle, flags outside 0..1, a byte above 2 or a nonzero byte on a corner or an interior cell (the
 * message names the first such cell), a non-finite inflow (the first such member) and wrong download sizes.
 *   A CHANGE OF THE MASK behind a map (sfl_batch_set_solids, sfl_set_solids) forms the openings' codes again.  If that fails
 * (SFL_ERR_NOMEM, SFL_ERR_HIP) the call returns the error with the mask as it asked for and the openings OFF: the one case in
 * which a failing call leaves a change behind.  Set the map again.
 *   NOT THERE: openings together with viscosity and in the viscous kernels; openings on slabs and on the batches of
 * sfl_batch_create_large.  (A per-cell inflow profile and a flux diagnostic, once listed here, are the calls of "INFLOW
 * PROFILES AND FLUX" below.)                                                                                               */
#define SFL_OPEN_INFLOW  1
#define SFL_OPEN_OUTFLOW 2
/* Set the openings: open = dim_y * dim_x bytes shared by all members (per_member 0) or batch * dim_y * dim_x bytes, member-
 * major (per_member 1), cell (i, j) at dim_x * j + i; inflow = one (x, y) for all members (inflow_per_member 0) or `batch` of
 * them (1).  Both are read during the call only.  open NULL clears the openings (inflow is then ignored): the batch then
 * launches exactly what it launched before they were set.  No field is touched.  Synchronous.                             */
SFL_API int sfl_batch_set_openings(sfl_batch *b, const uint8_t *open, int per_member, const float *inflow, int inflow_per_member);
/* Change the inflow velocity of a batch that has openings set (without: SFL_ERR_STATE).  The map stays.  Synchronous.      */
SFL_API int sfl_batch_set_inflow(sfl_batch *b, const float *inflow, int per_member);
/* Whether openings are set, whether the map and the inflow are per member, and the numbers of live -- fluid -- inflow and
 * outflow cells over all members (a shared map counts once per member).  Any out pointer may be NULL.  Never waits.        */
SFL_API int sfl_batch_openings_info(sfl_batch *b, int *set, int *per_member, int *inflow_per_member, int64_t *inflow_cells,
                                    int64_t *outflow_cells);
/* The maps of members [first, first + count) as given, member-major (a shared map: repeated; none set: zeros); bytes must be
 * count * dim_y * dim_x.  Never waits.                                                                                     */
SFL_API int sfl_batch_openings_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes);
/* The inflow (x, y) of members [first, first + count) (shared: repeated; none set: zeros); bytes must be count * 8.  Never
 * waits.                                                                                                                   */
SFL_API int sfl_batch_inflow_download(sfl_batch *b, int first, int count, float *host, size_t bytes);
/* --- OPENINGS OF A CONTEXT: the same openings on the rim of a whole-domain context, at any grid size.  The map, the rule and
 *     the inflow are those of "OPENINGS" above, unchanged, with ONE inflow velocity per context: one step of a context with
 *     openings set computes, bit for bit, what one step of a batch member of the same shape with the same map, mask and inflow
 *     computes, and with no opening in the map what the context computes without one.
 *   WHICH CALLS HONOUR OPENINGS while a map is set, with and without a mask, as the calls of "SOLIDS OF A CONTEXT" honour solids:
 *     sfl_step, sfl_step_n      ONE UNFUSED SEQUENCE per step: the velocity advection, the forces, item 2a over a compact list
 *                               of the fluid inflow cells, the divergence (which also zeroes the solid cells), the solve, the
 *                               gradient, the dye advection.  Item 2a runs only here: the operators never impose the inflow.
 *     sfl_calculate_divergence, sfl_poisson_solve, sfl_poisson_continue, sfl_subtract_gradient   items 4, 5, 5 and 6.
 *     sfl_residual, sfl_poisson_solve_until, sfl_flow_stats, sfl_history_*   the update norm with the k of item 5 and
 *                               max_abs_div by item 4; a history's sample is what the two calls return after the same step.
 *   The solve is the masked solve's tile, ceil(iters / 8) launches, with k set up from n.  With openings and no mask the library
 * forms the codes of an all-fluid grid itself; sfl_solids_info still reports "not set".  Loads, render, sfl_distance, tracers
 * and the speed, vorticity and pressure views work unchanged.
 *   REFUSED WHOLE with SFL_ERR_STATE, each with its own message and with nothing staged or launched: sfl_set_openings with a map
 * on a slab (nranks != 1), on a context that has a transport attached and while viscosity is set; sfl_comm_attach,
 * sfl_comm_emulate, sfl_comm_emulate_rccl and sfl_group_link, SFL_VIEW_DIVERGENCE and sfl_set_viscosity with a nu while openings
 * are set.  A call's own argument checks come first: a NULL handle, a non-finite inflow, a bad map (the message names the first
 * such cell) and a wrong download size return SFL_ERR_INVALID.                                                              */
/* Set the openings: open = dim_y * dim_x bytes, cell (i, j) at dim_x * j + i, read during the call only.  open NULL clears them
 * (the inflow is then ignored): the context then launches exactly what it launched before.  No field is touched.  Synchronous. */
SFL_API int sfl_set_openings(sfl_context *ctx, const uint8_t *open, float inflow_x, float inflow_y);
/* Change the inflow velocity of a context that has openings set (without: SFL_ERR_STATE).  The map stays.  Never waits.    */
SFL_API int sfl_set_inflow(sfl_context *ctx, float inflow_x, float inflow_y);
/* Whether openings are set, the inflow, and the numbers of live -- fluid -- inflow and outflow cells.  Any out pointer may be
 * NULL.  Never waits.                                                                                                      */
SFL_API int sfl_openings_info(sfl_context *ctx, int *set, float *inflow_x, float *inflow_y, int64_t *inflow_cells,
                              int64_t *outflow_cells);
/* The map as given (none set: zeros); bytes must be dim_y * dim_x.  Never waits.                                           */
SFL_API int sfl_openings_download(sfl_context *ctx, uint8_t *host, size_t bytes);
/* --- INFLOW PROFILES AND FLUX: an inflow velocity per cell instead of one per member or context -- parabolic inlets, shear
 *     layers, jets --, and how much fluid enters and leaves through the openings, without a download.  Both extend "OPENINGS"
 *     and "OPENINGS OF A CONTEXT" by calls of their own; with no profile set and no flux call made, every call launches exactly
 *     what it launched before.
 *   A PROFILE is a set of records (cell (i, j), velocity (u, v)).  It extends item 2a: after the forces, a fluid inflow cell
 * named by a record holds that record's velocity, both components; every other fluid inflow cell holds the uniform inflow as
 * before.  A force record on a profiled cell has no effect, as on any inflow cell.  Items 1, 3 and 4 to 7 are unchanged.
 *     - A record must name a cell whose map byte is SFL_OPEN_INFLOW -- in a batch with per-member maps, in the map of every
 *       member the record applies to.  Otherwise the call returns SFL_ERR_INVALID and the message names the first offending
 *       record, and the member where there is one.  The velocity must be finite.
 *     - Of two records on one cell of one member the later wins.  The host removes the duplicates: the device sees unique
 *       cells, and the result does not depend on the order of execution.
 *     - A record on an inflow cell that is solid at the time has no effect: an opening counts only where the cell is fluid.
 *       The record is kept, and counts again when the cell is fluid again.
 *     - A call replaces the profile that was set; n == 0 clears it.  A new map (sfl_batch_set_openings, sfl_set_openings) drops
 *       the profile; a new uniform inflow (sfl_batch_set_inflow, sfl_set_inflow) keeps it -- with a profile set, sfl_set_inflow
 *       forms the context's table again and waits for the stream.
 *     - A CHANGE OF THE MASK behind a map forms the profile's device table again together with the openings' codes; the rule
 *       for a failure there, in "OPENINGS", covers it: the openings go OFF, and the profile with them.
 *     - ANCHOR: a profile that gives every inflow cell the uniform inflow velocity produces the bits of no profile.
 *   A batch keeps the profile as one table on the device, staged once per change of the profile, the map or the mask, never
 * per step, and steps through kernels of its own (sfl_batch_step_n, sfl_batch_step_n_each; one launch per step, as with
 * openings alone); without a profile it launches what it launched before.  A context runs item 2a over its compact list with
 * one velocity per list entry: the record's where there is one, the uniform inflow elsewhere.
 *   THE FLUX is computed from the velocity HELD, over the LIVE OPEN CELLS: the fluid cells with a nonzero map byte.  After a
 * step the inflow cells hold the inflow MINUS the pressure gradient of item 6: the figure is what actually enters, not what
 * was imposed.  The quantisation is that of "LOADS", word for word:
 *     n              the outward normal component of the cell's velocity: -v.x on the W rim, +v.x on E, -v.y on S, +v.y on N;
 *     nonfinite      the number of live open cells whose n is NaN or +-Inf; those cells take no further part;
 *     max_abs_n      the maximum of |n| over the remaining cells of both kinds; 0.0f when there is none;
 *     exp2           q = floor(log2(max_abs_n)) - 32, denormals included, exactly as exp2 of "LOADS"; q = 0 when max_abs_n == 0.
 *                    ONE q serves both sums, so that inflow - outflow is itself an exact integer;
 *     a cell's term  t = (int64_t)trunc(ldexp((double)n, -q)), |t| < 2^33;
 *     inflow         minus the sum of t over the live inflow cells: positive when fluid enters;
 *     outflow        the sum of t over the live outflow cells: positive when fluid leaves;
 *     inflow_cells, outflow_cells   the numbers of live cells of each kind.
 *   A side of the largest context has fewer than 2^16 rim cells: the sums cannot overflow.  The flux in velocity times cell
 * widths is inflow * 2^exp2 (outflow * 2^exp2); the caller multiplies by dx.  With no openings set, or with no live open cell,
 * the record is all zeros and no launch is made.  Integer sums, counts and maxima over bit patterns do not depend on the order
 * of reduction: every field is, bit for bit, what the rule computes from the downloaded velocity, map and mask, and a context
 * and a batch member of the same shape report the same bytes.  A batch: one launch, one workgroup per member over the rim
 * cells of the member; a context: one launch of one workgroup over the 2 (dim_x + dim_y) - 4 rim cells, never a pass over the
 * grid.  No atomics, no float sums.
 *   Admission as everywhere.  A call's own argument checks come first, SFL_ERR_INVALID and answered on a machine without a GPU
 * where they need no handle: n < 0, NULL arrays with n > 0, a non-finite velocity (the message names the record), a NULL
 * handle, a member outside the batch, a wrong size.  The state refusals come next, each with its own message: a profile on a
 * batch of sfl_batch_create_large and a profile without openings set give SFL_ERR_STATE -- so everything that
 * sfl_[batch_]set_openings refuses stays refused: without openings there is no profile.  Then the records against the map.  A
 * refused call stages and launches nothing and leaves the profile as it was.                                                */
struct sfl_open_flux {
    int64_t  inflow, outflow;
    int32_t  exp2;
    float    max_abs_n;
    uint32_t inflow_cells, outflow_cells, nonfinite, reserved;
};                                     /* 40 bytes: offsets 0, 8, 16, 20, 24, 28, 32, 36 */
/* Set the inflow profile of a context: record k is cell (cells_ij[2 k], cells_ij[2 k + 1]) with velocity (vel_xy[2 k],
 * vel_xy[2 k + 1]); both arrays are read during the call only.  n == 0 clears the profile (the arrays may then be NULL).
 * Synchronous.                                                                                                             */
SFL_API int sfl_set_inflow_profile(sfl_context *ctx, const int *cells_ij, const float *vel_xy, int n);
/* The number of unique cells the profile holds (0 without one).  Never waits.                                              */
SFL_API int sfl_inflow_profile_info(sfl_context *ctx, int *records);
/* The records held, in cell-index order (dim_x * j + i ascending); capacity counts records, and capacity < records returns
 * SFL_ERR_INVALID.  Never waits.                                                                                           */
SFL_API int sfl_inflow_profile_download(sfl_context *ctx, int *cells_ij, float *vel_xy, int capacity);
/* The flux record of the velocity held.  One launch, synchronous; changes no field.                                        */
SFL_API int sfl_openings_flux(sfl_context *ctx, struct sfl_open_flux *out);
/* Set the inflow profile of a batch made by sfl_batch_create, in the idiom of sfl_batch_queue_forces: record k belongs to
 * member members[k]; members == NULL gives every record to every member.  n == 0 clears the profile.  Synchronous.          */
SFL_API int sfl_batch_set_inflow_profile(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n);
/* Whether a profile is set, and the number of unique cells held over all members (a shared profile counts once per member).
 * Either out pointer may be NULL.  Never waits.                                                                            */
SFL_API int sfl_batch_inflow_profile_info(sfl_batch *b, int *set, int64_t *records);
/* The records of one member, in cell-index order; *records (may be NULL) gets their number; capacity < that number returns
 * SFL_ERR_INVALID with *records set.  Never waits.                                                                         */
SFL_API int sfl_batch_inflow_profile_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records);
/* The flux records of members [first, first + count) from the velocity held: host[m - first] is member m's; bytes must be
 * count * 40.  One launch, synchronous; changes no field.  A batch without openings reports zero records without a launch.  */
SFL_API int sfl_batch_openings_flux(sfl_batch *b, int first, int count, struct sfl_open_flux *host, size_t bytes);
/* --- FRICTION: how hard the flow DRAGS solid bodies along -- the skin friction on every body, beside the pressure load of
 *     "LOADS": as figures (sfl_batch_friction, sfl_friction) and as curves recorded while stepping (sfl_batch_friction_start,
 *     sfl_friction_start), without a download.  The rule below is a definition stated here, like the loads': the reference
 *     knows no bodies.  It is the TANGENTIAL viscous force only: the normal viscous stress 2 nu dv_n/dn is left out -- it
 *     vanishes at a no-slip wall of a divergence-free flow -- and there is no torque.
 *   FACES AND BODIES are those of "LOADS", word for word: a wet face is a pair (fluid cell F, solid cell S) where S is one of
 * F's four neighbours, S is INSIDE THE DOMAIN and S belongs to a body; the rim has no faces; labels, `bodies` and
 * SFL_MAX_BODIES come from sfl_batch_set_bodies / sfl_set_bodies; a label counts only where the cell is solid at the time of
 * the sample.  For the same mask and labels, faces[4] of a friction record equals faces[4] of the load record.
 *   THE WALL IS AT REST AND LIES AT NODE S, the node-based wall of items 1 and 3a.  The shear on the face is
 * nu * (tangential velocity of F) / dx; over a face of length dx the force is nu * (tangential velocity of F): the face's
 * term is F's tangential component alone.
 *     F lies W or E of S (directions 0 and 1): the term is v.y and goes into fy;
 *     F lies S or N of S (directions 2 and 3): the term is v.x and goes into fx.
 * The sign is plain -- the fluid drags the body along with it: no subtraction between sides.  A fluid cell with several
 * faces contributes once per face, possibly to different bodies.
 *   THE RECORD, per body, over its wet faces, from the velocity held, with the quantisation of "LOADS" unchanged:
 *     nonfinite   the number of faces whose TANGENTIAL component is NaN or +-Inf; the normal component is not looked at;
 *                 those faces take no further part;
 *     max_abs_t   the maximum of |tangential component| over the remaining faces; 0.0f when there is none;
 *     exp2        q = floor(log2(max_abs_t)) - 32, denormals included, exactly as exp2 of "LOADS"; q = 0 when max_abs_t == 0.
 *                 ONE q serves both fx and fy;
 *     a face's term  t = (int64_t)trunc(ldexp((double)v_t, -q)), |t| < 2^33;
 *     fx          the sum of t over the faces whose fluid cell lies SOUTH or NORTH of its solid cell;
 *     fy          the sum of t over the faces whose fluid cell lies WEST or EAST of it;
 *     faces[4]    as in "LOADS": the numbers of faces whose fluid cell lies W, E, S, N of the solid cell.
 *   Fewer than 2^30 faces: the sums cannot overflow.
 *   The friction force on the body per unit depth is rho * nu * fx * 2^exp2 (rho * nu * fy * 2^exp2): there is NO FACTOR dx,
 * unlike the pressure load.  The library does not multiply by nu: the record is defined with or without a viscosity set, and
 * the caller supplies nu.  All zeros mean a body without a face, or no solids set.  Integer sums, maxima over bit patterns
 * and counts do not depend on the order of reduction: every field of every record is, bit for bit, what the rule computes
 * from the downloaded velocity, mask and labels, and a context and a batch member of the same shape, mask, labels and
 * velocity report the same bytes.  The pressure plays no part.
 *   THE FRICTION RECORDER follows the loads recorder's rules unchanged: steps count across calls; sample s belongs to step
 * (s + 1) * every; a step call without room for its samples is refused WHOLE with SFL_ERR_STATE before anything is staged or
 * launched, with a message that names the friction recorder; a restart keeps the buffer; a sample taken without solids is
 * zero records; a batch's one-launch replay of a timeline and the fused seams of sfl_step_n are NOT cut.  It is independent
 * of the loads recorder and of the history: any of the three may be on together, and behind a step the order is history,
 * loads, friction.  With no friction recorder on, every call launches exactly what it launched before there was one.
 * sfl_batch_set_bodies / sfl_set_bodies are refused with SFL_ERR_STATE while the friction recorder is on, with a message of
 * their own: the layout of its samples depends on `bodies` too.
 *   Admission as everywhere: the argument checks and their order are those of the loads' calls, one for one.  (The moment
 * of both forces about a pivot per body: "TORQUE", below.)                                                                  */
struct sfl_body_friction {
    int64_t  fx, fy;
    int32_t  exp2;
    float    max_abs_t;
    uint32_t faces[4];
    uint32_t nonfinite, reserved;
};                                     /* 48 bytes: offsets 0, 8, 16, 20, 24, 40, 44 -- those of sfl_body_load */
/* The friction records of members [first, first + count) from the velocity held: count * bodies records, member-major, as
 * sfl_batch_loads; bytes must be count * bodies * 48.  One launch, synchronous; changes no field.  A batch without solids set
 * reports zero records without a launch.  Batches of either kind.                                                          */
SFL_API int sfl_batch_friction(sfl_batch *b, int first, int count, struct sfl_body_friction *host, size_t bytes);
/* The friction recorder of a batch: the calls of the loads recorder, one for one (sfl_batch_loads_start, _stop, _info,
 * _read), with a buffer, a step count and samples of their own.                                                            */
SFL_API int sfl_batch_friction_start(sfl_batch *b, int every, int first, int count, int capacity);
SFL_API int sfl_batch_friction_stop(sfl_batch *b);
SFL_API int sfl_batch_friction_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies);
SFL_API int sfl_batch_friction_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_friction *host, size_t bytes);
/* The same for a whole-domain context: `bodies` records per sample.  A slab and a context with a transport attached get
 * SFL_ERR_STATE, as from sfl_loads.  A sample is two streaming passes over the code bytes, the maxima and then the sums,
 * behind a memset of the sample's records, all on the context's stream.                                                    */
SFL_API int sfl_friction(sfl_context *ctx, struct sfl_body_friction *host, size_t bytes);
SFL_API int sfl_friction_start(sfl_context *ctx, int every, int capacity);
SFL_API int sfl_friction_stop(sfl_context *ctx);
SFL_API int sfl_friction_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies);
SFL_API int sfl_friction_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_friction *host, size_t bytes);
/* --- AVERAGES: the time-averaged flow -- per-cell sums over time of the velocity, its second moments, the pressure and the
 *     dye, added on the device while stepping, without a download per sample.  Every other record of this library reports one
 *     instant; a wake or drag study is read through the mean velocity field, the mean pressure, the Reynolds stresses and
 *     the long exposure of the dye.  The accumulators live in device memory, one PLANE per quantity, one value per cell.
 *     After every `every`-th step of any step call ONE launch on the stream adds that step's fields to them; the step calls
 *     stay asynchronous, the host never waits, and the sums are downloaded afterwards.  The rule below is a definition stated
 *     here: the reference keeps no averages.
 *   `what` is a mask of four groups; only the planes of the chosen groups exist:
 *     SFL_MEAN_VELOCITY (1)   planes U (0), V (1)            float64   a sample adds (double)v.x, (double)v.y
 *     SFL_MEAN_STRESS   (2)   planes UU (2), VV (3), UV (4)  float64   (double)v.x * (double)v.x, (double)v.y * (double)v.y,
 *                                                                      (double)v.x * (double)v.y
 *     SFL_MEAN_PRESSURE (4)   planes P (5), PP (6)           float64   (double)p, (double)p * (double)p
 *     SFL_MEAN_DYE      (8)   planes R (7), G (8), B (9)     uint64    the raw UQ32 value of each channel
 *   Every plane STARTS AT +0.0 (0 for the dye planes).  A sample adds THE FIELDS HELD, exactly as the table says: the projected
 * velocity of the step it follows, the pressure of that step's solve (SFL_FIELD_PRESSURE as held) and that step's dye.  Every
 * cell takes part as it is, SOLID CELLS INCLUDED.
 *   A sample is ONE IEEE-754 DOUBLE ADDITION PER PLANE AND CELL, in sample order.  The product of two float32 values is exact
 * in a double (48 <= 53 bits), so a fused multiply-add gives the same bits as multiply-then-add and the rule needs no word
 * about contraction.  Special values are PLAIN IEEE: a NaN or +-Inf in a cell goes into that cell's sums as IEEE says and
 * into NO OTHER CELL'S; a float32 denormal converts exactly and is NEVER FLUSHED; +0.0 + (-0.0) is +0.0.
 *   Each cell's sum is sequential in time and integer sums do not depend on any order: every plane is, BIT FOR BIT, what the
 * rule computes from the downloaded fields.  That is the whole contract; there is NO TOLERANCE anywhere.  The dye sums cannot
 * wrap below 2^32 samples.
 *   THE MEANS ARE NOT THE LIBRARY'S: it reports SUMS and the number of samples.  The mean is sum / samples, and the central
 * moment <u'u'> = UU / n - (U / n)^2; the caller forms both (the Python binding does, in float64).  There is no division on
 * the device.
 *   `every` >= 1: steps count across calls, as the histories' do, and a sample is due after step (s + 1) * every.  While such
 * averages are on, a batch's one-launch replay of a timeline IS CUT at the steps whose sample is due, and sfl_step_n of a
 * context runs WITHOUT ITS FUSED STEP BOUNDARIES, every step as sfl_step runs it, exactly as with a history on: the sample
 * reads the projected velocity, which a fused boundary never stores.  `every` == 0: nothing is added behind the steps and no
 * hook is set -- the step calls keep their fusion and their one-launch replay -- and only sfl_mean_sample /
 * sfl_batch_mean_sample add.  Behind a step the order is tracers, history, loads, friction, averages.
 *   There is NO CAPACITY and so no admission rule: a step call is never refused for the averages.  With no averages on, every
 * call launches exactly what it launched before there were any.
 *   MEMORY: a plane is 8 bytes per cell and recorded member (a member's cells rounded up to an even number on the device).
 * Ten planes at 8192 x 8192 are 5.4 GB; choose the groups that are needed.  Out of memory is SFL_ERR_NOMEM with nothing set.
 *   Whole-domain contexts and batches of either kind; a slab and a context with a transport attached get SFL_ERR_STATE, each
 * with its own message.  Admission as everywhere: argument checks come first.                                              */
#define SFL_MEAN_VELOCITY 1
#define SFL_MEAN_STRESS   2
#define SFL_MEAN_PRESSURE 4
#define SFL_MEAN_DYE      8
#define SFL_MEAN_ALL      15
#define SFL_MEAN_PLANE_U  0
#define SFL_MEAN_PLANE_V  1
#define SFL_MEAN_PLANE_UU 2
#define SFL_MEAN_PLANE_VV 3
#define SFL_MEAN_PLANE_UV 4
#define SFL_MEAN_PLANE_P  5
#define SFL_MEAN_PLANE_PP 6
#define SFL_MEAN_PLANE_R  7
#define SFL_MEAN_PLANE_G  8
#define SFL_MEAN_PLANE_B  9
#define SFL_MEAN_PLANES   10
/* Start the averages of a whole-domain context: allocate the planes of `what` (1..15), zero them on the stream, and, for
 * every >= 1, add a sample behind every `every`-th step from now on.  A start while on begins anew from zero.              */
SFL_API int sfl_mean_start(sfl_context *ctx, int what, int every);
/* Drains the stream, frees the planes and takes the hook away.  Without averages on it does nothing.                       */
SFL_API int sfl_mean_stop(sfl_context *ctx);
/* Adds the fields held now as one more sample, asynchronously on the stream, whatever `every` is.                          */
SFL_API int sfl_mean_sample(sfl_context *ctx);
/* The mask, `every`, the samples added and the steps counted since the start; all zero without averages on.  Any pointer
 * may be NULL.                                                                                                             */
SFL_API int sfl_mean_info(sfl_context *ctx, int *what, int *every, int64_t *samples, int64_t *steps);
/* One plane (SFL_MEAN_PLANE_*) to the host, synchronously: dim_y x dim_x values of 8 bytes, densely packed, whatever the
 * padding on the device; float64, uint64 for the dye planes.  bytes must be exactly that.  Refused: a plane outside `what`,
 * another byte count, averages that are not on.                                                                            */
SFL_API int sfl_mean_download(sfl_context *ctx, int plane, void *host, size_t bytes);
/* The same for members [first, first + count) of a batch of either kind: the planes hold those members only.  A download
 * takes members [first_member, first_member + members), which must lie inside the recorded range: members x dim_y x dim_x
 * values, members in order.                                                                                                */
SFL_API int sfl_batch_mean_start(sfl_batch *b, int what, int every, int first, int count);
SFL_API int sfl_batch_mean_stop(sfl_batch *b);
SFL_API int sfl_batch_mean_sample(sfl_batch *b);
SFL_API int sfl_batch_mean_info(sfl_batch *b, int *what, int *every, int64_t *samples, int64_t *steps);
SFL_API int sfl_batch_mean_download(sfl_batch *b, int plane, int first_member, int members, void *host, size_t bytes);
/* --- TORQUE: how hard the flow TURNS solid bodies -- the moment about z of the pressure load of "LOADS" and of the skin
 *     friction of "FRICTION" on every body, about a pivot per body: as figures (sfl_batch_torque, sfl_torque) and as curves
 *     recorded while stepping (sfl_batch_torque_start, sfl_torque_start), without a download.  It is the pitching moment of a
 *     plate or a foil, with the loads the centre of pressure, and the torque that spins a disc.  The rule below is a definition
 *     stated here, like the loads' and the friction's: the reference knows no bodies.  ONE walk over the faces reads both
 *     fields.  The normal viscous stress has no part, as in "FRICTION"; the bodies are at rest.
 *   FACES, BODIES AND LABELS are those of "LOADS", word for word: a wet face is a pair (fluid cell F, solid cell S) where S is
 * one of F's four neighbours, S is INSIDE THE DOMAIN and S belongs to a body; the rim has no faces; labels and `bodies` come
 * from sfl_batch_set_bodies / sfl_set_bodies; a label counts only where the cell is solid at the time of the sample.
 *   AXES AND ARMS.  x grows with i (towards E) and y with j (towards N); the moment is about z, COUNTER-CLOCKWISE POSITIVE.  The
 * wall lies at node S, as in "FRICTION": both the pressure and the shear of a face ACT AT NODE S = (iS, jS).  A body's PIVOT
 * is given in HALF cell widths, int32_t pivot2[2]: the pivot is (pivot2[0] / 2, pivot2[1] / 2), so that the centre of a body
 * of even width is exact.  Every component satisfies |pivot2| <= SFL_TORQUE_MAX_PIVOT2 = 2^24.  Without pivots every pivot is
 * (0, 0).  The DOUBLED ARMS of a face are rx2 = 2 * iS - pivot2[0] and ry2 = 2 * jS - pivot2[1], in int32.
 *   PER BODY, FROM PASS 1 over its wet faces:
 *     max_abs_p   the load record's: the maximum of |p| over the finite pressures of the fluid cells of its faces;
 *     max_abs_t   the friction record's: the maximum over the finite tangential components (v.y for a fluid cell W or E of
 *                 its solid cell, v.x for one S or N of it);
 *     faces       the number of ALL of its wet faces, non-finite ones included;
 *     max_arm2    the maximum over its faces of max(|rx2|, |ry2|);
 *     s           with L(x) the bit length of x (0 for 0): s = max(0, L(faces) + L(max_arm2) - 30);
 *     exp2_p, exp2_f   q_p + s and q_f + s, where q_p and q_f are the exp2 of "LOADS" and of "FRICTION".
 *   A FACE'S TERMS.  tp = (int64_t)trunc(ldexp((double)p, -exp2_p)), and tf the same from the tangential component with exp2_f;
 * both satisfy |t| < 2^(33 - s).  A non-finite p (tangential component) takes that face out of mp (mf) and into nonfinite_p
 * (nonfinite_t); the other sum still takes it.
 *   THE SUMS, with dir as everywhere: the FLUID cell lies 0 = W, 1 = E, 2 = S, 3 = N of the solid one.
 *     mp (pressure)   adds -ry2 * tp for dir 0, +ry2 * tp for dir 1, +rx2 * tp for dir 2 and -rx2 * tp for dir 3;
 *     mf (friction)   adds +rx2 * tf for dir 0 and 1 (tf from v.y) and -ry2 * tf for dir 2 and 3 (tf from v.x).
 * These are rx * Fy - ry * Fx with the signs of fx and fy of the two existing records.
 *   NO OVERFLOW.  |arm| < 2^L(max_arm2) and |t| < 2^(33 - s), so a product is below 2^(33 - s + L(max_arm2)) and the sum of
 * `faces` < 2^L(faces) of them satisfies |sum| < 2^(33 - s + L(max_arm2) + L(faces)) <= 2^63: for s = 0 because then
 * L(faces) + L(max_arm2) <= 30, else because s makes up the difference exactly.  mp and mf never overflow.
 *   UNITS.  The pressure torque is mp * 2^(exp2_p - 1) in pressure x cell widths^2 (the arms are doubled); the caller
 * multiplies by dx^2.  The friction torque per unit depth is rho * nu * mf * 2^(exp2_f - 1) * dx.
 *   IDENTITY WITH THE EXISTING RECORDS.  For every real body s = 0 -- s > 0 needs L(faces) + L(max_arm2) > 30, more than 2^14
 * faces at arms beyond 2^16 half cells.  Then tp and tf ARE the terms of the load and of the friction record, and moving the
 * pivot by (a2, b2) half cells changes mp by exactly -(a2 * fy - b2 * fx) of the load record, and mf in the same way with the
 * friction record: the centre of pressure follows from the three records without a second sample.
 *   A body without a face reports all zeros, and so does every body while no solids are set; in both cases pivot2 is still
 * filled in.  Integer sums, maxima and counts do not depend on the order of reduction: every field of every record is, bit
 * for bit, what the rule computes from the downloaded pressure, velocity, mask, labels and pivots, and a context and a batch
 * member of the same shape, mask, labels, pivots and fields report the same bytes.
 *   THE TORQUE RECORDER follows the loads recorder's rules unchanged, with a buffer, a step count and samples of its own:
 * steps count across calls; sample s belongs to step (s + 1) * every; a step call without room for its samples is refused
 * WHOLE with SFL_ERR_STATE before anything is staged or launched, with a message that names the torque recorder; a restart
 * keeps the buffer; a batch's one-launch replay of a timeline and the fused seams of sfl_step_n are NOT cut (they only run
 * without solids, where a sample reads no field).  It is independent of the history, of the loads recorder and of the
 * friction recorder: any of the four may be on together, and behind a step the order is history, loads, friction, torque.
 * With no torque recorder on, every call launches exactly what it launched before there was one.  sfl_batch_set_bodies /
 * sfl_set_bodies are refused with SFL_ERR_STATE while the torque recorder is on, with a message of their own; a call of
 * theirs that changes the number of bodies puts every pivot back to (0, 0).
 *   Admission as everywhere: the argument checks and their order are those of the loads' calls, one for one; the state
 * refusals follow; a slab and a context with a transport attached are refused as from sfl_loads.                            */
#define SFL_TORQUE_MAX_PIVOT2 16777216
struct sfl_body_torque {
    int64_t  mp, mf;
    int32_t  exp2_p, exp2_f;
    float    max_abs_p, max_abs_t;
    uint32_t faces, max_arm2;
    uint32_t nonfinite_p, nonfinite_t;
    int32_t  pivot2[2];
    uint32_t reserved[2];
};                                     /* 64 bytes: offsets 0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56 */
/* The pivots: pivot2 = bodies pairs (x2, y2) shared by all members (per_member 0) or batch * bodies pairs, member-major
 * (per_member 1), the pair of body k of member m at pivot2[2 * (m * bodies + k - 1)]; read during the call only.  pivot2 NULL
 * goes back to (0, 0) for every body (bodies and per_member are then not looked at).  `bodies` must equal what
 * sfl_batch_bodies_info reports.  b NULL, per_member outside 0..1, another `bodies` and a component beyond
 * SFL_TORQUE_MAX_PIVOT2 (the message names the body) return SFL_ERR_INVALID.  Allowed while a recorder is on: the new pivots
 * hold from the next sample.  Batches of either kind.                                                                      */
SFL_API int sfl_batch_set_body_pivots(sfl_batch *b, const int32_t *pivot2, int per_member, int bodies);
/* The pivots of members [first, first + count), member-major (shared pivots: repeated; none set: zeros); bytes must be
 * count * bodies * 8.                                                                                                       */
SFL_API int sfl_batch_body_pivots_download(sfl_batch *b, int first, int count, int32_t *host, size_t bytes);
/* The torque records of members [first, first + count) from the pressure and the velocity held: count * bodies records,
 * member-major, as sfl_batch_loads; bytes must be count * bodies * 64.  One launch, synchronous; changes no field.  A batch
 * without solids set reports records that are zero but for pivot2, without a launch.                                        */
SFL_API int sfl_batch_torque(sfl_batch *b, int first, int count, struct sfl_body_torque *host, size_t bytes);
/* The torque recorder of a batch: the calls of the loads recorder, one for one (sfl_batch_loads_start, _stop, _info, _read). */
SFL_API int sfl_batch_torque_start(sfl_batch *b, int every, int first, int count, int capacity);
SFL_API int sfl_batch_torque_stop(sfl_batch *b);
SFL_API int sfl_batch_torque_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies);
SFL_API int sfl_batch_torque_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_torque *host, size_t bytes);
/* The same for a whole-domain context: `bodies` pairs, `bodies` records per sample.  A slab and a context with a transport
 * attached get SFL_ERR_STATE, as from sfl_loads.  A sample is two streaming passes over the code bytes, pass 1 and then the
 * sums, behind a memset of the sample's records, all on the context's stream.                                              */
SFL_API int sfl_set_body_pivots(sfl_context *ctx, const int32_t *pivot2, int bodies);
SFL_API int sfl_body_pivots_download(sfl_context *ctx, int32_t *host, size_t bytes);
SFL_API int sfl_torque(sfl_context *ctx, struct sfl_body_torque *host, size_t bytes);
SFL_API int sfl_torque_start(sfl_context *ctx, int every, int capacity);
SFL_API int sfl_torque_stop(sfl_context *ctx);
SFL_API int sfl_torque_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies);
SFL_API int sfl_torque_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_torque *host, size_t bytes);

/* --- WALL VELOCITIES: solid cells that move -- the lid of a cavity, a belt under a body, a spinning disc.  The geometry stays
 *     where it is; only what the wall cells HOLD changes.  Extends "SOLIDS" and "SOLIDS OF A CONTEXT" by calls of their own;
 *     with no table set every call launches exactly what it launched before.
 *   A WALL TABLE is a set of records (cell (i, j), velocity (u, v)), in grid units as every velocity here.  It extends the
 * solids' step by two statements and changes no other item:
 *     - ITEM 3, EXTENDED: after the forces, every solid cell holds (0, 0), except a solid cell named by a record: that cell
 *       holds the record's velocity, both components, bits as given -- a -0.0f or a denormal is stored as it stands.
 *     - ITEM 8, NEW, behind item 7: every solid cell named by a record holds its record's velocity again (item 6 has just
 *       zeroed it).
 *     - Items 4 to 7 are unchanged: the pressure sees an impermeable wall at rest, and a solid cell's dye is traced back with
 *       (0, 0).
 *   The wall acts on the flow through two things only: item 3a ("VISCOSITY"), whose sweeps read a solid neighbour as it is,
 * and item 1, whose samples interpolate the stored field, wall cells included.  A velocity component NORMAL to a wet face is
 * accepted and acts through those two items only: it drives nothing through the wall, which stays impermeable.  Consequence:
 * from rest and without viscosity a wall moves nothing; with nu > 0 a lid drags the row beside it.
 *     - A record must name a cell that is solid in the mask that is set -- in a batch with per-member masks, in the mask of
 *       every member the record applies to.  Otherwise the call returns SFL_ERR_INVALID and the message names the first
 *       offending record, and the member where there is one.  The velocity must be finite.
 *     - Of two records on one cell of one member the later wins.  The host removes the duplicates: the device sees unique
 *       cells in cell order, and the result does not depend on the order of execution.
 *     - A call replaces the table that was set; n == 0 clears it.  Every successful sfl_batch_set_solids / sfl_set_solids, a
 *       clear included, DROPS the table: it was checked against the mask that call replaced.  Nothing is staged again.
 *     - The table acts in step calls only: sfl_step, sfl_step_n, sfl_batch_step_n, sfl_batch_step_n_each.  Operators called on
 *       their own and sfl_diffuse_velocity are unchanged.
 *     - It works with and without viscosity and with and without openings and inflow profiles: walls are solid cells, inflow
 *       cells are fluid cells, and the two tables never meet.  Whatever the solids refuse stays refused.
 *     - THE RECORDS OF "FRICTION" AND "TORQUE" KEEP THEIR DEFINITION: the fluid's tangential velocity with the wall AT REST.
 *       No byte of them moves; the wall's share is the caller's to subtract from what the table says.
 *     - ANCHORS: a table whose velocities are all +0.0f gives the bits of no table; a context holds what a batch member of
 *       its shape holds; n steps of one call equal n calls of one step.
 *   A batch keeps the table as one CSR table on the device with a row per member (a shared table counts once per member),
 * staged once per call, never per step, and steps through kernels of its own, one launch per step.  A context keeps a compact
 * list; a step is the step that would have run with ONE launch over the list behind it (item 8: a thread per record), and,
 * where item 3a runs, ONE launch over the code bytes in front of the diffusion that stores (0, 0) or the record's velocity into
 * every solid cell.  Where item 3a does not run the extended item 3 cannot be observed and is not launched.
 *   Admission as everywhere.  A call's own argument checks come first, SFL_ERR_INVALID and answered on a machine without a GPU
 * where they need no handle: n < 0, NULL arrays with n > 0, a non-finite velocity (the message names the record), a NULL
 * handle, a member outside the batch.  The state refusal comes next: no solids set gives SFL_ERR_STATE -- so everything that
 * sfl_[batch_]set_solids refuses stays refused.  Then the records against the mask.  A refused call stages and launches
 * nothing and leaves the table as it was.                                                                                   */
/* Set the wall table of a context: record k is cell (cells_ij[2 k], cells_ij[2 k + 1]) with velocity (vel_xy[2 k],
 * vel_xy[2 k + 1]); both arrays are read during the call only.  n == 0 clears the table (the arrays may then be NULL).
 * Synchronous.                                                                                                             */
SFL_API int sfl_set_wall_velocity(sfl_context *ctx, const int *cells_ij, const float *vel_xy, int n);
/* The number of unique cells the table holds (0 without one).  Never waits.                                                */
SFL_API int sfl_wall_velocity_info(sfl_context *ctx, int *records);
/* The records held, in cell-index order (dim_x * j + i ascending); capacity counts records, and capacity < records returns
 * SFL_ERR_INVALID.  Never waits.                                                                                           */
SFL_API int sfl_wall_velocity_download(sfl_context *ctx, int *cells_ij, float *vel_xy, int capacity);
/* The same for a batch.  members NULL: every record goes to every member; else record k goes to member members[k] alone, and
 * a member that no record names has no moving wall.  Synchronous.                                                          */
SFL_API int sfl_batch_set_wall_velocity(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n);
/* set: a table is held; records: the unique cells over all members, a shared table counted once per member.  Never waits.  */
SFL_API int sfl_batch_wall_velocity_info(sfl_batch *b, int *set, int64_t *records);
/* The records of one member, in cell-index order; *records (may be NULL) receives their number whatever the capacity, and
 * capacity < that number returns SFL_ERR_INVALID -- except capacity 0 with both arrays NULL, which asks for the number alone and
 * succeeds.  Never waits.                                                                                                  */
SFL_API int sfl_batch_wall_velocity_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records);
/* A batch is used from one thread at a time, as a context is.                                    */
SFL_API int sfl_batch_synchronize(sfl_batch *b);

#ifdef __cplusplus
}
#endif
#endif /* SFL_H */
