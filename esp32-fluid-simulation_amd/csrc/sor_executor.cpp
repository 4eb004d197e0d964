// sor_executor.cpp -- poisson_solve (poisson.cpp:114-125) on a context: walks the launch / exchange program of
// slab_plan.h.  Three schedules for the halo exchanges of a slab (all the same bits):
//   in line            every launch whole, every exchange awaited (SFL_OPT_EXCHANGE_SCHEDULE = 1, the baseline kernel)
//   early, by events   the halo of a superstep travels one launch early on the exchange stream, its ghost rows are
//                      relaxed behind the message, the launch after waits for an event (SFL_OPT_EXCHANGE_SCHEDULE = 2)
//   in time, counted   the halo follows the launch that produces it; sender tiles count themselves, the message leaves
//                      on that count, only the next launch's cut-adjacent tiles wait -- inside the kernel -- for a
//                      count of arrivals (SFL_OPT_EXCHANGE_SCHEDULE = 3)
// (Round 4's fourth executor -- the launches of a solve as ONE chained launch -- bought -4 .. +3 % on the emulated ranks and was
// retired in round 6: DESIGN.md 6, history up to commit 77c9c76.)
// Host C++ only; the kernels live in sor_fused.hip / stencil_kernels.hip / small_grid.hip.
#include "transport.h"

namespace sfl {
namespace host {

// The folded interior relaxation (SFL_OPT_SOR_FOLD, sor_stream_core.h relax) multiplies by -0.25f * omega: that quarter must itself be
// exact, i.e. must not underflow -- an omega below 2^-124 is solved with both products whatever the option says.
static bool quarter_omega_is_exact(float omega) { return (-0.25f * omega) * -4.0f == omega; }

sfl::SorParams sor_params(const sfl_context *c, float dx, float omega)
{
    sfl::SorParams prm;
    prm.dx = dx;
    prm.omega = omega;
    prm.one_minus_omega = 1.0f - omega;  // (1 - omega) in float, poisson.cpp:98,111
    prm.neg_quarter_omega = -0.25f * omega;
    prm.fold = c->opt.sor_fold && quarter_omega_is_exact(omega) ? 1 : 0;
    return prm;
}

// Fuse depth: explicit option, or auto from the slab size.  Measured on MI355X, ms per 80-iteration
// solve at fuse 8 / 10 / 12 / 14 / 16 (round 2, gpurun_out/r02_run13-14, auto rows per tile):
// 8192 x 8192: 3.6 / 3.0 / 2.51 / 2.39 / 1.95; 8192 x 4096: - / - / 1.26 / 1.14 / 1.08; 8192 x 2048: - / 0.70 /
// 0.64 / 0.60 / 0.60; 8192 x 1024: 0.458 / 0.398 / 0.425 / 0.57 / 0.64; 8192 x 512 (round 1): 0.39 / - / 0.42 /
// - / 0.45; 40 iterations: 4096^2 - / 0.343 / 0.327 / 0.308 / 0.294; 3072^2 0.245 / 0.208 / 0.223 / 0.294 / 0.297; 2048^2
// 0.155 / 0.143 / 0.175 / - / 0.217; 1024^2 0.086 / 0.090 / 0.097; 8192 x 768 (80): 0.366 / 0.333 / 0.393; 8192 x 512: 0.303 /
// 0.305 / 0.350.  Big slabs are bound by the pass over memory
// each launch makes and want the deepest fusion; small ones by the 2 * NS warm-up rows each tile
// re-streams.  Every rank of a group sees the same thinnest slab, so all ranks resolve the same value.
int effective_fuse(const sfl_context *c)
{
    int f = c->opt.sor_fuse;
    if (f == 0) {
        const int64_t cells = (int64_t)min_owned_rows(c) * c->dim_x;
        f = cells >= 12000000 ? 16 : cells >= 3000000 ? 10 : 8;
    }
    if (f < 2) f = 2;
    if (f > SFL_MAX_FUSE) f = SFL_MAX_FUSE;
    return f & ~1;
}

int effective_kernel(const sfl_context *c) { return c->opt.sor_kernel == 1 ? 1 : 2; }

// One workgroup, fields in LDS (small_grid.hip): whole-domain contexts of at most kSmallGridMaxCells cells whose
// kernel options are all automatic (an explicit kernel / fuse / tile choice is honoured as given).
bool small_grid(const sfl_context *c)
{
    return c->opt.small_grid && c->nranks == 1 && !c->transport &&
           sfl::small_grid_fits(c->dim_x, c->gdim_y) && c->opt.sor_kernel == 0 &&
           c->opt.sor_fuse == 0 && c->opt.sor_rows == 0 && c->opt.sor_lane_cells == 0 && c->opt.advect_kernel == 0;
}


// What a solve of `iters` iterations costs a middle rank (a cut on both sides) of the thinnest slab with halo depth
// `halo`, in microseconds, by a model with ONE measured input -- the exchange (sfl_context::exchange_latency_us /
// exchange_ns_per_row, transport.cpp measure_exchange) -- and two constants of this kernel on this chip:
//   launch        3.5 us of dispatch, ramp-up and drain + 0.2 ps per cell and colour pass over the rows it streams: the
//                 owned rows plus, on each side, the ghost rows it still has to keep exact and its own warm-up
//                 (profiles/r04_thin_share_lower_bound.txt: 23.4 us per launch of 8192 x (1024 + 2 x 43) cells at 10 passes;
//                 profiles/r04_default_fuse16_summary.txt: 176 us per launch of 8192^2 at 16 passes);
//   exchange      what a message costs the critical path: its measured latency (cross-stream hand-over included) + its rows
//                 at the measured rate, all of it exposed when the launches are short (profiles/r04_wire_delay_curve.txt:
//                 0.95 D per exchange at 23 us launches), 0.6 of it when a launch lasts more than twice the message
//                 (0.62 D at 108 us launches).
// Only differences between depths matter: a deeper halo trades exchanges for redundantly relaxed ghost rows.
static double modelled_solve_us(const sfl_context *c, int iters, int fuse, int halo, bool in_time)
{
    const int nranks = c->nranks, mid = nranks > 2 ? 1 : 0;   // (a rank with a cut on both sides where the group has one)
    const std::vector<sfl_plan_step> prog = sfl::plan_poisson(c->gdim_y, nranks, mid, iters, fuse, in_time ? 3 : 2, halo, c->solve_tail);
    const double lat = c->exchange_latency_us, per_row = c->exchange_ns_per_row * 1e-3 * (c->dim_x / 8192.0);
    double us = 0.0, launch_us = 0.0;
    int launches = 0;
    for (const sfl_plan_step &st : prog)
        if (st.kind == SFL_STEP_SOR) {
            const double t = 3.5 + (double)(st.g_end - st.g_begin + 2 * st.nsweeps) * c->dim_x * st.nsweeps * 0.2e-6;
            us += t;
            launch_us += t;
            ++launches;
        }
    const double per_launch = launches ? launch_us / launches : 0.0;
    for (const sfl_plan_step &st : prog)
        if (st.kind == SFL_STEP_EXCHANGE) {
            const double msg = lat + st.rows * per_row;   // (measured on p: 4-byte rows; the right-hand side's are the same size)
            us += (per_launch > 2.0 * msg ? 0.6 : 1.0) * msg;
        }
    return us;
}

// Halo depth of a solve's supersteps.  An explicit SFL_OPT_SOR_HALO is taken as given.  Automatic: the depth rounds 2 - 4 settled
// on with self-copies as the transport (64 rows on slabs of >= 1024 rows: 2 - 3 exchanges per 80-iteration solve, ~5 % extra
// rows recomputed; 32 on thinner ones) is the starting point and the fallback; with RCCL's own kernels as the transport an
// exchange costs a solve 10 - 17 us more than a copy (profiles/r05_emulate_rccl.txt) and a real wire adds to that -- 8192^2 on
// 8 GPUs then does better with ONE p exchange per solve (80 rows) or none (160) than with two.  The model above names the
// candidates, timed solves decide (choose_halo).  Every rank of a group sees the same measurement (its maximum over the ranks)
// and the same thinnest slab, so all ranks name the same candidates.
static int clamp_halo(const sfl_context *c, int fuse, int h)
{
    const int thinnest = min_owned_rows(c);
    if (h > thinnest) h = thinnest;  // a neighbour can only send rows it owns
    if (h > kGhostRows) h = kGhostRows;
    return h < fuse ? fuse : h;
}

static int legacy_halo(const sfl_context *c, int fuse) { return clamp_halo(c, fuse, min_owned_rows(c) >= 1024 ? kLegacySorHalo : 32); }

// the depth the model likes best (the legacy depth when nothing has been measured)
static int modelled_best_halo(const sfl_context *c, int fuse, int iters, bool in_time)
{
    const int legacy = legacy_halo(c, fuse);
    if (c->exchange_latency_us < 0 || iters < 1 || c->nranks < 2) return legacy;
    int best = legacy;
    double best_us = modelled_solve_us(c, iters, fuse, legacy, in_time);
    for (int h : {32, 48, 64, 80, 96, 112, 128, 144, 160}) {
        if (clamp_halo(c, fuse, h) != h || h == legacy) continue;   // (depths the slab cannot carry)
        const double us = modelled_solve_us(c, iters, fuse, h, in_time);
        if (us < best_us) {
            best_us = us;
            best = h;
        }
    }
    return best;
}

// What effective_halo answers WITHOUT side effects: the option, a depth already decided for this kind of solve, else the
// legacy depth (plans queried from outside, the model's own plans).
int effective_halo(const sfl_context *c, int fuse, int iters, bool in_time)
{
    if (c->opt.sor_halo) return clamp_halo(c, fuse, c->opt.sor_halo);
    const HaloTuner &t = c->group ? c->group->halo_tuner : c->halo_tuner;
    const HaloTuner::Kind kind{iters, fuse, c->solve_tail, in_time ? 1 : 0};
    for (const HaloTuner::Decided &d : t.decided)
        if (d.kind == kind) return d.halo;
    return legacy_halo(c, fuse);
}

// Halo depth of THIS solve (see HaloTuner).  Candidates: the legacy depth, the model's favourite, the deepest the slab can
// carry.  Until the kind is decided, solve after solve runs on the candidates in turn, each between its own pair of events on
// the compute stream; nothing is read back meanwhile (the solves are queued as they are in steady state); the thirteenth solve
// of the kind waits for the twelfth, reads the pairs and decides.  RCCL ranks decide on the maximum over the ranks -- a
// collective at that solve, which every rank reaches in step (the ranks of a communicator issue the same calls).  An
// explicit SFL_OPT_SOR_HALO switches all of this off.
static int choose_halo(sfl_context *ctx, int fuse, int iters, bool in_time, int *timed_solve)
{
    *timed_solve = -1;
    HaloTuner &t = ctx->group ? ctx->group->halo_tuner : ctx->halo_tuner;
    if (ctx->opt.sor_halo || !ctx->transport || ctx->nranks < 2 || iters < 1 || ctx->exchange_latency_us < 0) {
        t.active = false;
        return effective_halo(ctx, fuse, iters, in_time);
    }
    const HaloTuner::Kind kind{iters, fuse, ctx->solve_tail, in_time ? 1 : 0};
    for (const HaloTuner::Decided &d : t.decided)
        if (d.kind == kind) return d.halo;
    if (!t.active || !(t.kind == kind)) {   // a new kind of solve: name the candidates
        t.active = true;
        t.kind = kind;
        t.ncand = 0;
        for (int h : {legacy_halo(ctx, fuse), modelled_best_halo(ctx, fuse, iters, in_time), clamp_halo(ctx, fuse, kGhostRows)}) {
            bool seen = false;
            for (int k = 0; k < t.ncand; ++k) seen = seen || t.cand[k] == h;
            if (!seen) t.cand[t.ncand++] = h;
        }
        t.solve_no = 0;
    }
    if (t.ncand > 1 && t.solve_no < t.ncand * HaloTuner::kSolvesEach) {
        // the candidates take turns, round after round, every second round in reverse order: the first solves after a pause run
        // at clocks that are still climbing (2.7 -> 1.9 ms over the first 15 solves of 8192^2), and a candidate measured as a
        // block would be judged by WHEN it ran (C5 with self-copies: the deepest halo, timed last, was chosen 3.5 % too slow)
        const int round = t.solve_no / t.ncand, pos = t.solve_no % t.ncand;
        const int k = (round & 1) ? t.ncand - 1 - pos : pos;
        t.which[t.solve_no] = k;
        *timed_solve = t.solve_no++;
        return t.cand[k];
    }
    // decide: the FASTEST timed solve of each candidate (a stall of the host or a clock step hits one solve, not three; the
    // first round is every depth's warm-up), the maximum over the ranks where they are separate processes
    int us[HaloTuner::kCandidates] = {0, 0, 0};
    for (int k = 1; k < HaloTuner::kCandidates; ++k) us[k] = 1 << 30;
    if (t.ncand > 1) {
        us[0] = 1 << 30;
        const int last = t.solve_no - 1;
        const bool done = t.ev[2 * last + 1] && hipEventSynchronize(t.ev[2 * last + 1]) == hipSuccess;
        for (int n = t.ncand; done && n <= last; ++n) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, t.ev[2 * n], t.ev[2 * n + 1]) == hipSuccess && ms > 0.0f && ms < 1e5f)
                us[t.which[n]] = std::min(us[t.which[n]], (int)(ms * 1e3f + 0.5f));
        }
        if (us[0] == 1 << 30) us[0] = 0;   // (nothing usable: the legacy depth)
    }
    if (t.ncand > 1 && reduces_on_device(ctx)) {
        // (the context's own scratch words: no allocation that could fail on one rank and leave the others in the reduction alone)
        int *dev = ctx->d_collective;
        Overlap o;
        static_assert(HaloTuner::kCandidates <= kCollectiveWords, "scratch words of the ranks' reductions");
        if (hipMemcpy(dev, us, sizeof us, hipMemcpyHostToDevice) != hipSuccess) (void)hipMemset(dev, 0x7f, sizeof us);
        const bool ok = overlap_of(ctx, &o) == SFL_OK && ctx->transport->allreduce_max(ctx, dev, HaloTuner::kCandidates, o.xstream) == SFL_OK &&
                        hipStreamSynchronize(o.xstream) == hipSuccess && hipMemcpy(us, dev, sizeof us, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok)
            for (int k = 1; k < t.ncand; ++k) us[k] = 1 << 30;   // (then the legacy depth, on every rank that got this far)
    }
    int best = 0;
    for (int k = 1; k < t.ncand; ++k)
        if (us[k] < us[best] && (long)us[k] * 1000 < (long)us[0] * 985) best = k;   // (another depth has to beat the legacy one by 1.5 %: box noise)
    if (getenv("SFL_TUNER_LOG"))   // (what the choice was made from, for whoever wants to see it)
        fprintf(stderr, "sfl halo tuner: slab %d/%d iters %d fuse %d tail %d %s: exchange %d us + %d ns/row; candidates %d / %d / %d rows: "
                "%d / %d / %d us per solve -> %d rows\n", ctx->rank, ctx->nranks, iters, fuse, ctx->solve_tail, in_time ? "in time" : "by events",
                ctx->exchange_latency_us, ctx->exchange_ns_per_row, t.cand[0], t.ncand > 1 ? t.cand[1] : 0, t.ncand > 2 ? t.cand[2] : 0,
                us[0], t.ncand > 1 ? us[1] : 0, t.ncand > 2 ? us[2] : 0, t.cand[best]);
    t.decided.push_back(HaloTuner::Decided{kind, t.cand[best]});
    t.active = false;
    return t.cand[best];
}

// Exchanges IN TIME with everything counted on the device (run_poisson_in_time; SFL_OPT_EXCHANGE_SCHEDULE = 3) instead of early exchanges
// behind cross-stream events: slabs with a transport, the fused kernel, exchanges overlapped -- where the transport takes it by
// default (Transport::arrival_by_default) or the option asks for it, and only where the compute and the exchange stream were
// seen to run side by side (resolve_schedule: a launch that waits inside the kernel must not sit in front of its message).
bool in_time_exchanges(const sfl_context *c)
{
    if (!c->transport || !c->opt.sor_overlap || c->nranks < 2 || c->opt.sor_kernel == 1) return false;
    const int asked = c->opt.sor_arrival >= 0 ? c->opt.sor_arrival : (c->transport->arrival_by_default() ? 1 : 0);
    const int side_by_side = c->group ? c->group->streams_concurrent : c->streams_concurrent;
    return asked && side_by_side == 1;
}

// The one thing in_time_exchanges cannot find out as a const query: do the two streams run side by side?  Measured once
// (transport.cpp streams_run_concurrently); ranks of a communicator measured it at attach and agreed on the result.
int resolve_schedule(sfl_context *ctx)
{
    if (!ctx->transport || ctx->nranks < 2) return SFL_OK;
    bool yes = false;
    SFL_TRY(streams_run_concurrently(ctx, &yes));
    // what an exchange costs (the automatic halo depth is chosen from it): RCCL ranks measured it, collectively, at
    // attach; ranks that share this host thread do it here, once, when no halo depth was asked for; and everybody again
    // after an option changed the protocol it was measured with
    if (ctx->exchange_latency_us < 0 && ctx->opt.sor_halo == 0 && ctx->opt.sor_kernel != 1)
        SFL_TRY(measure_exchange(ctx));   // (RCCL ranks get here together: each of them changed the option that invalidated it)
    return SFL_OK;
}

int halo_timeout_us(const sfl_context *c)
{
    if (c->opt.halo_timeout_ms > 0) return c->opt.halo_timeout_ms > 2000000 ? 2000000000 : c->opt.halo_timeout_ms * 1000;
    return c->transport ? c->transport->default_timeout_us() : 2000000;
}

// ---- poisson_solve executor --------------------------------------------------------------
// One SOR launch of a plan step over output rows [g_begin, g_end) (a step may be issued in pieces:
// all pieces read c->p and write c->p_alt; the caller swaps once per step).  `on` = stream (null: the compute stream)
int launch_sor_rows(sfl_context *c, const sfl_plan_step &st, const sfl::SorParams &prm, int g_begin, int g_end,
                    int g2_begin = 0, int g2_end = 0, hipStream_t on = nullptr, const sfl::HaloWait *wait = nullptr,
                    int *senders = nullptr)
{
    if (senders) *senders = 0;
    if (g_end <= g_begin && g2_end <= g2_begin) return SFL_OK;
    const float *in = c->p;
    float *out = c->p_alt;
    SFL_TRY(use_device(c));
    // Slabs that outgrow the Infinity Cache (256 MB; p + d of 48 M cells = 384 MB) reverse the stream direction of
    // every tile from one launch to the next: a launch then begins on the rows its predecessor read and wrote
    // last, the only ones still cached (8192^2: -3 % per launch; no gain or a small loss on slabs that fit:
    // profiles/r03_alternate_sweep.txt).  last_launches counts the plan steps issued so far in this solve.
    const int sweep = c->local_cells() >= kAlternateSweepCells ? c->last_launches : 0;
    HIP_TRY(sfl::launch_sor_fused(on ? on : c->stream, out, st.from_zero ? nullptr : in, c->div, c->geom,
                                  sfl::SorRows{g_begin, g_end, g2_begin, g2_end}, st.nsweeps, st.first_colour,
                                  prm, c->opt.sor_rows, sweep, wait, senders));
    return SFL_OK;
}

// Device-side halo arrival (run_poisson_in_time, kernels.h HaloWait).  The exchange stream counts a context's arrived
// messages in a device word; the next launch on the compute stream is queued WITHOUT a cross-stream event and lets only
// its cut-adjacent tiles wait for the count.
sfl::HaloWait arrival_wait(const sfl_context *c)
{
    sfl::HaloWait w;
    w.flag = c->d_arrival;
    w.timed_out = c->d_arrival + 1;
    w.epoch = c->arrival_epoch;
    w.own_lo = c->rank > 0 ? c->g0 : -(1 << 30);                 // no cut on that side: nothing to wait for
    w.own_hi = c->rank < c->nranks - 1 ? c->g1 : (1 << 30);
    w.done = nullptr;
    w.send_lo_end = w.send_hi_begin = 0;
    w.timeout_us = halo_timeout_us(c);
    w.system_scope = c->transport && c->transport->separate_processes();   // the halo rows were written by another GPU
    return w;
}

int exec_sor_step(sfl_context *c, const sfl_plan_step &st, const sfl::SorParams &prm)
{
    SFL_TRY(use_device(c));
    if (st.kind == SFL_STEP_ZERO) {
        HIP_TRY(sfl::launch_zero_rows(c->stream, c->p, c->geom, clip_lo(c, c->geom.grow0),
                                      clip_hi(c, c->geom.grow0 + c->geom.lrows)));
        ++c->last_launches;
        return SFL_OK;
    }
    if (st.nsweeps == 1) {
        HIP_TRY(sfl::launch_sor_half_sweep(c->stream, c->p, c->div, c->geom, st.g_begin, st.g_end,
                                           st.first_colour, prm));
        ++c->last_launches;
        return SFL_OK;
    }
    SFL_TRY(launch_sor_rows(c, st, prm, st.g_begin, st.g_end));
    std::swap(c->p, c->p_alt);
    ++c->last_launches;  // plan steps, not pieces: an overlapped step counts once as well
    return SFL_OK;
}

// Exchanges IN TIME (slab_plan.cpp kernel 3; SFL_OPT_EXCHANGE_SCHEDULE = 3): the halo of a superstep is sent after the launch that
// produces it, as in the textbook -- but nothing waits for a whole launch any more.  The launch in front of an exchange
// marks the tiles whose rows the message carries as SENDERS (top priority; each counts itself once its rows are written
// back); the exchange stream waits for that count, not for the launch, so the message leaves while the rest of the launch
// is still running; the launch behind the exchange is queued at once and only its cut-adjacent tiles wait for the arrival
// count.  No event on the compute stream, no ghost launch, no launch split.  (The right-hand side at the head of a solve
// was produced by other kernels: its exchange still starts behind an event.)
int run_poisson_in_time(sfl_context *ctx, const std::vector<sfl_context *> &peers,
                        const std::vector<std::vector<sfl_plan_step>> &progs, const sfl::SorParams &prm, const Overlap &o)
{
    bool flagged = false;   // the next launch's cut-adjacent tiles wait for the arrival count
    const size_t n = progs[0].size();
    for (size_t i = 0; i < n; ++i) {
        const sfl_plan_step &st0 = progs[0][i];
        if (st0.kind == SFL_STEP_EXCHANGE) {   // the right-hand side (a p exchange is taken together with the launch before it)
            SFL_TRY(start_exchange(peers, o, st0.field, st0.rows, st0.g_begin, false, true));
            flagged = true;
            continue;
        }
        const bool sends = i + 1 < n && progs[0][i + 1].kind == SFL_STEP_EXCHANGE && progs[0][i + 1].field == SFL_FIELD_PRESSURE;
        for (size_t k = 0; k < peers.size(); ++k) {
            sfl_context *c = peers[k];
            const sfl_plan_step &st = progs[k][i];
            sfl::HaloWait w = arrival_wait(c);
            if (!flagged) w.flag = nullptr;
            if (sends) {
                const sfl_plan_step &x = progs[k][i + 1];
                w.done = c->d_done;
                w.send_lo_end = c->rank > 0 ? c->g0 + x.g_begin + x.rows : -(1 << 30);
                w.send_hi_begin = c->rank < c->nranks - 1 ? c->g1 - x.g_begin - x.rows : (1 << 30);
            }
            int senders = 0;
            SFL_TRY(launch_sor_rows(c, st, prm, st.g_begin, st.g_end, 0, 0, nullptr,
                                    (flagged || sends) ? &w : nullptr, &senders));
            c->done_target += senders;
            std::swap(c->p, c->p_alt);
            ++c->last_launches;
        }
        flagged = false;
        if (sends) {
            const sfl_plan_step &x = progs[0][i + 1];
            SFL_TRY(exchange(peers, SFL_FIELD_PRESSURE, x.rows, o.xstream, x.g_begin, true, true));
            flagged = true;
            ++i;   // the exchange step has been issued
        }
    }
    return SFL_OK;
}

// EARLY exchanges behind cross-stream events (slab_plan.cpp kernel 2 with halo >= 2 x fuse: every automatic
// configuration; SFL_OPT_EXCHANGE_SCHEDULE = 2, and the default of a transport whose peers are other processes).  The ghost rows
// are still valid as deep as the next launch needs for the OWNED rows when the halo of the following superstep is sent:
//   compute stream    that launch, owned rows only, whole -- no piece of it waits for the wire;
//   exchange stream   the message (rows beyond that depth), then the same launch's passes on the ghost rows it feeds
//                     (output rows [g_begin, g0) and [g1, g_end)).  Both read p and write p_alt, on disjoint rows; the
//                     message lands in rows of p that the owned-row launch reads only into its throw-away rim;
//   the launch AFTER  waits for `arrived` -- WHOLE: it overwrites the owned rows this rank's own outgoing message is
//                     still being read from (round 4 let only its cut-adjacent tiles wait, on a device-side count: one
//                     solve in 26 000 came out wrong, profiles/r04_exchanges_counted_on_the_device.txt).
// Every other exchange of the program (the right-hand side at the head of a solve; p at halo < 2 x fuse) is awaited in
// line: round 2's split launches around them (cut-adjacent rows first / last) are gone -- one more executor that had to
// stay bit-exact for 16 us per solve.  The same bits as the in-line order.
int run_poisson_early(sfl_context *ctx, const std::vector<sfl_context *> &peers,
                      const std::vector<std::vector<sfl_plan_step>> &progs, const sfl::SorParams &prm, const Overlap &o)
{
    bool pending = false;  // an early exchange is in flight, with the ghost rows relaxed behind it: the next launch needs all of it
    const size_t n = progs[0].size();
    for (size_t i = 0; i < n; ++i) {
        const sfl_plan_step &st0 = progs[0][i];
        if (pending) {
            SFL_TRY(await_exchange(peers, o));
            pending = false;
        }
        if (st0.kind == SFL_STEP_EXCHANGE && st0.field == SFL_FIELD_PRESSURE && st0.g_begin > 0 && i + 1 < n &&
            progs[0][i + 1].kind == SFL_STEP_SOR && progs[0][i + 1].nsweeps <= st0.g_begin) {
            SFL_TRY(start_exchange(peers, o, SFL_FIELD_PRESSURE, st0.rows, st0.g_begin, false));
            for (size_t k = 0; k < peers.size(); ++k) {
                sfl_context *c = peers[k];
                const sfl_plan_step &st = progs[k][i + 1];
                const int lo = c->rank > 0 ? c->g0 : st.g_begin;
                const int hi = c->rank < c->nranks - 1 ? c->g1 : st.g_end;
                SFL_TRY(launch_sor_rows(c, st, prm, lo, hi));                                      // compute stream
                SFL_TRY(launch_sor_rows(c, st, prm, st.g_begin, lo, hi, st.g_end, o.xstream));     // behind the message
            }
            SFL_TRY(mark_arrived(peers, o));
            for (sfl_context *c : peers) {
                std::swap(c->p, c->p_alt);
                ++c->last_launches;
            }
            pending = true;
            ++i;  // the launch has been issued
            continue;
        }
        if (st0.kind == SFL_STEP_EXCHANGE) {
            SFL_TRY(start_exchange(peers, o, st0.field, st0.rows, st0.g_begin));
            SFL_TRY(await_exchange(peers, o));
            continue;
        }
        for (size_t k = 0; k < peers.size(); ++k) SFL_TRY(exec_sor_step(peers[k], progs[k][i], prm));
    }
    if (pending) SFL_TRY(await_exchange(peers, o));
    return SFL_OK;
}

int run_poisson_overlapped(sfl_context *ctx, const std::vector<sfl_context *> &peers,
                           const std::vector<std::vector<sfl_plan_step>> &progs, const sfl::SorParams &prm)
{
    Overlap o;
    SFL_TRY(overlap_of(ctx, &o));
    const int rc = in_time_exchanges(ctx) ? run_poisson_in_time(ctx, peers, progs, prm, o)
                                          : run_poisson_early(ctx, peers, progs, prm, o);
    if (rc != SFL_OK) {
        // a launch or an RCCL call failed half way: nothing of this solve may still be in flight on the exchange
        // stream when the caller looks at (or destroys) the context; the error message of the failure is kept
        const std::string why = last_error();
        (void)hipStreamSynchronize(o.xstream);
        (void)hipStreamSynchronize(o.compute);
        last_error() = why;
    }
    return rc;
}

// warm (whole-domain contexts on the general kernels; solve_until.cpp: sfl_poisson_continue, the segments of run_poisson_until): the program of a solve of `iters`
// iterations with its FIRST launch reading the pressure the context holds instead of taking it as zero, and without the
// baseline kernel's zero fill.  Everything else is the same walk, so the result does not depend on the fuse depth either.
int run_poisson(sfl_context *ctx, float dx, int iters, float omega, bool warm)
{
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    if (warm && ctx->nranks > 1)   // (a slab's plan sends no halo for its first superstep: p is zero there)
        return fail(SFL_ERR_STATE, "a solve continues from the pressure it holds on whole-domain contexts only (slab %d/%d)",
                    ctx->rank, ctx->nranks);

    std::vector<sfl_context *> peers = peers_of(ctx);
    SFL_TRY(resolve_schedule(ctx));
    const int fuse = effective_fuse(ctx), kernel = effective_kernel(ctx);
    const bool in_time = in_time_exchanges(ctx);
    int timed_solve = -1;   // >= 0: an exploratory solve of the halo tuner, between its pair of events
    const int halo = kernel == 2 && !small_grid(ctx) ? choose_halo(ctx, fuse, iters, in_time, &timed_solve) : effective_halo(ctx, fuse, iters, in_time);
    HaloTuner &tuner = ctx->group ? ctx->group->halo_tuner : ctx->halo_tuner;
    if (timed_solve >= 0) {
        SFL_TRY(use_device(ctx));
        for (int k = 0; k < 2; ++k)
            if (!tuner.ev[2 * timed_solve + k]) HIP_TRY(hipEventCreate(&tuner.ev[2 * timed_solve + k]));
        HIP_TRY(hipEventRecord(tuner.ev[2 * timed_solve], ctx->stream));
    }
    std::vector<std::vector<sfl_plan_step>> progs;
    for (sfl_context *c : peers) {
        SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
        SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
        progs.push_back(sfl::plan_poisson(c->gdim_y, c->nranks, c->rank, iters, fuse, kernel == 2 && in_time ? 3 : kernel, halo,
                                          ctx->solve_tail));
        c->last_halo = kernel == 2 && c->nranks > 1 ? halo : 0;
        c->last_launches = c->last_exchanges = 0;
        c->p_ghost_valid = 0;
        c->last_fuse = kernel == 1 ? 1 : fuse;
    }
    if (warm)
        for (std::vector<sfl_plan_step> &prog : progs) {
            if (!prog.empty() && prog.front().kind == SFL_STEP_ZERO) prog.erase(prog.begin());
            for (sfl_plan_step &st : prog)
                if (st.kind == SFL_STEP_SOR) {
                    st.from_zero = 0;
                    break;
                }
        }
    const sfl::SorParams prm = sor_params(ctx, dx, omega);
    if (warm && iters == 0) return SFL_OK;   // the pressure stays as it is
    if (small_grid(ctx)) {  // one workgroup, p and d in LDS, every iteration in one launch
        SFL_TRY(use_device(ctx));
        if (warm)   // (solve_until.cpp launches the one-workgroup kernel that starts from a pressure itself)
            return fail(SFL_ERR_STATE, "the warm walk is the general kernels': a small grid continues in its own launch");
        HIP_TRY(sfl::launch_small_solve(ctx->stream, ctx->p, ctx->div, ctx->dim_x, ctx->gdim_y, iters, prm));
        ctx->last_launches = 1;
        ctx->last_fuse = 2 * iters;
        return SFL_OK;
    }
    if (iters == 0) {  // the reference still zero-fills p (poisson.cpp:117-119)
        for (sfl_context *c : peers) {
            SFL_TRY(use_device(c));
            HIP_TRY(sfl::launch_zero_rows(c->stream, c->p, c->geom, c->g0, c->g1));
        }
        return SFL_OK;
    }
    if (kernel == 2 && ctx->nranks > 1 && ctx->opt.sor_overlap && ctx->transport) {
        SFL_TRY(run_poisson_overlapped(ctx, peers, progs, prm));
    } else {
        for (size_t i = 0; i < progs[0].size(); ++i) {
            const sfl_plan_step &st0 = progs[0][i];
            if (st0.kind == SFL_STEP_EXCHANGE) {
                SFL_TRY(exchange_inline(ctx, peers, st0.field, st0.rows, st0.g_begin));
            } else {
                for (size_t k = 0; k < peers.size(); ++k) SFL_TRY(exec_sor_step(peers[k], progs[k][i], prm));
            }
        }
    }
    // ghost rows of p the last launch left exact (the plan's tail): what subtract_gradient may read without an exchange
    int tail = ctx->nranks > 1 ? ctx->solve_tail : 0;
    for (size_t k = 0; k < peers.size() && tail > 0; ++k) {
        const sfl_context *c = peers[k];
        const sfl_plan_step &last = progs[k].back();
        if (last.kind != SFL_STEP_SOR) tail = 0;
        if (c->rank > 0) tail = std::min(tail, c->g0 - last.g_begin);
        if (c->rank < c->nranks - 1) tail = std::min(tail, last.g_end - c->g1);
    }
    for (sfl_context *c : peers) c->p_ghost_valid = tail > 0 ? tail : 0;
    if (timed_solve >= 0) {
        SFL_TRY(use_device(ctx));
        HIP_TRY(hipEventRecord(tuner.ev[2 * timed_solve + 1], ctx->stream));
    }
    return SFL_OK;
}

}  // namespace host
}  // namespace sfl
