// sor_probe.h -- what tools/sor_clock_probe.hip adds to the product's fused SOR kernel: a backend that can leave parts of the
// work out, and a kernel that records per-wave clocks around the product's relax_tile.  Included AFTER csrc/sor_fused.hip (as
// text, so that file's anonymous namespace is open to this one).  Nothing here is ever part of the library.
//
// Build-time switches (-D..., all default 0; every one of them computes WRONG results -- they answer "what does this part cost"):
//   SFL_PROBE_NO_LDS       no rhs ring traffic
//   SFL_PROBE_NO_LOAD      no global loads
//   SFL_PROBE_P_LOAD_AUX   cache-policy bits of the 8-byte p loads  (16 = sc1: agent scope, bypasses L1)
//   SFL_PROBE_P_STORE_AUX  ... of the 8-byte p stores               (16 = sc1: written through the XCD's L2)
//   SFL_PROBE_NO_STORE     the finished rows are not stored (profiles/r06_pressure_never_stored.txt)
//   SFL_PROBE_SHIFT        1 = no lane shift at all, 2 = row_shr / row_shl instead of the full-wave shifts
//   SFL_PROBE_NO_EDGE      every tile takes the interior path (wrong at the walls)
// With none set, ProbeLane2 adds nothing to Lane2 and the probe kernel runs the product's instructions between its clock reads.
#pragma once

#ifndef SFL_PROBE_NO_LDS
#define SFL_PROBE_NO_LDS 0
#endif
#ifndef SFL_PROBE_NO_LOAD
#define SFL_PROBE_NO_LOAD 0
#endif
#ifndef SFL_PROBE_P_LOAD_AUX
#define SFL_PROBE_P_LOAD_AUX 0
#endif
#ifndef SFL_PROBE_P_STORE_AUX
#define SFL_PROBE_P_STORE_AUX 0
#endif
#ifndef SFL_PROBE_NO_STORE
#define SFL_PROBE_NO_STORE 0
#endif
#ifndef SFL_PROBE_SHIFT
#define SFL_PROBE_SHIFT 0
#endif
#ifndef SFL_PROBE_NO_EDGE
#define SFL_PROBE_NO_EDGE 0
#endif

namespace sfl {
namespace {

// Lane2 with the switched-off parts hidden.  sor::stream_tile calls every backend function through the backend's own type, so
// hiding a name is enough; each replacement is compiled only when its switch is set.
template <int NS, bool VEC, bool ZERO_IN, int ST = 0, bool FOLD = false>
struct ProbeLane2 : Lane2<NS, VEC, ZERO_IN, ST, FOLD> {
    using Base = Lane2<NS, VEC, ZERO_IN, ST, FOLD>;
    using V = typename Base::V;

    __device__ __forceinline__ sor::EdgeCell<ProbeLane2> edge_cell(int lane, int x0, int which) const
    {
        const sor::EdgeCell<Base> ec = Base::edge_cell(lane, x0, which);
        return {ec.in, ec.k_full, ec.k_part, ec.z_full};
    }
#if SFL_PROBE_SHIFT == 1
    __device__ __forceinline__ V from_lower_lane(V x) const { return x; }
    __device__ __forceinline__ V from_upper_lane(V x) const { return x; }
#elif SFL_PROBE_SHIFT == 2
    __device__ __forceinline__ V from_lower_lane(V x) const
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x111, 0xf, 0xf, false));
    }
    __device__ __forceinline__ V from_upper_lane(V x) const
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x101, 0xf, 0xf, false));
    }
#endif
#if SFL_PROBE_NO_LOAD
    __device__ __forceinline__ void load_row(int r, V &pa, V &pb, V &da, V &db) const
    {
        asm volatile("" : "+v"(pa), "+v"(pb), "+v"(da), "+v"(db));
    }
#elif SFL_PROBE_P_LOAD_AUX
    __device__ __forceinline__ void load_row(int r, V &pa, V &pb, V &da, V &db) const
    {
        if (!VEC || ZERO_IN) return Base::load_row(r, pa, pb, da, db);
        // Lane2::load_row's 8-byte path, the policy bits on the p load
        const int soff = this->load_row_bytes(r);
        const v2f f = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(this->rs_d, this->off_a, soff, 0));
        da = f.x;
        db = f.y;
        const v2f q = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(this->rs_p, this->off_a, soff, SFL_PROBE_P_LOAD_AUX));
        pa = q.x;
        pb = q.y;
    }
#endif
#if SFL_PROBE_NO_STORE
    __device__ __forceinline__ void store_row(int r, V a, V b) const
    {
        asm volatile("" ::"v"(a), "v"(b));   // the values stay "used": the relaxations are not optimised away
    }
#elif SFL_PROBE_P_STORE_AUX
    __device__ __forceinline__ void store_row(int r, V a, V b) const
    {
        if (!VEC) return Base::store_row(r, a, b);
        if (this->a_out) {   // Lane2::store_row's 8-byte path with other policy bits
            v2f o;
            o.x = a;
            o.y = b;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, o), this->rs_out, this->off_out, this->row_bytes(r), SFL_PROBE_P_STORE_AUX);
        }
    }
#endif
#if SFL_PROBE_NO_LDS
    __device__ __forceinline__ void ring_store(int slot, int plane, V x) const {}
    __device__ __forceinline__ V ring_load(int slot, int plane) const
    {
        V r = __builtin_bit_cast(float, this->off_out);
        asm volatile("" : "+v"(r));
        return r;
    }
#endif
};

// Every wave records when it started and ended on the shader clock (s_memtime) AND on the constant 100 MHz real-time clock
// (s_memrealtime), plus where it ran -- 6 words per tile, at g_sor_trace (a global, not a kernel argument: an argument would sit
// in two SGPRs for the wave's whole life, in a kernel that already spills them).
__device__ unsigned long long *g_sor_trace;
struct WaveTrace {
    unsigned long long t0, w0;
    unsigned hwid, xcc;
    __device__ __forceinline__ void begin()
    {
        t0 = __builtin_readcyclecounter();
        w0 = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    }
    __device__ __forceinline__ void end(int tile, int kind) const
    {
        const unsigned long long t1 = __builtin_readcyclecounter(), w1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0 && g_sor_trace) {
            unsigned long long *o = g_sor_trace + 6 * (size_t)tile;
            o[0] = t0; o[1] = t1; o[2] = w0; o[3] = w1; o[4] = hwid; o[5] = ((unsigned long long)kind << 32) | xcc;
        }
    }
};

#if SFL_PROBE_NO_EDGE
// relax_tile without its boundary branch: MIRRORS sor_fused.hip relax_tile (the backend's construction and the two interior
// branches), keep in step with it.
template <class B, int NS, bool DX1, bool ZERO_IN>
__device__ __forceinline__ int probe_relax_tile(float *p_out, const float *p_in, const float *d, const Slab &g, const sor::Tiling &t,
                                                const sor::TileRect &rect, const SorParams &prm, float *ring_base, int lane)
{
    const size_t bytes = (size_t)g.lrows * (size_t)g.dim_x * 4;
    const unsigned records = bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)bytes;
    auto backend = [&](int row_sign) {   // (row_sign a constant in each branch, as in relax_tile)
        B bk;
        bk.rs_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ZERO_IN ? d : p_in), 0, records, 0x00020000);
        bk.rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(d), 0, records, 0x00020000);
        bk.rs_out = __builtin_amdgcn_make_buffer_rsrc(p_out, 0, records, 0x00020000);
        bk.dim_x = g.dim_x;
        bk.gdim_y = g.gdim_y;
        bk.grow0 = g.grow0;
        bk.row_lo = max(g.grow0, 0);
        bk.row_hi = min(g.grow0 + g.lrows, g.gdim_y);
        bk.row_sign = row_sign;
        bk.prio_on = t.rotate;
        bk.start_turns();
        bk.setup(ring_base, lane, sor::strip_x0(t, rect.strip), t.halo_cols);
        return bk;
    };
    const sor::EdgeCell<B> none{};
    if (sor::tile_may_flip(t, rect)) {
        B bk = backend(-1);
        sor::Consts<B> c{bk.splat(prm.dx), bk.splat(prm.omega), bk.splat(prm.one_minus_omega), bk.splat(prm.neg_quarter_omega)};
        sor::stream_tile<B, NS, false, DX1, ZERO_IN, true>(bk, c, none, none, 1 - rect.r1, 1 - rect.r0);
        return 2;
    }
    B bk = backend(1);
    sor::Consts<B> c{bk.splat(prm.dx), bk.splat(prm.omega), bk.splat(prm.one_minus_omega), bk.splat(prm.neg_quarter_omega)};
    sor::stream_tile<B, NS, false, DX1, ZERO_IN>(bk, c, none, none, rect.r0, rect.r1);
    return 0;
}
#endif

// sor_fused_kernel with clocks: the same block-and-wave to tile mapping (tile_of_wave, then the lines of sor_fused_kernel that
// pick the tiling and the rectangle, MIRRORED here), the product's relax_tile, and a wait for the stores before the second clock
// read.  The probe never waits for a halo message and has no sender tiles, so neither piece of the product kernel is here.
template <class B, int NS, bool DX1, bool ZERO_IN>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(min_waves_per_simd(NS))))
sor_probe_kernel(float *p_out, const float *p_in, const float *d, Slab g, sor::Tiling t1, sor::Tiling t2, SorParams prm, int rot_c,
                 int rot_e, int free_blocks)
{
    __shared__ __attribute__((aligned(16))) float ring_mem[kWavesPerBlock][B::kRingFloats];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    int tile = tile_of_wave(wave, free_blocks);
    if (tile >= t1.n_tiles + t2.n_tiles) return;
    WaveTrace trace;
    trace.begin();
    const int trace_tile = tile;
    const bool second = tile >= t1.n_tiles;
    const sor::Tiling t = second ? t2 : t1;
    if (second) tile -= t1.n_tiles;
    const sor::TileRect rect = sor::tile_rect(t, tile, second ? 0 : rot_c, second ? 0 : rot_e);
#if SFL_PROBE_NO_EDGE
    const int kind = probe_relax_tile<B, NS, DX1, ZERO_IN>(p_out, p_in, d, g, t, rect, prm, ring_mem[wave], lane);
#else
    const int kind = relax_tile<B, NS, DX1, ZERO_IN>(p_out, p_in, d, g, t, rect, prm, false, ring_mem[wave], lane);
#endif
    __builtin_amdgcn_s_waitcnt(0);  // the wave's stores have left
    trace.end(trace_tile, kind);
}

// One probe launch of the product's plan: the backend is chosen as launch_lane chooses it (8-byte accesses where they are
// possible, non-temporal stores on large slabs), the geometry is what plan_launch decides for the product's kernel.
// dx == 1, p_in != nullptr, exact arithmetic, no halo wait.  *plan (optional) receives the plan.
template <int NS, bool VEC, int ST>
hipError_t probe_launch_as(hipStream_t s, float *p_out, const float *p_in, const float *d, Slab g, SorRows rows, SorParams prm,
                           int rows_per_chunk, int sweep, LaunchPlan *plan)
{
    const LaunchPlan pl = plan_launch<Lane2<NS, VEC, false, ST>, NS, true, false>(g, rows, rows_per_chunk, sweep, nullptr);
    if (plan) *plan = pl;
    if (pl.blocks == 0) return hipSuccess;
    sor_probe_kernel<ProbeLane2<NS, VEC, false, ST>, NS, true, false><<<pl.blocks, kThreads, 0, s>>>(
        p_out, p_in, d, g, pl.t1, pl.t2, prm, pl.rot_c, pl.rot_e, pl.free_blocks);
    return hipGetLastError();
}

template <int NS>
hipError_t probe_launch(hipStream_t s, float *p_out, const float *p_in, const float *d, Slab g, SorRows rows, SorParams prm,
                        int rows_per_chunk, int sweep, LaunchPlan *plan = nullptr)
{
    const uintptr_t all = reinterpret_cast<uintptr_t>(p_out) | reinterpret_cast<uintptr_t>(p_in) | reinterpret_cast<uintptr_t>(d);
    if (prm.dx != 1.0f || p_in == nullptr) return hipErrorInvalidValue;
    if ((g.dim_x % 2 != 0) || (all & 7) != 0)
        return probe_launch_as<NS, false, 0>(s, p_out, p_in, d, g, rows, prm, rows_per_chunk, sweep, plan);
    if ((size_t)g.lrows * (size_t)g.dim_x >= kNtStoreCells)
        return probe_launch_as<NS, true, 2>(s, p_out, p_in, d, g, rows, prm, rows_per_chunk, sweep, plan);
    return probe_launch_as<NS, true, 0>(s, p_out, p_in, d, g, rows, prm, rows_per_chunk, sweep, plan);
}

}  // namespace
}  // namespace sfl
