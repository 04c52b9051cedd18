// spmm_timeshare.h -- family 10, the shared form (spmm_sharering.h) in the
// masked mode for fields whose mask does not change from batch to batch:
// (Time, nCells, nVertLevels) ocean data cut by bathymetry.
// Part of remap_spmm.hip: included there inside namespace remap::(anonymous),
// in the order given there; not a stand-alone header.
// ---------------------------------------------------------------------------
// The masked mode (remap_numpy.py:262-266) sums `den = A . [not isnan X]`
// beside `num = A . [X, NaN -> 0]`, per column: the reference recomputes den
// for every time slice of a mask that depends on (cell, level) only, and so
// does the per-lane form of spmm_rowgroup -- 64 more VGPRs, one K tile per
// wave, config 5 with a bathymetry mask at 26.9 ms where the frac_b mode
// takes 21.  spmm_grouptime.h cut the normalisers to one per lane and row by
// taking four time slices of a level per lane, and stayed at 27.2 ms: beside
// 80 accumulators the registers hold four entries in flight, not eight, and
// the launch is bound by the L1 miss queue, not by the VALU.
//
// The shared form has no entries in flight in registers at all -- the LDS
// ring holds them -- and 12 VGPRs to spare at four waves per SIMD.  Here it
// runs with TIME-MAJOR columns:
//
//   * a workgroup's chunk is (64 levels) x (4 time slices); an entry's piece
//     is 4 x 512 bytes, sent as before by two global_load_lds_dwordx4 (lanes
//     0 - 31: one time slice, 32 - 63: the next): LDS holds [slice][level];
//   * a lane OWNS A LEVEL: it reads its level's four slices (4 ds_read_b64)
//     and keeps four sums and ONE normaliser per row -- while the four
//     slices of every lane are valid together or missing together;
//   * validity once per owned entry (four v_cmp_u_f64, scalar XORs); an
//     entry valid everywhere adds its products with no select.
//
// A wave that meets an entry whose validity differs between the slices of
// some lane keeps sending its pieces and keeping the barriers, and redoes ITS
// group afterwards with per-element normalisers, one slice at a time, from
// global memory (spmm_groupmask.h's general tile).  Nothing is assumed about
// the data: same sums, same order, same bits, with or without
// REMAP_FLAG_BATCH_MASKS.
// ---------------------------------------------------------------------------

// x where the lane's bit of `mask` is clear, +0.0 where it is set: two
// v_cndmask_b32 reading the mask from its SGPR pair (written as `mask >> lane
// & 1` hipcc shifts a 64-bit VGPR pair per element; written as `x != x ? 0 :
// x` it compares again).  Inside a branch on the mask: the asm is volatile so
// that the branch is not flattened into selects on every entry.
__device__ __forceinline__ double tshare_zero_where(double x, uint64_t mask)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    asm volatile("v_cndmask_b32_e64 %0, %0, 0, %2\n\t"
                 "v_cndmask_b32_e64 %1, %1, 0, %2"
                 : "+v"(lo), "+v"(hi)
                 : "s"(mask));
    return __hiloint2double(hi, lo);
}

// 1.0 where the lane's bit of `mask` is clear, +0.0 where it is set
__device__ __forceinline__ double tshare_one_where_clear(uint64_t mask)
{
    int hi = 0x3ff00000;
    asm volatile("v_cndmask_b32_e64 %0, %0, 0, %1" : "+v"(hi) : "s"(mask));
    return __hiloint2double(hi, 0);
}

template <bool FMA, int AHEAD>
__global__ __launch_bounds__(4 * kWave)
__attribute__((amdgpu_waves_per_eu(4, 8))) void spmm_timeshare(
    const KParams p, const uint32_t flags,
    const int64_t *__restrict__ gmeta, const int32_t *__restrict__ gcol,
    const double *__restrict__ gw, const int32_t *__restrict__ gmask,
    const int32_t *__restrict__ grid, const int64_t *__restrict__ smeta,
    const int32_t *__restrict__ scol, const int32_t *__restrict__ smask,
    const double *__restrict__ X)
{
    constexpr int G = kShareRows, TB = 4;
    // [slice][64 levels]; a lane reads its level's four slices
    typedef SharePiece<8, TB, 512> piece_t;
    typedef typename I32Vec<G>::type rvec_t;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t L = logical_block(p);
    if (L >= p.n_blocks)
        return;
    REMAP_CLOCK_BEGIN();
    const ShareWork wk =
        share_decode(p, L, wave, gmeta, gw, smeta, scol, smask);
    // chunk = (block of 64 levels, block of TB time slices), time blocks
    // side by side.  A slice or a level that does not exist is sent from,
    // and read as, the first slice (the row's first value): the same data
    // as an element that does exist, valid or missing with it; never stored.
    const uint32_t n_batch = p.K / p.k_inner;
    const uint32_t n_tb = (n_batch + TB - 1) / TB;
    const uint32_t lb = static_cast<uint32_t>(wk.chunk) / n_tb;
    const uint32_t tb = static_cast<uint32_t>(wk.chunk) - lb * n_tb;
    // the sending side: lane -> (slice 2 t + lane / 32, two levels)
    // (64-bit offsets: the time slices of a (Time, nCells, nVertLevels)
    // field on a 3.7 M-cell mesh are 1.9 GB apart)
    uint64_t xob[2];
    {
        const uint32_t k2 = lb * kWave + 2u * (lane & 31);
        const bool k_on = k2 < p.k_inner;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t b = tb * TB + 2 * t + (lane >> 5);
            const uint32_t bx = b < n_batch ? b : tb * TB;
            xob[t] = k_on ? static_cast<uint64_t>(
                                (static_cast<int64_t>(bx) * p.bsx + k2) * 8)
                          : static_cast<uint64_t>(
                                static_cast<int64_t>(tb * TB) * p.bsx * 8);
        }
    }
    // (the summing side -- lane = level, element e = slice tb * TB + e --
    // needs its offsets only behind the step loop: computed there, 12
    // registers that decide between three and four waves per SIMD)
    const uint32_t ldx_bytes = static_cast<uint32_t>(p.ldx) * 8u;

    double acc[G][TB][1];
    double den_l[G];
#pragma unroll
    for (int m = 0; m < G; ++m) {
        den_l[m] = 0.0;
#pragma unroll
        for (int e = 0; e < TB; ++e)
            acc[m][e][0] = 0.0;
    }
    // lanes that met an entry whose slices disagree: != 0 -> the general form
    uint64_t mixed_bits = 0;

    share_walk<piece_t, AHEAD>(
        p, wk, lane, wave,
        [&](char *const dst, const int32_t c0, const int32_t c1) {
            share_send_rows<2>(dst, X, ldx_bytes, xob, c0, c1);
        },
        [&](const piece_t &xp, const uint32_t word, auto sb_c,
            const double my_w, int &idx) {
            constexpr int sb = decltype(sb_c)::value;
            double x[TB];
#pragma unroll
            for (int e = 0; e < TB; ++e)
                x[e] = xp.x[e];
            // lanes whose slice e is missing; lanes whose slices disagree
            // (kept as BITS: tested as a number, hipcc turns every `^` into
            // s_cmp + s_cselect)
            uint64_t nan_m[TB];
#pragma unroll
            for (int e = 0; e < TB; ++e)
                nan_m[e] = __ballot(x[e] != x[e]);
#pragma unroll
            for (int e = 1; e < TB; ++e)
                mixed_bits |= nan_m[e] ^ nan_m[0];
            if (mixed_bits == 0) {
                // valid in every lane and slice (the open ocean): the
                // products as they are; else missing in some lanes, in all
                // their slices: those lanes add a * 0.0 to num and to den --
                // selected by slice 0's mask, which is every slice's,
                // straight from its SGPR pair
                double vf = 1.0;
                if (nan_m[0] != 0) {
#pragma unroll
                    for (int e = 0; e < TB; ++e)
                        x[e] = tshare_zero_where(x[e], nan_m[0]);
                    vf = tshare_one_where_clear(nan_m[0]);
                }
#pragma unroll
                for (int m = 0; m < G; ++m) {
                    if (word & (1u << (sb + m))) {
                        const double a = readlane_f64(my_w, idx);
                        ++idx;
#pragma unroll
                        for (int e = 0; e < TB; ++e)
                            acc[m][e][0] =
                                mul_add<FMA>(a, x[e], acc[m][e][0]);
                        den_l[m] = den_add(a, vf, den_l[m]);
                    }
                }
            }
        });

    // the summing side's offsets: lane = level, element e = time slice
    const uint32_t k = lb * kWave + lane;
    const bool lane_on = k < p.k_inner;
    int64_t yoff[TB];
    bool act[TB];
#pragma unroll
    for (int e = 0; e < TB; ++e) {
        const uint32_t b = tb * TB + e;
        act[e] = lane_on && b < n_batch;
        yoff[e] = act[e] ? static_cast<int64_t>(b) * p.bsy + k : 0;
    }
    const bool mixed = mixed_bits != 0;
    if (wk.nmem > 0 && !mixed) {
        const rvec_t rid = *reinterpret_cast<const rvec_t *>(grid + wk.slot0);
#pragma unroll
        for (int m = 0; m < G; ++m) {
            if (m < wk.nmem)
                finish_row_lane_den<TB>(p, rid[m], den_l[m], act, yoff,
                                        acc[m]);
        }
    }
    if (wk.nmem > 0 && mixed) {
        // this wave's group again, with per-element normalisers, one time
        // slice at a time, from global memory (nobody waits for it: the
        // workgroup's last barrier is behind)
        const int64_t s = gmeta[2 * wk.g];
        const int64_t woff0 = gmeta[2 * wk.g + 1];
        const int64_t e_end = gmeta[2 * wk.g + 2];
#pragma unroll 1
        for (int e = 0; e < TB; ++e) {
            // (a slice is one batch: its offset goes into the base pointer,
            // the lane's own offset -- its level -- stays small)
            const uint32_t b_e = tb * TB + e;
            const double *X_e =
                X + static_cast<int64_t>(b_e < n_batch ? b_e : tb * TB) *
                        p.bsx;
            const uint32_t xo_e = lane_on ? k * 8u : 0u;
            const int64_t yoff_e = e == 0   ? yoff[0]
                                   : e == 1 ? yoff[1]
                                   : e == 2 ? yoff[2]
                                            : yoff[3];
            const bool act_e = e == 0   ? act[0]
                               : e == 1 ? act[1]
                               : e == 2 ? act[2]
                                        : act[3];
            groupmask_general_tile<double, FMA, G, 8, 1>(
                p, s, woff0, e_end, gcol, gw, gmask, grid, X_e, xo_e, yoff_e,
                act_e, wk.slot0, wk.nmem, lane);
        }
    }
    REMAP_CLOCK_END();
}
