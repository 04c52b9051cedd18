// spmm_cellshare.h -- family 10, the shared form (spmm_sharering.h) in the
// masked mode for fields whose cells are missing WHOLE (land, an ice shelf,
// a regional product: every column of the cell, or none):
// REMAP_FLAG_CELL_MASKS on a mapping with the shared lists.
// Part of remap_spmm.hip: included there inside namespace remap::(anonymous),
// in the order given there; not a stand-alone header.
// ---------------------------------------------------------------------------
// The masked mode (remap_numpy.py:262-266) sums `den = A . [not isnan X]`
// beside `num = A . [X, NaN -> 0]`.  While every source cell is valid in all
// of a wave's columns or missing in all of them, every lane's den is the same
// number, the sequential sum of the weights of the row's valid entries:
// spmm_groupmask.h keeps it in ONE register pair per row on the 8-row groups
// (config 5 with a quarter of the cells missing: 27.4 -> 22.4 ms).  This is
// the same normaliser on the shared form's decomposition -- a 4-wave
// workgroup per (4 x 8 tile of destination rows) x (256 columns), ONE union
// of source rows per tile through the two-buffer LDS ring, every
// vector-memory instruction of the loop an LDS-DMA:
//
//   * validity once per OWNED entry: two v_cmp_u_f64 over the lane's four
//     elements, a scalar OR; an entry valid everywhere adds the frac_b mode's
//     products and its weight onto the row's den (one add per (entry,
//     member)); an entry missing everywhere adds `a * 0.0` to num and den --
//     nothing, for a finite weight: skipped behind a test that the
//     weights are finite;
//   * the row's normaliser is wave-uniform: the frac_b mode's epilogue (one
//     reciprocal per row, finish_row_uniform) with `den > thr` in place of
//     `frac_b > 0`.
//
// A wave that meets an entry valid in some lanes or elements and missing in
// others (a field cut by bathymetry under a wrong hint), or a NaN / Inf
// weight on a missing cell, keeps sending its pieces and keeping the barriers
// and redoes ITS group afterwards with per-element normalisers, one K tile at
// a time, from global memory -- flat 64-bit addresses: the batches of a
// (Time, nCells, nVertLevels) field are further apart than a buffer offset
// reaches.  Nothing is assumed about the data: same sums, same order, same
// bits, with or without the flag.
// ---------------------------------------------------------------------------

template <bool FMA, int AHEAD>
__global__ __launch_bounds__(4 * kWave)
__attribute__((amdgpu_waves_per_eu(4, 8))) void spmm_cellshare(
    const KParams p, const uint32_t flags,
    const int64_t *__restrict__ gmeta, const int32_t *__restrict__ gcol,
    const double *__restrict__ gw, const int32_t *__restrict__ gmask,
    const int32_t *__restrict__ grid, const int64_t *__restrict__ smeta,
    const int32_t *__restrict__ scol, const int32_t *__restrict__ smask,
    const double *__restrict__ X)
{
    constexpr int G = kShareRows, VEC = 2, TILES = 2;
    typedef SharePiece<16, TILES, 1024> piece_t;
    typedef typename I32Vec<G>::type rvec_t;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t L = logical_block(p);
    if (L >= p.n_blocks)
        return;
    REMAP_CLOCK_BEGIN();
    const ShareWork wk =
        share_decode(p, L, wave, gmeta, gw, smeta, scol, smask);
    int64_t xoff[TILES], yoff[TILES];
    bool act[TILES];
    tile_offsets<VEC, TILES>(p, wk.chunk, lane, xoff, yoff, act);
    uint64_t xob[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t)
        xob[t] = static_cast<uint64_t>(xoff[t]) * 8u;
    const uint32_t ldx_bytes = static_cast<uint32_t>(p.ldx) * 8u;

    double acc[G][TILES][VEC];
    double den_u[G];
#pragma unroll
    for (int m = 0; m < G; ++m) {
        den_u[m] = 0.0;
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                acc[m][t][v] = 0.0;
    }
    bool mixed = false;

    share_walk<piece_t, AHEAD>(
        p, wk, lane, wave,
        [&](char *const dst, const int32_t c0, const int32_t c1) {
            share_send_rows<TILES>(dst, X, ldx_bytes, xob, c0, c1);
        },
        [&](const piece_t &x, const uint32_t word, auto sb_c,
            const double my_w, int &idx) {
            constexpr int sb = decltype(sb_c)::value;
            if (!mixed) {
                // lanes holding a NaN among their four elements
                const bool some = __builtin_isunordered(x.x[0][0], x.x[0][1]) ||
                                  __builtin_isunordered(x.x[1][0], x.x[1][1]);
                if (__ballot(some) == 0) {
                    // valid in every column: the frac_b mode's products, the
                    // weight onto the row's den
#pragma unroll
                    for (int m = 0; m < G; ++m) {
                        if (word & (1u << (sb + m))) {
                            const double a = readlane_f64(my_w, idx);
                            ++idx;
#pragma unroll
                            for (int t = 0; t < TILES; ++t)
#pragma unroll
                                for (int v = 0; v < VEC; ++v)
                                    acc[m][t][v] = mul_add<FMA>(a, x.x[t][v],
                                                                acc[m][t][v]);
                            den_u[m] = den_add(a, 1.0, den_u[m]);
                        }
                    }
                } else {
                    bool every = true;
#pragma unroll
                    for (int t = 0; t < TILES; ++t)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            const double xe = x.x[t][v];
                            every = every && (xe != xe);
                        }
                    if (__ballot(every) != ~0ull) {
                        mixed = true;   // -> the general form
                    } else {
                        // missing in every column: a * 0.0 onto num and den --
                        // nothing, for a finite weight
                        // (a NaN or Inf one: |a| == Inf or unordered, ORed
                        // over the members and tested once -- tested member
                        // by member hipcc takes a v_cmp_class_f64 for some,
                        // whose mask is the VGPR this kernel does not have)
                        bool odd = false;
#pragma unroll
                        for (int m = 0; m < G; ++m) {
                            if (word & (1u << (sb + m))) {
                                const double a = readlane_f64(my_w, idx);
                                odd |= !__builtin_islessgreater(
                                    __builtin_fabs(a), __builtin_inf());
                                ++idx;
                            }
                        }
                        if (odd)
                            mixed = true;
                    }
                }
            }
        });

    if (wk.nmem > 0 && !mixed) {
        const rvec_t rid = *reinterpret_cast<const rvec_t *>(grid + wk.slot0);
#pragma unroll
        for (int m = 0; m < G; ++m) {
            if (m < wk.nmem)
                finish_row_uniform<VEC, TILES>(p, rid[m], den_u[m],
                                               den_u[m] > p.thr, act, yoff,
                                               acc[m]);
        }
    }
    if (wk.nmem > 0 && mixed) {
        // this wave's group again, one K tile at a time, from global memory
        // (nobody waits for it: the workgroup's last barrier is behind)
        const int64_t s = gmeta[2 * wk.g];
        const int64_t woff0 = gmeta[2 * wk.g + 1];
        const int64_t e_end = gmeta[2 * wk.g + 2];
#pragma unroll 1
        for (int t = 0; t < TILES; ++t) {
            const bool first = t == 0;
            groupmask_general_tile<double, FMA, G, 4, VEC>(
                p, s, woff0, e_end, gcol, gw, gmask, grid, X,
                first ? xoff[0] : xoff[TILES - 1],
                first ? yoff[0] : yoff[TILES - 1],
                first ? act[0] : act[TILES - 1], wk.slot0, wk.nmem, lane);
        }
    }
    REMAP_CLOCK_END();
}
