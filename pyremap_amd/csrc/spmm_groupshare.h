// spmm_groupshare.h -- family 10, the shared form (spmm_sharering.h) of the
// frac_b and raw modes: 4 waves, one union, LDS; 128 or 256 columns per
// workgroup.
// Part of remap_spmm.hip: included there inside namespace remap::(anonymous),
// in the order given there; not a stand-alone header.
// ---------------------------------------------------------------------------
// A lane holds two columns of each of the workgroup's TILES K tiles: an
// entry's piece in the ring is TILES x 1 KiB, sent by TILES LDS-DMA
// instructions and read back with TILES ds_read_b128; the sums are
// spmm_rowgroup's, the epilogue the frac_b / raw one.  Why the form exists,
// what the ring is and what it relies on: spmm_sharering.h.
// (The masked mode with per-lane normalisers was built, measured on config 5
// and is not instantiated: 32.1 ms at one K tile and 37.8 at two against 27.0
// of the 8-row groups -- profiles/r06_analysis/config5_share.md.  The masked
// mode's shared forms are spmm_timeshare and spmm_cellshare.)
// ---------------------------------------------------------------------------

template <int TILES, int MODE, bool FMA, int AHEAD>
__global__ __launch_bounds__(kShareWaves *kWave) void spmm_groupshare(
    const KParams p, const uint32_t flags,
    const int64_t *__restrict__ gmeta, const double *__restrict__ gw,
    const int32_t *__restrict__ grid, const double *__restrict__ gfrac,
    const int64_t *__restrict__ smeta, const int32_t *__restrict__ scol,
    const int32_t *__restrict__ smask, const double *__restrict__ X)
{
    constexpr int G = kShareRows, VEC = 2;
    static_assert(MODE != REMAP_MODE_MASKED, "no per-lane normalisers here");
    static_assert(TILES == 1 || TILES == 2, "K tiles per wave");
    typedef SharePiece<16, TILES, 1024> piece_t;
    typedef typename I32Vec<G>::type rvec_t;
    typedef typename F64Vec<G>::type fvec_t;

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
#pragma unroll
    for (int m = 0; m < G; ++m)
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                acc[m][t][v] = 0.0;

    share_walk<piece_t, AHEAD>(
        p, wk, lane, wave,
        [&](char *const dst, const int32_t c0, const int32_t c1) {
            share_send_rows<TILES>(dst, X, ldx_bytes, xob, c0, c1);
        },
        [&](const piece_t &x, const uint32_t word, auto sb_c,
            const double my_w, int &idx) {
            constexpr int sb = decltype(sb_c)::value;
#pragma unroll
            for (int m = 0; m < G; ++m) {
                if (word & (1u << (sb + m))) {
                    const double a = readlane_f64(my_w, idx);
                    ++idx;
#pragma unroll
                    for (int t = 0; t < TILES; ++t)
#pragma unroll
                        for (int v = 0; v < VEC; ++v)
                            acc[m][t][v] =
                                mul_add<FMA>(a, x.x[t][v], acc[m][t][v]);
                }
            }
        });

    if (wk.nmem > 0) {
        const rvec_t rid = *reinterpret_cast<const rvec_t *>(grid + wk.slot0);
        fvec_t fbv;
        if constexpr (MODE == REMAP_MODE_FRACB)
            fbv = *reinterpret_cast<const fvec_t *>(gfrac + wk.slot0);
        const double no_den[TILES][VEC] = {};   // (the masked mode's)
#pragma unroll
        for (int m = 0; m < G; ++m) {
            if (m < wk.nmem) {
                const int64_t i = rid[m];
                double fb = 0.0;
                if constexpr (MODE == REMAP_MODE_FRACB)
                    fb = fbv[m];
                finish_row<VEC, TILES, MODE>(p, i, fb, act, yoff, acc[m],
                                             no_den);
            }
        }
    }
    REMAP_CLOCK_END();
}
