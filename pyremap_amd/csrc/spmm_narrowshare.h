// spmm_narrowshare.h -- family 10, the shared form (spmm_sharering.h) for at
// most 64 columns: ONE 3-D field of up to 64 levels on an entry-rich mapping.
// Part of remap_spmm.hip: included there inside namespace remap::(anonymous),
// in the order given there; not a stand-alone header.
// ---------------------------------------------------------------------------
// spmm_groupshare gives a lane two columns per K tile: at 64 columns half of
// every wave idles, and the 8-row groups (one column per lane) are faster --
// each of them pulling its own copy of every source row through L1.  Here a
// lane owns ONE column (64 lanes = the 64 columns of the chunk, 512 bytes per
// source row), the four waves of a workgroup own a 4 x 8 tile of destination
// rows and share ONE union of source rows through the same two-buffer LDS
// ring, and an LDS-DMA instruction carries TWO union entries: lanes 0 - 31
// the 16-byte pieces of one source row, lanes 32 - 63 those of the next (the
// instruction takes an address per lane; the LDS side is linear in the lane).
// A step of 8 entries is ONE global_load_lds_dwordx4 per wave.  Everything
// else -- the lanes holding the list's columns and member bytes, the weights
// through a wave-private LDS slot, the member chain, the sums in ascending
// column order -- is the ring walk's (share_walk): the same bits.
// (Instantiated for the frac_b and raw modes.  The masked mode with its
// per-lane normalisers was measured on config 5's mapping and is not: K = 64
// 2.21 ms against 2.19 of the 8-row groups, 34: 2.25 against 2.13 --
// profiles/r06_analysis/config5_share.md section 9.)
// ---------------------------------------------------------------------------

template <int MODE, bool FMA, int AHEAD>
__global__ __launch_bounds__(4 * kWave) void spmm_narrowshare(
    const KParams p, const uint32_t flags,
    const int64_t *__restrict__ gmeta, const double *__restrict__ gw,
    const int32_t *__restrict__ grid, const double *__restrict__ gfrac,
    const int64_t *__restrict__ smeta, const int32_t *__restrict__ scol,
    const int32_t *__restrict__ smask, const double *__restrict__ X)
{
    constexpr int G = kShareRows, VEC = 1, TILES = 1;
    static_assert(MODE != REMAP_MODE_MASKED, "no per-lane normalisers here");
    static_assert(kShareEpw == 2,
                  "one DMA instruction = the wave's two entries");
    // 64 columns of one source row; a lane reads its own
    typedef SharePiece<8, 1, 512> piece_t;
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

    // the sending side: lane -> the wave's first (lanes 0 - 31) or second
    // entry of the step, columns 2 (lane % 32) and the next of the chunk's 64
    // (flat column -> batch, level as tile_offsets cuts them; a pair lies in
    // one batch: the level count is even); columns behind the last one send
    // the row's first piece -- harmless, never summed.  Byte offsets from a
    // source row's base, 64 bits wide (share_send_rows)
    uint64_t xob;
    {
        const uint32_t kf = static_cast<uint32_t>(wk.chunk) * kWave +
                            2u * (lane & 31);
        const bool on = kf < p.K;
        const uint32_t b = on ? kf / p.k_inner : 0u;
        const uint32_t kk = on ? kf - b * p.k_inner : 0u;
        xob = static_cast<uint64_t>(static_cast<int64_t>(b) * p.bsx + kk) *
              8u;
    }
    const bool upper = lane >= 32;
    const uint32_t ldx_bytes = static_cast<uint32_t>(p.ldx) * 8u;

    double acc[G][TILES][VEC];
#pragma unroll
    for (int m = 0; m < G; ++m)
        acc[m][0][0] = 0.0;

    share_walk<piece_t, AHEAD>(
        p, wk, lane, wave,
        // the wave's two entries of the step in ONE instruction
        [&](char *const dst, const int32_t c0, const int32_t c1) {
            const uint32_t c = static_cast<uint32_t>(upper ? c1 : c0);
            const char *src = reinterpret_cast<const char *>(X) +
                              static_cast<uint64_t>(c) * ldx_bytes + xob;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        },
        [&](const piece_t &x, const uint32_t word, auto sb_c,
            const double my_w, int &idx) {
            constexpr int sb = decltype(sb_c)::value;
#pragma unroll
            for (int m = 0; m < G; ++m) {
                if (word & (1u << (sb + m))) {
                    const double a = readlane_f64(my_w, idx);
                    ++idx;
                    acc[m][0][0] = mul_add<FMA>(a, x.x[0], acc[m][0][0]);
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
