// spmm_sharering.h -- family 10, the SHARED form: what its kernels have in
// common -- the LDS ring, its layout, the work decode and the walk of a
// supergroup's union list.
// Part of remap_spmm.hip: included there inside namespace remap::(anonymous),
// in the order given there; not a stand-alone header.
// ---------------------------------------------------------------------------
// The row-group kernel (spmm_rowgroup.h) loads every distinct source row of a
// wave's 8 destination rows once per wave.  On entry-rich mappings (2nd-order
// conservative: config 5) neighbouring 8-row groups still share most of their
// source rows, every one of them pulls its own copy from L2, and the launch
// is bound by the L1 miss queue of the CU (profiles/r05_analysis/
// config5_forms.md: 218 GB of L1 fills for 30 GB of X).  Larger groups cut
// the fills and lose the occupancy that keeps that queue full: a wave has no
// room for more than 8 rows x 256 columns of accumulators at 3 waves per SIMD.
//
// Here W = 4 waves -- a workgroup -- own W consecutive 8-row groups, a
// SUPERGROUP: a 4 x 8 tile of the destination grid (the group tiles are
// walked inside such tiles: remap_groups_build's share_waves).  The
// supergroup has ONE sorted union of source rows (share_col, share_mask: bit
// 8 w + m = member m of wave w owns the entry; remap_share_build).  The list
// is walked in steps of UNR = 8 union entries through a ring of NBUF = 2
// buffers in LDS:
//
//   * every wave sends its share of a step's entries straight from global
//     memory into the ring by LDS-DMA (global_load_lds_dwordx4), one step
//     ahead of the sums -- each distinct source row enters the CU ONCE per
//     supergroup: 0.16 union entries per entry on config 5 where the 8-row
//     groups have 0.33;
//   * one s_barrier per step: behind it step s is in the ring for every wave
//     and the buffer of step s - 1 is free for step s + 1;
//   * every wave reads the step's entries from LDS (a few entries ahead of
//     the sums) and adds the ones its own 8 rows own -- exactly the inner
//     loop of spmm_rowgroup: member bits from the mask, the wave's weights
//     (group_w of the 8-row schedule: its own contiguous stream) handed over
//     by v_readlane with a running scalar index.  A row adds its own entries
//     in ascending column order: the same bits as every other family.
//
// What a kernel of the form brings: the bytes of one entry's PIECE in the
// ring and how a lane reads its part of it (SharePiece), how a wave SENDS its
// two entries of a step, and how it CONSUMES an entry its rows own
// (share_walk's two callbacks).  Everything else is written here, once.
//
// (Built, measured on config 5 and not kept: 2-wave workgroups over 4 x 4
// tiles, 28.5 ms against 20.5; rings of 8 x 3, 4 x 3, 4 x 4 entries x
// buffers, 31.2 / 21.4 / 21.2 -- profiles/r06_analysis/config5_share.md.
// With more than two buffers the wait in front of the barrier becomes
// vmcnt(DMAs of the steps that may stay in flight): see share_barrier_w.)
//
// Inside the step loop EVERY vector-memory instruction is an LDS-DMA and
// every step issues the same number of them -- the step's weights travel the
// same way, into a small wave-private ring -- so that "step s has landed" is
// the immediate of one s_waitcnt vmcnt(N): loads return in order, and a plain
// load issued between the DMAs could only be awaited together with
// everything issued before it.  Entries behind the list's end re-send its
// last entry (an L1 hit).
//
// Columns and masks do not pass through the scalar cache here: a scalar load
// in flight turns every LDS wait into lgkmcnt(0).  They are fetched once per
// segment of 128 union entries (nearly every list is one segment), one per
// lane, cut down to this wave's 8 member bits, and handed out by v_readlane;
// the weights each step takes are counted on the vector side (DPP adds) and
// summed up once per segment.  (The first build extracted bits and counts
// entry by entry on the scalar unit: 100 SALU instructions per step, 5.7e9
// per launch against the row-group kernel's 3.5e9, and an on-chip floor of
// 17.7 ms where that kernel has 14.6 -- profiles/r06_analysis.)
// ---------------------------------------------------------------------------

// The ring's shape: waves per workgroup, union entries per step, buffers,
// rows per wave; entries a wave sends per step; union entries per segment.
constexpr int kShareWaves = 4, kShareUnr = 8, kShareBufs = 2, kShareRows = 8;
constexpr int kShareEpw = kShareUnr / kShareWaves;
constexpr int kShareSeg = 2 * kWave;

// The ring's layout in dynamic LDS for pieces of ENTRY_BYTES per union entry:
// NBUF buffers of UNR entries, then NBUF x W slots of a step's weights, then
// slack for the lanes that read past the last slot.  The kernels and their
// launch sites both take their numbers from here.
template <int ENTRY_BYTES>
struct ShareRing {
    static constexpr int kEntryBytes = ENTRY_BYTES;
    static constexpr int kBufBytes = kShareUnr * ENTRY_BYTES;
    static constexpr int kWSlot = kShareUnr * kShareRows * 8;   // at most
    static constexpr int kWDma = kWSlot / 256;   // 256 bytes per instruction
    static constexpr int kWOffset = kShareBufs * kBufBytes;
    static constexpr uint32_t kLdsBytes =
        kShareBufs * (kBufBytes + kShareWaves * kWSlot) + 512;
};

// compile-time loop: the body sees its index as a constant (the offsets of
// the LDS reads below are instruction immediates)
template <int... I, typename F>
__device__ __forceinline__ void share_static_for(
    std::integer_sequence<int, I...>, F &&f)
{
    (f(std::integral_constant<int, I>{}), ...);
}

// The DMAs of this wave up to the N last ones have landed, every LDS read of
// the last step is done; then the workgroup's barrier.  (Not __syncthreads():
// that drains vmcnt altogether.)
template <int N>
__device__ __forceinline__ void share_barrier()
{
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier"
                 :
                 : "n"(N)
                 : "memory");
}

// The same with the read of the step's weights -- the wave's own slot, landed
// once ITS DMAs have -- issued in front of the barrier: its trip to LDS runs
// while the other waves arrive.
#ifdef REMAP_DIAG
// (ablation: the waits and the read without the barrier)
template <int N>
__device__ __forceinline__ void share_nobarrier_w(double &w, uint32_t addr)
{
    asm volatile("s_waitcnt vmcnt(%2) lgkmcnt(0)\n\t"
                 "ds_read_b64 %0, %1"
                 : "=v"(w)
                 : "v"(addr), "n"(N)
                 : "memory");
}
#endif

template <int N>
__device__ __forceinline__ void share_barrier_w(double &w, uint32_t addr)
{
    asm volatile("s_waitcnt vmcnt(%2) lgkmcnt(0)\n\t"
                 "ds_read_b64 %0, %1\n\ts_barrier"
                 : "=v"(w)
                 : "v"(addr), "n"(N)
                 : "memory");
}

// (the step's weights: lane j's is weight j of the wave's slot)
template <int N>
__device__ __forceinline__ void share_wait_w(double &w)
{
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(w) : "n"(N));
}

// A lane's part of one union entry's piece in the ring: N reads of BYTES (8:
// one double, 16: two), STRIDE bytes apart; the piece is N x STRIDE bytes.
// The ring is read with explicit ds_read / s_waitcnt lgkmcnt(CNT): left to
// hipcc, every read into a register whose last value was never used (an
// entry this wave's rows do not own) is preceded by `s_waitcnt lgkmcnt(0)`
// -- the reads ahead are drained at every entry that is skipped, and more
// than half of them are.  LDS reads return in order and nothing else in the
// loop counts on lgkmcnt, so CNT = the reads issued behind the one awaited (a
// scalar load the compiler may add only makes the wait longer, never too
// short).  The "+v" operands tie the uses of the values behind the wait.
typedef double share_x2 __attribute__((ext_vector_type(2)));

template <int BYTES, int N, int STRIDE>
struct SharePiece {
    static_assert((BYTES == 8 || BYTES == 16) && (N == 1 || N == 2 || N == 4),
                  "piece shape");
    static constexpr int kReads = N, kLaneBytes = BYTES;
    static constexpr int kEntryBytes = N * STRIDE;
    typedef std::conditional_t<BYTES == 16, share_x2, double> elem_t;
    elem_t x[N];

    template <int OFF>
    static __device__ __forceinline__ void read_one(elem_t &v,
                                                    const uint32_t addr)
    {
        if constexpr (BYTES == 16)
            asm volatile("ds_read_b128 %0, %1 offset:%2"
                         : "=v"(v)
                         : "v"(addr), "n"(OFF));
        else
            asm volatile("ds_read_b64 %0, %1 offset:%2"
                         : "=v"(v)
                         : "v"(addr), "n"(OFF));
    }

    // the lane's reads of the piece OFF bytes behind addr
    template <int OFF>
    __device__ __forceinline__ void read(const uint32_t addr)
    {
        read_one<OFF>(x[0], addr);
        if constexpr (N >= 2)
            read_one<OFF + STRIDE>(x[1], addr);
        if constexpr (N == 4) {
            read_one<OFF + 2 * STRIDE>(x[2], addr);
            read_one<OFF + 3 * STRIDE>(x[3], addr);
        }
    }

    template <int CNT>
    __device__ __forceinline__ void wait()
    {
        if constexpr (N == 1)
            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x[0]) : "n"(CNT));
        else if constexpr (N == 2)
            asm volatile("s_waitcnt lgkmcnt(%2)"
                         : "+v"(x[0]), "+v"(x[1])
                         : "n"(CNT));
        else
            asm volatile("s_waitcnt lgkmcnt(%4)"
                         : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])
                         : "n"(CNT));
    }
};

// Member bytes of the 8 entries of a step, packed into the step's first
// lane (row_shl: lane i reads lane i + n of its row of 16): lo = entries
// 0 - 3 (byte j = entry j), hi = entries 4 - 7 -- two v_readlane per step
// instead of eight.
__device__ __forceinline__ void share_pack_step(int32_t mine, int32_t &lo,
                                                int32_t &hi)
{
    int32_t t = mine | (__builtin_amdgcn_update_dpp(0, mine, 0x101, 0xf, 0xf,
                                                    true)
                        << 8);
    t |= __builtin_amdgcn_update_dpp(0, t, 0x102, 0xf, 0xf, true) << 16;
    lo = t;
    hi = __builtin_amdgcn_update_dpp(0, t, 0x104, 0xf, 0xf, true);
}

// v = w behind a SCALAR branch (left to itself hipcc turns `half ? a : b`
// into s_cmp, s_cselect, v_cndmask in every step of the loop)
__device__ __forceinline__ void share_switch(int32_t &v, int32_t w)
{
    asm volatile("v_mov_b32 %0, %1" : "+v"(v) : "v"(w));
}

// What a wave of a workgroup works on: its K chunk and supergroup, its 8-row
// group g (rows [slot0, slot0 + nmem) of the schedule), the supergroup's list
// [0, len) of union entries and this wave's stream of weights (32-bit
// positions from here on), the shift to its member bits.
struct ShareWork {
    int64_t chunk, sg, g, slot0;
    bool have;
    int nmem, len, sh;
    const int32_t *lcol, *lmask;
    const double *lw;
};

__device__ __forceinline__ ShareWork share_decode(
    const KParams &p, const int64_t L, const int wave,
    const int64_t *__restrict__ gmeta, const double *__restrict__ gw,
    const int64_t *__restrict__ smeta, const int32_t *__restrict__ scol,
    const int32_t *__restrict__ smask)
{
    constexpr int G = kShareRows;
    ShareWork k;
    if (p.xcd_map & 2) {
        const int64_t n_chunks = p.n_blocks / p.n_rowblocks;
        k.sg = L / n_chunks;
        k.chunk = L - k.sg * n_chunks;
    } else {
        k.chunk = L / p.n_rowblocks;
        k.sg = L - k.chunk * p.n_rowblocks;
    }
    const int64_t n_slots = p.row_end - p.row_begin;
    const int64_t n_groups = (n_slots + G - 1) / G;
    k.g = k.sg * kShareWaves + wave;
    // (a wave past the last group sends its share of the pieces and keeps
    // the barriers; it owns no entry and no row)
    k.have = k.g < n_groups;
    k.slot0 = k.g * G;
    k.nmem = !k.have ? 0
             : (n_slots - k.slot0) < G
                 ? static_cast<int>(n_slots - k.slot0)
                 : G;
    const int64_t s0 = smeta[2 * k.sg];
    k.len = static_cast<int>(smeta[2 * k.sg + 2] - s0);
    k.lcol = scol + s0;
    k.lmask = smask + s0;
    k.lw = gw + gmeta[2 * (k.have ? k.g : n_groups) + 1];
    k.sh = wave * G;
    return k;
}

// A wave's two entries of a step whose pieces are NP DMA instructions of
// 1 KiB each, entry after entry in the ring: source rows c0 and c1, the
// lane's byte offsets xob[] from a row's base -- 64 bits: the batches of a
// (Time, nCells, nVertLevels) field on a 3.7 M-cell mesh are 1.9 GB apart,
// and the DMA takes a flat address per lane anyway; a row's base from its
// index with one 32 x 32 -> 64 bit product (the host checked that range).
template <int NP>
__device__ __forceinline__ void share_send_rows(
    char *const dst, const double *__restrict__ X, const uint32_t ldx_bytes,
    const uint64_t (&xob)[NP], const int32_t c0, const int32_t c1)
{
#pragma unroll
    for (int i = 0; i < kShareEpw; ++i) {
        const char *src =
            reinterpret_cast<const char *>(X) +
            static_cast<uint64_t>(static_cast<uint32_t>(i == 0 ? c0 : c1)) *
                ldx_bytes;
#pragma unroll
        for (int t = 0; t < NP; ++t)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(
                    src + xob[t]),
                (__attribute__((address_space(3))) void *)(
                    dst + (i * NP + t) * 1024),
                16, 0, 0);
    }
}

// The walk of the supergroup's union list.  Two callbacks:
//
//   send_entries(dst, c0, c1)   issue this wave's entry DMAs of one step:
//       its two entries' source rows c0, c1 (scalars), their place in the
//       ring `dst` (2 x Piece::kEntryBytes).  The SAME number of DMA
//       instructions every time.
//   consume(x, word, sb, my_w, idx)   an entry this wave's rows own: its
//       piece x (awaited), its member byte (bits sb ... sb + 7 of `word`; sb
//       a std::integral_constant), the step's weights my_w (lane j: weight
//       j) and the running scalar index idx of the next one, to be advanced
//       by the number of members.
//
// Both must inline completely and keep their state in registers: scalars
// and references to single registers across this boundary, never a local
// array indexed by a lane-dependent value (hipcc makes that private memory).
// AHEAD: entries read from LDS in front of the sums.
// REMAP_DIAG ablations (WRONG results, timing only): 4 = no s_barrier, 8 =
// no sums, 16 = no DMA sends.
template <typename Piece, int AHEAD, typename Send, typename Consume>
__device__ __forceinline__ void share_walk(
    const KParams &p, const ShareWork &wk, const int lane, const int wave,
    Send &&send_entries, Consume &&consume)
{
    typedef ShareRing<Piece::kEntryBytes> R;
    constexpr int W = kShareWaves, UNR = kShareUnr, NBUF = kShareBufs;
    constexpr int EPW = kShareEpw, kSeg = kShareSeg;
    static_assert(AHEAD >= 1 && AHEAD < UNR && AHEAD * Piece::kReads <= 15,
                  "LDS reads ahead of the sums");
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const uint32_t ring_lds = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(
        (__attribute__((address_space(3))) char *)ring));
    char *const wring = ring + R::kWOffset;
    const uint32_t wring_lds = ring_lds + R::kWOffset;
    const int len = wk.len, sh = wk.sh;
    const int32_t *__restrict__ lcol = wk.lcol;
    const int32_t *__restrict__ lmask = wk.lmask;
    const double *__restrict__ lw = wk.lw;

    int seg_w = 0;   // weights of this wave's stream the earlier segments took
    for (int seg0 = 0; seg0 < len; seg0 += kSeg) {
        const int seg_len = (len - seg0) < kSeg ? len - seg0 : kSeg;
        const int seg_steps = (seg_len + UNR - 1) / UNR;
        if (seg0 > 0)   // the ring of the segment before is read to the end
            share_barrier<0>();
        // columns and masks of the segment, one entry per lane and block (the
        // arrays are padded: always in bounds); the masks cut down to this
        // wave's member bits (none behind the list's end); in the lanes of a
        // step the number of bits set in the step
        int32_t colv[2], bitsv[2], bitsh[2], cntv[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            colv[b] = lcol[seg0 + b * kWave + lane];
            const int32_t raw = lmask[seg0 + b * kWave + lane];
            int32_t mine = (raw >> sh) & 0xff;
            mine = seg0 + b * kWave + lane < len ? mine : 0;
            int32_t pc = __builtin_popcount(mine);
            pc += __builtin_amdgcn_update_dpp(0, pc, 0xB1, 0xf, 0xf, true);
            pc += __builtin_amdgcn_update_dpp(0, pc, 0x4E, 0xf, 0xf, true);
            pc += __builtin_amdgcn_update_dpp(0, pc, 0x141, 0xf, 0xf, true);
            share_pack_step(mine, bitsv[b], bitsh[b]);
            cntv[b] = pc;
        }
        // (the loads above are awaited HERE, in straight-line code: met
        // first behind a branch, hipcc's wait-count pass no longer knows
        // whether they are still in flight and puts `s_waitcnt vmcnt(0)` in
        // front of every send of the pipeline's fill -- each of them then
        // waits for the one before to land)
        asm volatile("" : : "v"(colv[0]), "v"(colv[1]));
        // lane j: the weights the steps before step j of the segment took
        int32_t cumv = 0;
        {
            int run = seg_w;
            for (int j = 0; j < seg_steps; ++j) {
                cumv = lane == j ? run : cumv;
                const int e = j * UNR;
                run += __builtin_amdgcn_readlane(
                    e < kWave ? cntv[0] : cntv[1], e & (kWave - 1));
            }
            seg_w = run;
        }

        // the half of the segment (64 entries: one register of columns, two
        // of member bytes) the sending side / the summing side is in
        int32_t col_s = colv[0], bits_lo = bitsv[0], bits_hi = bitsh[0];
        // this wave's pieces of step st of the segment: its entries of the
        // step and the step's weights
        auto send = [&](const int st) {
            const int buf = st % NBUF;
            if (st * UNR == kWave)
                share_switch(col_s, colv[1]);
            if (REMAP_DIAG_ON(p, 16))
                return;
            int e0 = st * UNR + wave * EPW, e1 = e0 + 1;
            e0 = e0 < seg_len ? e0 : seg_len - 1;   // (same step, same half)
            e1 = e1 < seg_len ? e1 : seg_len - 1;
            int32_t c0 = __builtin_amdgcn_readlane(col_s, e0 & (kWave - 1));
            int32_t c1 = __builtin_amdgcn_readlane(col_s, e1 & (kWave - 1));
            REMAP_DIAG_COL(p, c0);
            REMAP_DIAG_COL(p, c1);
            send_entries(ring + buf * R::kBufBytes +
                             wave * EPW * R::kEntryBytes,
                         c0, c1);
            const int wo = __builtin_amdgcn_readlane(cumv, st);
            const char *wsrc = reinterpret_cast<const char *>(lw + wo);
#pragma unroll
            for (int q = 0; q < R::kWDma; ++q)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(
                        wsrc + q * 256 + lane * 4),
                    (__attribute__((address_space(3))) void *)(
                        wring + (buf * W + wave) * R::kWSlot + q * 256),
                    4, 0, 0);
        };

        // the pipeline fills: step 0 leaves
        if (seg_steps > 0)
            send(0);
        for (int st = 0; st < seg_steps; ++st) {
            const int buf = st % NBUF;
            // step st has landed in this wave's eyes when none of its DMAs
            // is in flight (two buffers: only step st's can be)
            double my_w;
            const uint32_t my_w_lds =
                wring_lds + (buf * W + wave) * R::kWSlot + lane * 8;
#ifdef REMAP_DIAG
            if (REMAP_DIAG_ON(p, 4))
                share_nobarrier_w<0>(my_w, my_w_lds);
            else
#endif
                share_barrier_w<0>(my_w, my_w_lds);
            // ... and in everybody's behind the barrier, and the buffer of
            // step st - 1 is free: step st + 1 leaves
            if (st + 1 < seg_steps)
                send(st + 1);
            const int e0 = st * UNR;
            if (e0 == kWave) {
                share_switch(bits_lo, bitsv[1]);
                share_switch(bits_hi, bitsh[1]);
            }
            const uint32_t step_lo = static_cast<uint32_t>(
                __builtin_amdgcn_readlane(bits_lo, e0 & (kWave - 1)));
            const uint32_t step_hi = static_cast<uint32_t>(
                __builtin_amdgcn_readlane(bits_hi, e0 & (kWave - 1)));

            // the step's entries from LDS, AHEAD of the sums (its weights
            // were asked for in front of the barrier)
            const uint32_t mine =
                ring_lds + buf * R::kBufBytes + lane * Piece::kLaneBytes;
            Piece xr[AHEAD + 1];
            share_static_for(
                std::make_integer_sequence<int, AHEAD>{}, [&](auto d_c) {
                    constexpr int d = decltype(d_c)::value;
                    xr[d].template read<d * R::kEntryBytes>(mine);
                });
            share_wait_w<AHEAD * Piece::kReads>(my_w);
            int idx = 0;   // scalar: next weight of the step
            share_static_for(
                std::make_integer_sequence<int, UNR>{}, [&](auto uu_c) {
                    constexpr int uu = decltype(uu_c)::value;
                    constexpr int slot = uu % (AHEAD + 1);
                    if constexpr (uu + AHEAD < UNR) {
                        constexpr int nx = (uu + AHEAD) % (AHEAD + 1);
                        xr[nx].template read<(uu + AHEAD) * R::kEntryBytes>(
                            mine);
                    }
                    // the entry's member byte: tested in place
                    const uint32_t word = uu < 4 ? step_lo : step_hi;
                    constexpr int sb = 8 * (uu & 3);
                    if ((word & (0xffu << sb)) && !REMAP_DIAG_ON(p, 8)) {
                        // reads issued behind this entry's: those of the
                        // entries uu + 1 ... min(uu + AHEAD, UNR - 1)
                        constexpr int behind =
                            (uu + AHEAD < UNR ? AHEAD : UNR - 1 - uu) *
                            Piece::kReads;
                        xr[slot].template wait<behind>();
                        consume(xr[slot], word,
                                std::integral_constant<int, sb>{}, my_w, idx);
                    }
                });
        }
    }
}
