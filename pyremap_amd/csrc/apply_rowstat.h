// apply_rowstat.h -- REMAP_MODE_MIN, _MAX, _VAR and _MEDIAN of
// remap_apply_f64: sub-grid statistics (CDO's remapmin, remapmax, remapvar,
// remapmedian).  Every other mode gives a destination element one number that
// stands for the mean over its cell; these say how the source values under
// the cell spread: the roughness of a topography, the shallowest and deepest
// depth, a median that outliers do not pull.  Included by remap_spmm.hip;
// stands on rowpass.h; the forms and the launch decisions are apply_laf.h's.
//
// Definition (include/remap_hip.h has the contract;
// pyremap_amd.rowstat.row_statistic is the same statement in numpy).
// For destination element (i, b, k) the entries j of row i are walked in
// CSR order:
//   x_j = (double) X[cell(col_j), b, k]
//   an entry counts iff x_j is no NaN; +-inf are values like any other
//   valid starts at +0.0; for every counted entry, in CSR order,
//   valid = valid + S_j, each sum rounded
//   ok = (some entry counts) && valid > threshold; where !ok, y = NaN
// MIN / MAX:
//   the first counted x sets m; after it, if (x < m) m = x  (MAX: >)
//   strict, so the first seen wins a tie and -0.0 against +0.0 is
//   decided by CSR order (remap_limit_rows has the same rule)
//   weights enter only through valid; y = m
// VAR (weighted population variance, in two walks):
//   walk 1: num starts at +0.0; for counted entries
//   num = num + (S_j * x_j), the product rounded and the sum rounded;
//   mean = num / valid
//   walk 2: m2 starts at +0.0; for counted entries d = x_j - mean;
//   m2 = m2 + (S_j * (d * d)), every operation rounded, no FMA
//   contraction
//   y = m2 / valid; a NaN result is written as the canonical NaN (an inf
//   among the values gives inf - inf)
// MEDIAN (lower weighted median, needs no table):
//   half = 0.5 * valid
//   for a counted entry j, below_j starts at +0.0 and adds S_q, in CSR
//   order, over the counted q of the row with x_q <= x_j (j itself
//   included)
//   j qualifies iff below_j >= half
//   y is the least x_j among the qualifying entries (strict <: the first
//   seen wins a tie); none qualifies: y = NaN
// Every NaN written is 0x7ff8000000000000.  (Built with -ffp-contract=off, as
// every apply kernel: a product and the sum that takes it stay two roundings.)
//
// Register form.  A row of at most kSlots entries -- most rows: the metric
// map averages 3.3 entries a row -- is gathered once, all its loads in flight
// together: its x stay in registers, slot c holding entry c of the row (a NaN
// x, or a slot past the row's end, is a slot that does not count), and every
// walk of the definition -- VAR's second, both loops of MEDIAN -- runs over
// the slots, unrolled, every index a constant: nothing is indexed at run time
// and nothing goes to scratch.  Which form a row takes depends on its length
// alone, so it is the same in every lane of a wave.  A longer row is walked
// from memory, four gathers in flight; VAR gathers it a second time (L1: the
// row was just read), MEDIAN takes the rescan: its candidates j in chunks of
// kSlots, a chunk's x_j and below_j in registers, the row's (x_q, S_q)
// streamed past them.  Both routes perform the operations of the definition
// in the order of the definition, so the bytes are the same.
//
// Two forms, as apply_laf.h has them:
//   rowlane  one lane per (row, column), for runs shorter than a wave,
//            columns fastest across the lanes, or rows for runs shorter than
//            kRowsFastRun in several batches;
//   rowwave  one wave per (row, chunk of kWave * VEC columns) for
//            k_inner >= kWave: col and val are wave-uniform scalar loads, Y
//            leaves once through store_once.
// Registers and global memory only: no workgroup memory, no read-modify-write
// of memory, every element written once by the lane that owns it.
#ifndef REMAP_APPLY_ROWSTAT_H
#define REMAP_APPLY_ROWSTAT_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace rowstat {

using namespace rowpass;

constexpr char kName[] = "remap_apply_f64";
constexpr int kSlots = 8;             // entries a row keeps in registers
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)
constexpr unsigned kMaxGridY = 65535;

enum Stat { kMin, kMax, kVar, kMedian };

struct StatParams {                 // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    double *__restrict__ Y;
    uint8_t *__restrict__ mask_out;
    const int32_t *__restrict__ gate;
    int32_t gate_value;
    double thr;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner
    int64_t ldx, bsx, ldy, bsy;
    int64_t src_outer;
    uint32_t src_fold;
    int64_t total;                  // n_rows * K
    uint32_t cols_per_block;        // rowlane, columns fastest: the lanes of
    uint32_t rows_per_block;        // a block are rows_per_block rows of
                                    // cols_per_block columns
};

__device__ inline bool gate_closed(const StatParams &p)
{
    return p.gate != nullptr && *p.gate != p.gate_value;
}

__device__ inline double quiet_nan()
{
    return __longlong_as_double(0x7ff8000000000000LL);
}

// element offset of source cell a in X
__device__ inline int64_t x_offset(const StatParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// VEC neighbouring columns of source cell a, widened
template <typename XT, int VEC>
__device__ inline Pack<double, VEC> gather(const StatParams &p,
                                           const XT *__restrict__ X,
                                           int32_t a)
{
    const Pack<XT, VEC> x =
        *reinterpret_cast<const Pack<XT, VEC> *>(X + x_offset(p, a));
    Pack<double, VEC> out;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        out.v[v] = static_cast<double>(x.v[v]);
    return out;
}

// What one walk over the row keeps of an element: valid, whether an entry
// counted, and m (MIN / MAX) or num (VAR).
struct Walk {
    double valid, acc;
    bool any;
};

template <int STAT>
__device__ inline void count(Walk &t, double x, double s)
{
    if (!(x == x))
        return;
    t.valid = t.valid + s;
    if constexpr (STAT == kMin)
        t.acc = (!t.any || x < t.acc) ? x : t.acc;
    else if constexpr (STAT == kMax)
        t.acc = (!t.any || x > t.acc) ? x : t.acc;
    else if constexpr (STAT == kVar)
        t.acc = t.acc + (s * x);
    t.any = true;
}

// The first walk of every statistic over entries [s, e), four gathers in
// flight.  (The index of a gather past the end is the last entry's: one code
// path for every length, nothing read outside the row.)
template <int STAT, typename XT, int VEC>
__device__ inline void walk(const StatParams &p, const XT *__restrict__ X,
                            int64_t s, int64_t e, Walk (&t)[VEC])
{
    constexpr int UNR = 4;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        t[v].valid = 0.0;
        t[v].acc = 0.0;
        t[v].any = false;
    }
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double w[UNR];
        Pack<double, VEC> xs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            w[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            xs[u] = gather<XT, VEC>(p, X, c[u]);
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    count<STAT>(t[v], xs[u].v[v], w[u]);
            }
    }
}

// VAR, walk 2: m2 of the elements around their means
template <typename XT, int VEC>
__device__ inline void spread(const StatParams &p, const XT *__restrict__ X,
                              int64_t s, int64_t e,
                              const double (&mean)[VEC], double (&m2)[VEC])
{
    constexpr int UNR = 4;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        m2[v] = 0.0;
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double w[UNR];
        Pack<double, VEC> xs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            w[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            xs[u] = gather<XT, VEC>(p, X, c[u]);
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double x = xs[u].v[v];
                    const double d = x - mean[v];
                    const double term = w[u] * (d * d);
                    m2[v] = x == x ? m2[v] + term : m2[v];
                }
            }
    }
}

// One candidate of MEDIAN behind its below: y is the least qualifying x so
// far (has: there is one).
__device__ inline void qualify(double x, double below, double half,
                               double &y, bool &has)
{
    const bool take = x == x && below >= half && (!has || x < y);
    y = take ? x : y;
    has = has || take;
}

// The statistic of a row of at most kSlots entries, from registers: the row
// is gathered once, all of it in flight at a time, and every walk of the
// definition runs over the slots.  valid comes out beside it.
template <int STAT, typename XT, int VEC>
__device__ inline void slots_form(const StatParams &p,
                                  const XT *__restrict__ X, int64_t s,
                                  int64_t e, double (&valid)[VEC],
                                  bool (&any)[VEC], double (&y)[VEC])
{
    double w[kSlots];
    Pack<double, VEC> x[kSlots];
    int32_t c[kSlots];
#pragma unroll
    for (int n = 0; n < kSlots; ++n) {
        const int64_t jj = s + n < e ? s + n : e - 1;
        c[n] = p.col[jj];
        w[n] = p.val[jj];
    }
#pragma unroll
    for (int n = 0; n < kSlots; ++n) {
        x[n] = gather<XT, VEC>(p, X, c[n]);
        if (!(s + n < e)) {         // a slot past the row's end counts not
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                x[n].v[v] = quiet_nan();
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        double sum = 0.0;
        bool some = false;
#pragma unroll
        for (int n = 0; n < kSlots; ++n) {
            const bool counts = x[n].v[v] == x[n].v[v];
            sum = counts ? sum + w[n] : sum;
            some = some || counts;
        }
        valid[v] = sum;
        any[v] = some;
        if constexpr (STAT == kMin || STAT == kMax) {
            double m = 0.0;
            bool has = false;
#pragma unroll
            for (int n = 0; n < kSlots; ++n) {
                const double xn = x[n].v[v];
                const bool counts = xn == xn;
                const bool better = STAT == kMin ? xn < m : xn > m;
                m = (counts && (!has || better)) ? xn : m;
                has = has || counts;
            }
            y[v] = m;
        } else if constexpr (STAT == kVar) {
            double num = 0.0;
#pragma unroll
            for (int n = 0; n < kSlots; ++n) {
                const double xn = x[n].v[v];
                const double term = w[n] * xn;
                num = xn == xn ? num + term : num;
            }
            const double mean = num / sum;
            double m2 = 0.0;
#pragma unroll
            for (int n = 0; n < kSlots; ++n) {
                const double xn = x[n].v[v];
                const double d = xn - mean;
                const double term = w[n] * (d * d);
                m2 = xn == xn ? m2 + term : m2;
            }
            y[v] = m2 / sum;
        } else {
            const double half = 0.5 * sum;
            double least = 0.0;
            bool has = false;
#pragma unroll
            for (int j = 0; j < kSlots; ++j) {
                double below = 0.0;
#pragma unroll
                for (int q = 0; q < kSlots; ++q)    // (a NaN is <= nothing)
                    below = x[q].v[v] <= x[j].v[v] ? below + w[q] : below;
                qualify(x[j].v[v], below, half, least, has);
            }
            y[v] = has ? least : quiet_nan();
        }
    }
}

// MEDIAN of a row of any length behind its valid: the candidates in chunks
// of kSlots, the row streamed past each chunk.
template <typename XT, int VEC>
__device__ inline void median_rescan(const StatParams &p,
                                     const XT *__restrict__ X, int64_t s,
                                     int64_t e, const double (&valid)[VEC],
                                     double (&y)[VEC])
{
    double half[VEC], least[VEC];
    bool has[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        half[v] = 0.5 * valid[v];
        least[v] = 0.0;
        has[v] = false;
    }
    for (int64_t base = s; base < e; base += kSlots) {
        Pack<double, VEC> xc[kSlots], below[kSlots];
#pragma unroll
        for (int n = 0; n < kSlots; ++n) {
            const int64_t jj = base + n < e ? base + n : e - 1;
            xc[n] = gather<XT, VEC>(p, X, p.col[jj]);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (!(base + n < e))
                    xc[n].v[v] = quiet_nan();
                below[n].v[v] = 0.0;
            }
        }
        for (int64_t q = s; q < e; ++q) {
            const Pack<double, VEC> xq = gather<XT, VEC>(p, X, p.col[q]);
            const double sq = p.val[q];
#pragma unroll
            for (int n = 0; n < kSlots; ++n)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    below[n].v[v] = xq.v[v] <= xc[n].v[v]
                                        ? below[n].v[v] + sq
                                        : below[n].v[v];
        }
#pragma unroll
        for (int n = 0; n < kSlots; ++n)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                qualify(xc[n].v[v], below[n].v[v], half[v], least[v],
                        has[v]);
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        y[v] = has[v] ? least[v] : quiet_nan();
}

// The statistic of VEC neighbouring elements of row entries [s, e); X points
// at their columns of source cell 0.
template <int STAT, typename XT, int VEC>
__device__ inline Pack<double, VEC> row_stat(const StatParams &p,
                                             const XT *__restrict__ X,
                                             int64_t s, int64_t e)
{
    double valid[VEC], y[VEC];
    bool any[VEC];
    if (s >= e) {                   // an empty row: nothing counts
        Pack<double, VEC> none;
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            none.v[v] = quiet_nan();
        return none;
    }
    if (e - s <= kSlots) {
        slots_form<STAT, XT, VEC>(p, X, s, e, valid, any, y);
    } else {
        Walk t[VEC];
        walk<STAT, XT, VEC>(p, X, s, e, t);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            valid[v] = t[v].valid;
            any[v] = t[v].any;
            y[v] = t[v].acc;
        }
        if constexpr (STAT == kVar) {
            double mean[VEC], m2[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                mean[v] = t[v].acc / t[v].valid;
            spread<XT, VEC>(p, X, s, e, mean, m2);
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                y[v] = m2[v] / valid[v];
        }
        if constexpr (STAT == kMedian)
            median_rescan<XT, VEC>(p, X, s, e, valid, y);
    }
    Pack<double, VEC> out;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const bool ok = any[v] && valid[v] > p.thr;
        out.v[v] = (ok && y[v] == y[v]) ? y[v] : quiet_nan();
    }
    return out;
}

// ---------------------------------------------------------------------------
// rowlane: one lane per (row, column).  ROWS_FAST: thread -> row, blockIdx.y
// (and a loop) -> flat column; else the block is rows_per_block rows of
// cols_per_block columns, blockIdx.y (and a loop) the column tile.
// ---------------------------------------------------------------------------
template <int STAT, typename XT>
__device__ inline void lane_element(const StatParams &p, int64_t i,
                                    uint32_t kf)
{
    const uint32_t ki = static_cast<uint32_t>(p.k_inner);
    const uint32_t b = kf / ki;
    const uint32_t k = kf - b * ki;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) +
                               static_cast<int64_t>(b) * p.bsx +
                               static_cast<int64_t>(k);
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    const Pack<double, 1> y =
        row_stat<STAT, XT, 1>(p, X, p.rowptr[i], p.rowptr[i + 1]);
    p.Y[o] = y.v[0];
    if (p.mask_out)
        p.mask_out[o] = y.v[0] == y.v[0] ? 0 : 1;
}

template <int STAT, typename XT, bool ROWS_FAST>
__global__ __launch_bounds__(kBlock) void stat_rowlane(const StatParams p)
{
    if (gate_closed(p))
        return;
    const uint32_t K = static_cast<uint32_t>(p.K);
    if constexpr (ROWS_FAST) {
        const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r >= p.n_rows)
            return;
        for (uint32_t kf = blockIdx.y; kf < K; kf += gridDim.y)
            lane_element<STAT, XT>(p, p.row_begin + r, kf);
    } else {
        const uint32_t rl = threadIdx.x / p.cols_per_block;
        const uint32_t cl = threadIdx.x - rl * p.cols_per_block;
        const int64_t r = (int64_t)blockIdx.x * p.rows_per_block + rl;
        if (rl >= p.rows_per_block || r >= p.n_rows)
            return;
        // (64 bits: the last tile's first column plus the step may pass 2^32)
        const uint64_t step = (uint64_t)gridDim.y * p.cols_per_block;
        for (uint64_t kf = (uint64_t)blockIdx.y * p.cols_per_block + cl;
             kf < K; kf += step)
            lane_element<STAT, XT>(p, p.row_begin + r,
                                   static_cast<uint32_t>(kf));
    }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns; the work list and VEC are rowpass.h's.  The row is the
// same in every lane: the row pointers, the column indices and the weights
// are scalar loads and every loop over the row's entries is wave-uniform.
// ---------------------------------------------------------------------------
template <int STAT, typename XT, int VEC>
__global__ __launch_bounds__(kBlock) void stat_rowwave(const StatParams p,
                                                       const int64_t n_waves,
                                                       const int64_t chunks,
                                                       const int64_t per_xcd)
{
    if (gate_closed(p))
        return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = rowwave_place(per_xcd);
    if (w >= n_waves)
        return;
    const int64_t cb = w / p.n_rows;            // (batch, chunk), chunk-major
    const int64_t r = w - cb * p.n_rows;
    const int64_t b = cb / chunks;
    const int64_t chunk = cb - b * chunks;
    const int64_t k = chunk * (kWave * VEC) + (int64_t)lane * VEC;
    if (k >= p.k_inner)                         // (VEC = 2: k_inner is even)
        return;
    const int64_t i = p.row_begin + r;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) + b * p.bsx + k;
    const int64_t o = i * p.ldy + b * p.bsy + k;
    const Pack<double, VEC> y =
        row_stat<STAT, XT, VEC>(p, X, p.rowptr[i], p.rowptr[i + 1]);
    store_once<VEC>(p.Y + o, y);
    if (p.mask_out) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            p.mask_out[o + v] = y.v[v] == y.v[v] ? 0 : 1;
    }
}

template <int STAT, typename XT>
int launch_rowwave(const StatParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((stat_rowwave<STAT, XT, 2>), g.grid, dim3(kBlock),
                           0, stream, p, g.n_waves, g.chunks, g.per_xcd);
    else
        hipLaunchKernelGGL((stat_rowwave<STAT, XT, 1>), g.grid, dim3(kBlock),
                           0, stream, p, g.n_waves, g.chunks, g.per_xcd);
    return REMAP_OK;
}

template <int STAT, typename XT>
void launch_rowlane(StatParams &p, bool rows_fast, hipStream_t stream)
{
    if (rows_fast) {
        const dim3 grid(
            static_cast<unsigned>((p.n_rows + kBlock - 1) / kBlock),
            static_cast<unsigned>(p.K < kMaxGridY ? p.K : kMaxGridY));
        hipLaunchKernelGGL((stat_rowlane<STAT, XT, true>), grid, dim3(kBlock),
                           0, stream, p);
        return;
    }
    // tiles of equal width, at most a block wide
    const int64_t tiles = (p.K + kBlock - 1) / kBlock;
    p.cols_per_block = static_cast<uint32_t>((p.K + tiles - 1) / tiles);
    p.rows_per_block = kBlock / p.cols_per_block;
    const dim3 grid(
        static_cast<unsigned>((p.n_rows + p.rows_per_block - 1) /
                              p.rows_per_block),
        static_cast<unsigned>(tiles < kMaxGridY ? tiles : kMaxGridY));
    hipLaunchKernelGGL((stat_rowlane<STAT, XT, false>), grid, dim3(kBlock), 0,
                       stream, p);
}

template <int STAT, typename XT>
int launch(StatParams &p, const remap_apply_args *a, hipStream_t stream)
{
    if (a->k_inner >= kWave)
        return launch_rowwave<STAT, XT>(p, a->n_batch, stream);
    // short runs in several batches whose rows lie closer than its batches:
    // neighbouring lanes take neighbouring rows
    const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                           a->y_row_stride <= a->y_batch_stride;
    launch_rowlane<STAT, XT>(p, rows_fast, stream);
    return REMAP_OK;
}

template <int STAT>
int launch(StatParams &p, const remap_apply_args *a, hipStream_t stream)
{
    return a->x_dtype == REMAP_DTYPE_F64 ? launch<STAT, double>(p, a, stream)
                                         : launch<STAT, float>(p, a, stream);
}

// remap_apply_f64 with mode in REMAP_MODE_MIN .. REMAP_MODE_MEDIAN, behind
// its argument checks
inline int apply(const remap_apply_args *a, hipStream_t stream)
{
    StatParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    // (n_rows < 2^31: the blocks of either form fit grid.x)
    if (p.K >= (int64_t(1) << 31))
        return fail(REMAP_ERR_ARG,
                    "%s: %lld x %lld columns are more than one launch "
                    "serves", kName, (long long)a->n_batch,
                    (long long)a->k_inner);
    p.val = a->A.val;
    p.X = a->X;
    p.Y = a->Y;
    p.mask_out = a->mask_out;
    p.gate = a->gate;
    p.gate_value = a->gate_value;
    p.thr = a->threshold;
    p.cols_per_block = p.rows_per_block = 0;
    int rc = REMAP_OK;
    switch (a->mode) {
    case REMAP_MODE_MIN: rc = launch<kMin>(p, a, stream); break;
    case REMAP_MODE_MAX: rc = launch<kMax>(p, a, stream); break;
    case REMAP_MODE_VAR: rc = launch<kVar>(p, a, stream); break;
    default: rc = launch<kMedian>(p, a, stream); break;
    }
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace rowstat
}  // namespace remap

#endif  // REMAP_APPLY_ROWSTAT_H
