// apply_laf.h -- REMAP_MODE_LAF of remap_apply_f64: largest area fraction
// (CDO's remaplaf) for fields whose values are labels -- region and basin
// ids, land-cover classes, 0/1/2 flags.  Every destination element takes the
// source value whose weights in its row add up to the most, so only values
// the row's source cells hold come out.  Included by remap_spmm.hip; stands
// on rowpass.h.
//
// Definition (include/remap_hip.h has the contract;
// pyremap_amd.laf.largest_fraction is the same statement in numpy).  For
// destination element (i, b, k) the entries j of row i are walked in CSR
// order, which is ascending source cell:
//   x = (double) X[cell(col_j), b, k]
//   a NaN x is skipped; +-inf are values like any other
//   the entry's class is the first earlier counted value of the row with
//   value == x (so -0.0 and +0.0 are one class, and the class keeps the
//   bits of its first member); no such value: a new class, w_c = +0.0
//   w_c = w_c + S_j;   valid = valid + S_j
//   (valid starts at +0.0; every sum rounded, in CSR order)
//   winner: the classes in order of first appearance; the first one sets
//   best; a later one replaces it iff w_c > best
//   (strict: the first seen wins a tie; a NaN sum never replaces)
//   y = (a class exists && valid > threshold) ? the winner's value : NaN
// Sums of the row's weights and comparisons only: no product, no division,
// nothing that could be contracted, so two runs and the two forms below give
// the same bytes.  Every NaN written is 0x7ff8000000000000.
//
// Class list.  An element keeps kSlots (value, sum) pairs in registers: the
// loops over them are unrolled and every access is a compare-and-select
// under a compile-time index, so nothing is indexed at run time and nothing
// goes to scratch.  A stencil inside or on the edge of a region holds 1 to 3
// classes.  An element whose row holds more classes than slots is redone in
// the same launch by a rescan that needs no table: entry j is a candidate iff
// no earlier counted entry has its value, and its sum is taken over the later
// equal entries in CSR order -- the adds, their order and the order of the
// candidates are the table's, so the bytes are.
//
// Two forms, as remap_limit.hip has them:
//   rowlane  one lane per (row, column), for runs shorter than a wave.  Rows
//            come from the block index, columns from the lane, further column
//            tiles from grid.y and a loop: 32-bit divisions only and one code
//            path for every size.  Columns run fastest across the lanes, or
//            rows do for runs shorter than kRowsFastRun in several batches;
//   rowwave  one wave per (row, chunk of kWave * VEC columns) for
//            k_inner >= kWave: col and val are wave-uniform scalar loads, Y
//            leaves once through store_once.
// Registers and global memory only: no workgroup memory, no read-modify-write
// of memory, every element written once by the lane that owns it.
#ifndef REMAP_APPLY_LAF_H
#define REMAP_APPLY_LAF_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace laf {

using namespace rowpass;

constexpr char kName[] = "remap_apply_f64";
constexpr int kSlots = 4;             // classes an element keeps in registers
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)
constexpr unsigned kMaxGridY = 65535;

struct LafParams {                  // (rowpass.h: P)
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

__device__ inline bool gate_closed(const LafParams &p)
{
    return p.gate != nullptr && *p.gate != p.gate_value;
}

__device__ inline double quiet_nan()
{
    return __longlong_as_double(0x7ff8000000000000LL);
}

// element offset of source cell a in X
__device__ inline int64_t x_offset(const LafParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// The classes of one element: value and sum of the first kSlots classes in
// order of first appearance.  (Arrays under unrolled loops: every index is a
// constant once unrolled.)
struct Classes {
    double v[kSlots], w[kSlots];
    double valid;
    int n;
    bool over;      // the row holds more than kSlots classes
};

__device__ inline void clear(Classes &t)
{
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        t.v[c] = 0.0;
        t.w[c] = 0.0;
    }
    t.valid = 0.0;
    t.n = 0;
    t.over = false;
}

__device__ inline void count(Classes &t, double x, double s)
{
    if (!(x == x))
        return;
    t.valid = t.valid + s;
    bool hit = false;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const bool m = !hit && c < t.n && x == t.v[c];
        const double sum = t.w[c] + s;
        t.w[c] = m ? sum : t.w[c];
        hit = hit || m;
    }
    const bool fresh = !hit && t.n < kSlots;
    const double first = 0.0 + s;
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const bool m = fresh && c == t.n;
        t.v[c] = m ? x : t.v[c];
        t.w[c] = m ? first : t.w[c];
    }
    t.n += fresh ? 1 : 0;
    t.over = t.over || (!hit && !fresh);
}

// the winner of the table: the value, or NaN where the element is masked
__device__ inline double winner(const Classes &t, double thr)
{
    double best = t.w[0], value = t.v[0];
#pragma unroll
    for (int c = 1; c < kSlots; ++c) {
        const bool m = c < t.n && t.w[c] > best;
        best = m ? t.w[c] : best;
        value = m ? t.v[c] : value;
    }
    return (t.n > 0 && t.valid > thr) ? value : quiet_nan();
}

// The same without a table, for an element whose row holds more classes
// than slots.  X points at the element's column of source cell 0.
template <typename XT>
__device__ inline double rescan(const LafParams &p, const XT *__restrict__ X,
                                int64_t s, int64_t e)
{
    double valid = 0.0, best = 0.0, value = 0.0;
    bool has = false;
    for (int64_t j = s; j < e; ++j) {
        const double x = static_cast<double>(X[x_offset(p, p.col[j])]);
        if (!(x == x))
            continue;
        valid = valid + p.val[j];
        bool seen = false;
        for (int64_t q = s; q < j; ++q)
            seen = seen ||
                   static_cast<double>(X[x_offset(p, p.col[q])]) == x;
        if (seen)
            continue;
        double w = 0.0 + p.val[j];
        for (int64_t q = j + 1; q < e; ++q)
            if (static_cast<double>(X[x_offset(p, p.col[q])]) == x)
                w = w + p.val[q];
        if (!has || w > best) {
            best = w;
            value = x;
        }
        has = true;
    }
    return (has && valid > p.thr) ? value : quiet_nan();
}

// ---------------------------------------------------------------------------
// rowlane: one lane per (row, column).  ROWS_FAST: thread -> row, blockIdx.y
// (and a loop) -> flat column; else the block is rows_per_block rows of
// cols_per_block columns, blockIdx.y (and a loop) the column tile.
// ---------------------------------------------------------------------------
template <typename XT>
__device__ inline void lane_element(const LafParams &p, int64_t i,
                                    uint32_t kf)
{
    constexpr int UNR = 4;
    const uint32_t ki = static_cast<uint32_t>(p.k_inner);
    const uint32_t b = kf / ki;
    const uint32_t k = kf - b * ki;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) +
                               static_cast<int64_t>(b) * p.bsx +
                               static_cast<int64_t>(k);
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    Classes t;
    clear(t);
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double w[UNR];
        XT xs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            w[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            xs[u] = X[x_offset(p, c[u])];
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e)
                count(t, static_cast<double>(xs[u]), w[u]);
    }
    double y = winner(t, p.thr);
    if (t.over)
        y = rescan<XT>(p, X, s, e);
    p.Y[o] = y;
    if (p.mask_out)
        p.mask_out[o] = y == y ? 0 : 1;
}

template <typename XT, bool ROWS_FAST>
__global__ __launch_bounds__(kBlock) void laf_rowlane(const LafParams p)
{
    if (gate_closed(p))
        return;
    const uint32_t K = static_cast<uint32_t>(p.K);
    if constexpr (ROWS_FAST) {
        const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r >= p.n_rows)
            return;
        for (uint32_t kf = blockIdx.y; kf < K; kf += gridDim.y)
            lane_element<XT>(p, p.row_begin + r, kf);
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
            lane_element<XT>(p, p.row_begin + r, static_cast<uint32_t>(kf));
    }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns; the work list and VEC are rowpass.h's.  The row is the
// same in every lane: the row pointers, the column indices and the weights
// are scalar loads and the loop over the row's entries is wave-uniform.
// ---------------------------------------------------------------------------
template <typename XT, int VEC>
__global__ __launch_bounds__(kBlock) void laf_rowwave(const LafParams p,
                                                      const int64_t n_waves,
                                                      const int64_t chunks,
                                                      const int64_t per_xcd)
{
    constexpr int UNR = 4;
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
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    using PX = Pack<XT, VEC>;
    Classes t[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        clear(t[v]);
    int64_t j = s;
    for (; j + UNR <= e; j += UNR) {
        PX xs[UNR];
        double ws[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            xs[u] = *reinterpret_cast<const PX *>(
                X + x_offset(p, p.col[j + u]));
            ws[u] = p.val[j + u];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                count(t[v], static_cast<double>(xs[u].v[v]), ws[u]);
    }
    for (; j < e; ++j) {
        const PX x = *reinterpret_cast<const PX *>(
            X + x_offset(p, p.col[j]));
        const double ws = p.val[j];
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            count(t[v], static_cast<double>(x.v[v]), ws);
    }
    Pack<double, VEC> y;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        y.v[v] = winner(t[v], p.thr);
        if (t[v].over)
            y.v[v] = rescan<XT>(p, X + v, s, e);
    }
    store_once<VEC>(p.Y + o, y);
    if (p.mask_out) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            p.mask_out[o + v] = y.v[v] == y.v[v] ? 0 : 1;
    }
}

template <typename XT>
int launch_rowwave(const LafParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((laf_rowwave<XT, 2>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    else
        hipLaunchKernelGGL((laf_rowwave<XT, 1>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    return REMAP_OK;
}

template <typename XT>
void launch_rowlane(LafParams &p, bool rows_fast, hipStream_t stream)
{
    if (rows_fast) {
        const dim3 grid(
            static_cast<unsigned>((p.n_rows + kBlock - 1) / kBlock),
            static_cast<unsigned>(p.K < kMaxGridY ? p.K : kMaxGridY));
        hipLaunchKernelGGL((laf_rowlane<XT, true>), grid, dim3(kBlock), 0,
                           stream, p);
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
    hipLaunchKernelGGL((laf_rowlane<XT, false>), grid, dim3(kBlock), 0,
                       stream, p);
}

// remap_apply_f64 with mode == REMAP_MODE_LAF, behind its argument checks
inline int apply(const remap_apply_args *a, hipStream_t stream)
{
    LafParams p;
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
    const bool f64 = a->x_dtype == REMAP_DTYPE_F64;
    if (a->k_inner >= kWave) {
        const int rc = f64 ? launch_rowwave<double>(p, a->n_batch, stream)
                           : launch_rowwave<float>(p, a->n_batch, stream);
        if (rc != REMAP_OK)
            return rc;
    } else {
        // short runs in several batches whose rows lie closer than its
        // batches: neighbouring lanes take neighbouring rows
        const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                               a->y_row_stride <= a->y_batch_stride;
        if (f64)
            launch_rowlane<double>(p, rows_fast, stream);
        else
            launch_rowlane<float>(p, rows_fast, stream);
    }
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace laf
}  // namespace remap

#endif  // REMAP_APPLY_LAF_H
