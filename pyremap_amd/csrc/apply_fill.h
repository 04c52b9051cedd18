// apply_fill.h -- REMAP_MODE_FILL_BEST and REMAP_MODE_FILL_MEAN of
// remap_apply_f64: one pass of a creeping fill (compass' extrap_woa, CDO's
// fillmiss / setmisstonn, ESMF's --extrap_method creep).  A is the neighbour
// matrix of ONE grid (square; pyremap_amd.fill.neighbour_graph), X a field on
// that grid and Y the same field with every missing element that has a valid
// neighbour filled: by the value of the neighbour with the largest weight
// (FILL_BEST: labels, "nearest valid") or by the weighted mean of the valid
// neighbours (FILL_MEAN).  What is valid is kept.  The driver
// (engine.fill_tensor) repeats the pass between two buffers until nothing
// fillable is left.  Included by remap_spmm.hip; stands on rowpass.h.
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.fill.fill_pass
// is the same statement in numpy).
// For element (i, b, k), with x_i = (double) X[cell(i), b, k]:
//   x_i is no NaN: y = x_i (a copy: float32 widens exactly), mask 0
//   x_i is NaN: the entries j of row i are walked in CSR order (ascending col)
//     x_j = (double) X[cell(col_j), b, k]
//     an entry counts iff x_j is no NaN; +-inf are values like any other
//   FILL_BEST: the first counted entry sets best = S_j, v = x_j; a later one
//     replaces both iff S_j > best (strict: the lowest col wins a tie, a NaN
//     S_j never replaces)
//     y = some entry counts ? v : NaN
//   FILL_MEAN: num and den start at +0.0; for every counted entry, in CSR order,
//     num = num + (S_j * x_j), den = den + S_j, the product rounded, then each
//     sum; no FMA contraction
//     y = den > threshold ? num / den : NaN, one IEEE division
// Every NaN written is 0x7ff8000000000000; mask_out, where given, gets 1 where
// NaN was written and 0 elsewhere.  Only X is read: no value written by this
// launch is looked at.
//
// With non-negative weights FILL_MEAN at a missing element is byte for byte
// REMAP_MODE_MASKED of the same matrix, field and threshold (that mode's
// S_j * +0.0 terms never change a sum that starts at +0.0), so the whole pass
// is where(isnan(X), masked apply, X) in one launch and one read of X.
//
// Most elements are valid, so the pass is mostly a copy.  Two forms, as
// apply_laf.h has them:
//   rowlane  one lane per (row, column), for runs shorter than a wave; a lane
//            whose own element is valid stores it and is done;
//   rowwave  one wave per (row, chunk of kWave * VEC columns) for
//            k_inner >= kWave: the wave reads its own chunk, and where the
//            ballot of "is NaN" is empty (a wave-uniform branch) it never
//            touches the row: no row pointer, no column index, no gather.
//            Inside the walk col and val are wave-uniform scalar loads and
//            the lanes whose own element is valid do not take part.  Y leaves
//            once through store_once.
// Registers and global memory only: no workgroup memory, no read-modify-write
// of memory, every element written once by the lane that owns it.
#ifndef REMAP_APPLY_FILL_H
#define REMAP_APPLY_FILL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace fill {

using namespace rowpass;

constexpr char kName[] = "remap_apply_f64";
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)
constexpr unsigned kMaxGridY = 65535;

struct FillParams {                 // (rowpass.h: P)
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

__device__ inline bool gate_closed(const FillParams &p)
{
    return p.gate != nullptr && *p.gate != p.gate_value;
}

__device__ inline double quiet_nan()
{
    return __longlong_as_double(0x7ff8000000000000LL);
}

// element offset of cell a in X (the element's own cell and its neighbours)
__device__ inline int64_t x_offset(const FillParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// What a missing element keeps while its row is walked.  MEAN: a = num,
// b = den.  BEST: a = best, b = v, has = some entry counted.
struct Walk {
    double a, b;
    bool has;
};

__device__ inline void clear(Walk &t)
{
    t.a = 0.0;
    t.b = 0.0;
    t.has = false;
}

template <bool MEAN>
__device__ inline void count(Walk &t, double x, double s)
{
    if (!(x == x))
        return;
    if constexpr (MEAN) {
        const double prod = s * x;
        t.a = t.a + prod;
        t.b = t.b + s;
    } else {
        const bool take = !t.has || s > t.a;
        t.a = take ? s : t.a;
        t.b = take ? x : t.b;
    }
    t.has = true;
}

template <bool MEAN>
__device__ inline double result(const Walk &t, double thr)
{
    if constexpr (MEAN) {
        const double q = t.a / t.b;
        return (t.b > thr && q == q) ? q : quiet_nan();
    } else {
        return t.has ? t.b : quiet_nan();
    }
}

// ---------------------------------------------------------------------------
// rowlane: one lane per (row, column).  ROWS_FAST: thread -> row, blockIdx.y
// (and a loop) -> flat column; else the block is rows_per_block rows of
// cols_per_block columns, blockIdx.y (and a loop) the column tile.
// ---------------------------------------------------------------------------
template <typename XT, bool MEAN>
__device__ inline void lane_element(const FillParams &p, int64_t i,
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
    double y = static_cast<double>(X[x_offset(p, static_cast<int32_t>(i))]);
    if (!(y == y)) {
        const int64_t s = p.rowptr[i];
        const int64_t e = p.rowptr[i + 1];
        Walk t;
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
                    count<MEAN>(t, static_cast<double>(xs[u]), w[u]);
        }
        y = result<MEAN>(t, p.thr);
    }
    p.Y[o] = y;
    if (p.mask_out)
        p.mask_out[o] = y == y ? 0 : 1;
}

template <typename XT, bool MEAN, bool ROWS_FAST>
__global__ __launch_bounds__(kBlock) void fill_rowlane(const FillParams p)
{
    if (gate_closed(p))
        return;
    const uint32_t K = static_cast<uint32_t>(p.K);
    if constexpr (ROWS_FAST) {
        const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r >= p.n_rows)
            return;
        for (uint32_t kf = blockIdx.y; kf < K; kf += gridDim.y)
            lane_element<XT, MEAN>(p, p.row_begin + r, kf);
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
            lane_element<XT, MEAN>(p, p.row_begin + r,
                                   static_cast<uint32_t>(kf));
    }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns; the work list and VEC are rowpass.h's.  The row is the
// same in every lane, so whether any lane of the wave misses its element is
// one ballot, and a wave without a missing element is a copy of its chunk.
// ---------------------------------------------------------------------------
template <typename XT, bool MEAN, int VEC>
__global__ __launch_bounds__(kBlock) void fill_rowwave(const FillParams p,
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
    using PX = Pack<XT, VEC>;
    const PX own = *reinterpret_cast<const PX *>(
        X + x_offset(p, static_cast<int32_t>(i)));
    Pack<double, VEC> y;
    bool miss[VEC];
    bool any = false;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        y.v[v] = static_cast<double>(own.v[v]);
        miss[v] = !(y.v[v] == y.v[v]);
        any = any || miss[v];
    }
    if (__ballot(any) != 0) {                   // (wave-uniform)
        if (any) {
            const int64_t s = p.rowptr[i];
            const int64_t e = p.rowptr[i + 1];
            Walk t[VEC];
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
                        count<MEAN>(t[v], static_cast<double>(xs[u].v[v]),
                                    ws[u]);
            }
            for (; j < e; ++j) {
                const PX x = *reinterpret_cast<const PX *>(
                    X + x_offset(p, p.col[j]));
                const double ws = p.val[j];
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    count<MEAN>(t[v], static_cast<double>(x.v[v]), ws);
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                y.v[v] = miss[v] ? result<MEAN>(t[v], p.thr) : y.v[v];
        }
    }
    store_once<VEC>(p.Y + o, y);
    if (p.mask_out) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            p.mask_out[o + v] = y.v[v] == y.v[v] ? 0 : 1;
    }
}

template <typename XT, bool MEAN>
int launch_rowwave(const FillParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((fill_rowwave<XT, MEAN, 2>), g.grid, dim3(kBlock),
                           0, stream, p, g.n_waves, g.chunks, g.per_xcd);
    else
        hipLaunchKernelGGL((fill_rowwave<XT, MEAN, 1>), g.grid, dim3(kBlock),
                           0, stream, p, g.n_waves, g.chunks, g.per_xcd);
    return REMAP_OK;
}

template <typename XT, bool MEAN>
void launch_rowlane(FillParams &p, bool rows_fast, hipStream_t stream)
{
    if (rows_fast) {
        const dim3 grid(
            static_cast<unsigned>((p.n_rows + kBlock - 1) / kBlock),
            static_cast<unsigned>(p.K < kMaxGridY ? p.K : kMaxGridY));
        hipLaunchKernelGGL((fill_rowlane<XT, MEAN, true>), grid, dim3(kBlock),
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
    hipLaunchKernelGGL((fill_rowlane<XT, MEAN, false>), grid, dim3(kBlock), 0,
                       stream, p);
}

template <typename XT, bool MEAN>
int launch(FillParams &p, const remap_apply_args *a, hipStream_t stream)
{
    if (a->k_inner >= kWave)
        return launch_rowwave<XT, MEAN>(p, a->n_batch, stream);
    // short runs in several batches whose rows lie closer than its batches:
    // neighbouring lanes take neighbouring rows
    const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                           a->y_row_stride <= a->y_batch_stride;
    launch_rowlane<XT, MEAN>(p, rows_fast, stream);
    return REMAP_OK;
}

// remap_apply_f64 with mode == REMAP_MODE_FILL_BEST or _FILL_MEAN, behind its
// argument checks
inline int apply(const remap_apply_args *a, hipStream_t stream)
{
    if (a->A.n_rows != a->A.n_cols)
        return fail(REMAP_ERR_ARG,
                    "%s: a fill walks the neighbour matrix of ONE grid, and "
                    "a (%lld, %lld) matrix is not square", kName,
                    (long long)a->A.n_rows, (long long)a->A.n_cols);
    if (static_cast<const void *>(a->Y) == a->X)
        return fail(REMAP_ERR_ARG,
                    "%s: a fill reads the neighbours of an element from X "
                    "while it writes Y: Y must not be X", kName);
    FillParams p;
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
    const bool mean = a->mode == REMAP_MODE_FILL_MEAN;
    const int rc =
        f64 ? (mean ? launch<double, true>(p, a, stream)
                    : launch<double, false>(p, a, stream))
            : (mean ? launch<float, true>(p, a, stream)
                    : launch<float, false>(p, a, stream));
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace fill
}  // namespace remap

#endif  // REMAP_APPLY_FILL_H
