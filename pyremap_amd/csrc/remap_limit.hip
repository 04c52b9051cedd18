// remap_limit.hip -- the local-bounds limiter of the apply path: after an
// apply launch, every destination value is clamped to the bounds of the
// source values of its own row ("clip"; the first half of E3SM's clip and
// assured sum).
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.limiter.clip
// is the same statement in numpy).  For destination element (i, b, k) the
// row's stored entries are walked in CSR order, whatever their weights:
//   x = (double)X[cell(col), b, k]; a NaN is skipped; the first other value
//   sets lo = hi = x; then  if (x < lo) lo = x;  if (x > hi) hi = x;
//   no such value: y stays, lo = hi = y;
//   else y = y < lo ? lo : (y > hi ? hi : y)        (a NaN y stays NaN)
// Comparisons and copies only: nothing rounds, two runs give the same bytes,
// and -0.0 against +0.0 is decided by CSR order (the comparisons are strict).
//
// Two forms.  Runs of at least a wave's width (k_inner >= 64) take a wave per
// (row, chunk of columns), limit_rowwave below.  Everything else takes the
// first form: one lane per (row, column) as spmm_rowlane.h has it -- a lane
// walks its row UNR entries at a time, the UNR column indices fetched together
// (index clamped to the row's last entry: no load sits behind a branch), then
// the UNR source values together, then the comparisons in CSR order.  Which
// index runs fastest across the lanes is the launch's choice:
//   columns fastest  (n_a, K) and (Time, nCells, nVertLevels): the lanes of a
//                    wave read one source cell's contiguous run and write one
//                    row's -- whole lines both ways, the row's (rowptr, col)
//                    the same address in every lane (one line, broadcast);
//   rows fastest     (Time, nCells)-like layouts, runs shorter than
//                    kRowsFastRun in several batches: neighbouring lanes hold
//                    neighbouring rows of ONE column, so Y / lo / hi go out
//                    as whole lines and the source cells of neighbouring rows
//                    share theirs.
// No LDS, no atomics, no weights read.  The pass moves the apply's gather
// (without val) plus one read and one write of Y.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace {

using namespace rowpass;

constexpr char kName[] = "remap_limit_rows";
constexpr int kUnroll = 8;
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)

struct LimitParams {                // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const void *__restrict__ X;
    double *__restrict__ Y;
    double *__restrict__ lo;
    double *__restrict__ hi;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner
    int64_t ldx, bsx, ldy, bsy;
    int64_t src_outer;
    uint32_t src_fold;
    int64_t total;                  // n_rows * K
};

// element offset of source cell a in X
__device__ inline int64_t x_offset(const LimitParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// IT: the type the flat index is split in (rowpass::narrow_index)
template <typename XT, typename IT, bool ROWS_FAST>
__global__ __launch_bounds__(kBlock) void limit_rowlane(const LimitParams p)
{
    const int64_t gid64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid64 >= p.total)
        return;
    const IT gid = static_cast<IT>(gid64);
    IT r, kf;
    if constexpr (ROWS_FAST) {
        const IT n_rows = static_cast<IT>(p.n_rows);
        kf = gid / n_rows;
        r = gid - kf * n_rows;
    } else {
        const IT K = static_cast<IT>(p.K);
        r = gid / K;
        kf = gid - r * K;
    }
    const IT ki = static_cast<IT>(p.k_inner);
    const IT b = kf / ki;
    const IT k = kf - b * ki;
    const int64_t i = p.row_begin + static_cast<int64_t>(r);
    const XT *__restrict__ X = static_cast<const XT *>(p.X) +
                               static_cast<int64_t>(b) * p.bsx +
                               static_cast<int64_t>(k);
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    double y = p.Y[o];
    double lo = 0.0, hi = 0.0;
    bool has = false;
    for (int64_t base = s; base < e; base += kUnroll) {
        int32_t c[kUnroll];
        XT xs[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            xs[u] = X[x_offset(p, c[u])];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const double x = static_cast<double>(xs[u]);
            if (base + u < e && x == x) {
                if (!has) {
                    lo = x;
                    hi = x;
                    has = true;
                } else {
                    if (x < lo)
                        lo = x;
                    if (x > hi)
                        hi = x;
                }
            }
        }
    }
    if (has) {
        y = y < lo ? lo : (y > hi ? hi : y);
    } else {
        lo = y;
        hi = y;
    }
    p.Y[o] = y;
    if (p.lo)
        p.lo[o] = lo;
    if (p.hi)
        p.hi[o] = hi;
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns, as spmm_rowwave.h -- for runs of >= kWave columns; the
// work list and VEC are rowpass.h's.  The row is the same in every lane, so
// the row pointers and the column indices are scalar loads, the loop over the
// row's entries is wave-uniform and reads exactly the row's entries (no
// clamped duplicates), UNR source runs in flight at a time.  Y, lo and hi are
// touched once (load_once, store_once).
// ---------------------------------------------------------------------------
struct Bounds {
    double lo, hi;
    bool has;
};

__device__ inline void widen(Bounds &b, double x)
{
    if (x == x) {
        if (!b.has) {
            b.lo = x;
            b.hi = x;
            b.has = true;
        } else {
            if (x < b.lo)
                b.lo = x;
            if (x > b.hi)
                b.hi = x;
        }
    }
}

template <typename XT, int VEC>
__global__ __launch_bounds__(kBlock) void limit_rowwave(const LimitParams p,
                                                        const int64_t n_waves,
                                                        const int64_t chunks,
                                                        const int64_t per_xcd)
{
    constexpr int UNR = 4;
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
    using PY = Pack<double, VEC>;
    PY y = load_once<VEC>(p.Y + o);
    Bounds bd[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        bd[v] = {0.0, 0.0, false};
    int64_t j = s;
    for (; j + UNR <= e; j += UNR) {
        PX xs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            xs[u] = *reinterpret_cast<const PX *>(
                X + x_offset(p, p.col[j + u]));
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                widen(bd[v], static_cast<double>(xs[u].v[v]));
    }
    for (; j < e; ++j) {
        const PX x = *reinterpret_cast<const PX *>(
            X + x_offset(p, p.col[j]));
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            widen(bd[v], static_cast<double>(x.v[v]));
    }
    PY lo, hi;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const double yv = y.v[v];
        if (bd[v].has) {
            lo.v[v] = bd[v].lo;
            hi.v[v] = bd[v].hi;
            y.v[v] = yv < bd[v].lo ? bd[v].lo : (yv > bd[v].hi ? bd[v].hi
                                                               : yv);
        } else {
            lo.v[v] = yv;
            hi.v[v] = yv;
        }
    }
    store_once<VEC>(p.Y + o, y);
    if (p.lo)
        store_once<VEC>(p.lo + o, lo);
    if (p.hi)
        store_once<VEC>(p.hi + o, hi);
}

template <typename XT>
int launch_rowwave(const LimitParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16) && aligned_to(p.lo, 16) &&
                      aligned_to(p.hi, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((limit_rowwave<XT, 2>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    else
        hipLaunchKernelGGL((limit_rowwave<XT, 1>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    return REMAP_OK;
}

template <typename XT, typename IT>
void launch_limit(const LimitParams &p, bool rows_fast, hipStream_t stream)
{
    if (rows_fast)
        hipLaunchKernelGGL((limit_rowlane<XT, IT, true>),
                           rowlane_grid(p.total), dim3(kBlock), 0, stream, p);
    else
        hipLaunchKernelGGL((limit_rowlane<XT, IT, false>),
                           rowlane_grid(p.total), dim3(kBlock), 0, stream, p);
}

}  // namespace

int limit_rows(const remap_limit_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    LimitParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a->A.nnz > 0 && !p.col) || !a->X || !a->Y)
        return fail(REMAP_ERR_ARG, "%s: NULL rowptr, col, X or Y", kName);
    p.X = a->X;
    p.Y = a->Y;
    p.lo = a->lo;
    p.hi = a->hi;
    // short runs in several batches whose rows lie closer than its batches:
    // neighbouring lanes take neighbouring rows
    const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                           a->y_row_stride <= a->y_batch_stride;
    const bool narrow = narrow_index(p);
    if (a->k_inner >= kWave) {
        // runs of a wave's width and more: a wave per (row, chunk)
        const int rc = a->x_dtype == REMAP_DTYPE_F64
                           ? launch_rowwave<double>(p, a->n_batch, stream)
                           : launch_rowwave<float>(p, a->n_batch, stream);
        if (rc != REMAP_OK)
            return rc;
    } else if (a->x_dtype == REMAP_DTYPE_F64) {
        if (narrow)
            launch_limit<double, uint32_t>(p, rows_fast, stream);
        else
            launch_limit<double, int64_t>(p, rows_fast, stream);
    } else {
        if (narrow)
            launch_limit<float, uint32_t>(p, rows_fast, stream);
        else
            launch_limit<float, int64_t>(p, rows_fast, stream);
    }
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_limit_rows(const struct remap_limit_args *args, void *stream)
{
    return remap::limit_rows(args, static_cast<hipStream_t>(stream));
}

#ifdef REMAP_ROWPASS_WIDE_INDEX
// the mark of the tests' wide-index build (rowpass::narrow_index); the
// product does not define it and include/remap_hip.h does not declare it
REMAP_API int remap_rowpass_wide_index(void)
{
    return 1;
}
#endif

}  // extern "C"
