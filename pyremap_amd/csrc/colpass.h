// colpass.h -- the column pass: what the row passes that first reduce every
// entry's source COLUMN with a companion array and then enter the masked,
// renormalised sum share (remap_levels.hip: the column at a level, companion
// the level coordinate; remap_layers.hip: the column over a depth range,
// companion the layer thicknesses).  The parameters, the lane walk, the
// launch table, the dtype dispatch and the entry points' checks, once; a
// pass states what differs as a policy type Op:
//   Op::kBatches, Op::kBatchesShared   batches a lane serves (batch-major),
//                                      and where one walk of the companion
//                                      serves them all
//   Op::query(p, l)                    what output l asks for, read once
//   Op::entry<XT, CT, NW>(x, bsx, nw, c, n_levels, query, mode, a, sums)
//                                      one source column of weight a: the
//                                      NW batches x, x + bsx, .. of which nw
//                                      exist, against the ONE companion
//                                      column c; adds into sums[0 .. nw)
//
// One form: a lane per (row, b, l), l fastest, so neighbouring lanes walk the
// same source columns and share their lines; with several batches whose rows
// lie closer than the batches ((Time, nCells, nVertLevels)) the lanes run
// over (row, l) of ONE batch group and a lane serves kBatches batches with
// one fetch of the row's indices and weights, as sgs_rowlane does --
// kBatchesShared with a time-invariant companion (batch stride 0), whose one
// walk serves them all.  No LDS, no atomics.
#ifndef REMAP_COLPASS_H
#define REMAP_COLPASS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace colpass {

using namespace rowpass;

constexpr int kUnroll = 4;          // (col, S) pairs fetched together

struct ColumnParams {               // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    const void *__restrict__ C;     // the companion: Z, H
    const double *__restrict__ Q;   // what the outputs ask for: T, bounds
    double *__restrict__ Y;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner, k_inner = L, R
    int64_t ldx, bsx, ldy, bsy;
    int64_t ldc, bsc;               // C: row and batch stride (0: broadcast)
    int64_t src_outer, c_outer;
    uint32_t src_fold;
    int32_t n_levels;
    int32_t mode;                   // the pass's own (layers: the integral)
    int64_t total;                  // n_rows * K
    double thr;
};

// element offsets of source cell a in X and in C, from one split
__device__ inline void cell_offsets(const ColumnParams &p, int32_t a,
                                    int64_t &ox, int64_t &oc)
{
    int64_t o[2];
    rowpass::cell_offsets(p, a, {p.ldx, p.ldc}, {p.src_outer, p.c_outer}, o);
    ox = o[0];
    oc = o[1];
}

struct Sums {
    double num, valid;
};

// (a quotient that is itself a NaN -- inf / inf, a NaN weight -- leaves as
// the same quiet NaN as a masked element: the bits of Y are defined)
__device__ inline double finish(const Sums &s, double thr)
{
    const double q = s.num / s.valid;
    return (s.valid > thr && q == q) ? q : __builtin_nan("");
}

// IT: the type the flat index is split in (rowpass::narrow_index).
// NB > 1 (batch-major): the lanes run over (row, l) of ONE batch group, l
// fastest, and a lane serves NB batches of its (row, l); a batch past the
// last is neither read nor stored.  NB == 1: the lanes run over (row, b, l).
// SHARED (batch-major only): the companion's batch stride is 0, one
// entry<NB> serves the batches of the lane.
// (Op::entry adds into the sums as it goes and is always_inline: the shared
// forms stand at 127 to 129 VGPRs, the edge of 4 waves per SIMD, and values
// handed back for the kernel to add would have to live past it.)
template <typename Op, typename XT, typename CT, typename IT, int NB,
          bool SHARED>
__global__ __launch_bounds__(kBlock) void column_rowlane(
    const ColumnParams p, const int64_t n_batch)
{
    constexpr bool BATCH_MAJOR = NB > 1;
    const int64_t gid64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid64 >= p.total)
        return;
    const IT gid = static_cast<IT>(gid64);
    const IT ki = static_cast<IT>(p.k_inner);
    IT r, b, l;
    if constexpr (BATCH_MAJOR) {
        const IT per = static_cast<IT>(p.n_rows) * ki;
        const IT bg = gid / per;
        const IT rem = gid - bg * per;
        r = rem / ki;
        l = rem - r * ki;
        b = bg * NB;
    } else {
        const IT K = static_cast<IT>(p.K);
        r = gid / K;
        const IT kf = gid - r * K;
        b = kf / ki;
        l = kf - b * ki;
    }
    const int64_t i = p.row_begin + static_cast<int64_t>(r);
    const auto query = Op::query(p, static_cast<int64_t>(l));
    const bool mode = p.mode != 0;
    const int64_t b0 = static_cast<int64_t>(b);
    const XT *__restrict__ X = static_cast<const XT *>(p.X) + b0 * p.bsx;
    const CT *__restrict__ C = static_cast<const CT *>(p.C) + b0 * p.bsc;
    // the batches of the lane that exist (wave-uniform but for the lanes of
    // two batch groups in one wave)
    const int nb = n_batch - b0 < NB ? static_cast<int>(n_batch - b0) : NB;
    const int64_t o = i * p.ldy + b0 * p.bsy + static_cast<int64_t>(l);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    Sums sum[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
        sum[n] = {0.0, 0.0};
    for (int64_t base = s; base < e; base += kUnroll) {
        int32_t c[kUnroll];
        double a[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            a[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (base + u >= e)
                break;
            int64_t ox, oc;
            cell_offsets(p, c[u], ox, oc);
            if constexpr (SHARED) {
                Op::template entry<XT, CT, NB>(X + ox, p.bsx, nb, C + oc,
                                               p.n_levels, query, mode, a[u],
                                               sum);
            } else {
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    if (n < nb)
                        Op::template entry<XT, CT, 1>(
                            X + n * p.bsx + ox, 0, 1, C + n * p.bsc + oc,
                            p.n_levels, query, mode, a[u], sum + n);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (n < nb)
            __builtin_nontemporal_store(finish(sum[n], p.thr),
                                        p.Y + o + n * p.bsy);
}

template <typename Op, typename XT, typename CT>
void launch_columns(const ColumnParams &p, int64_t n_batch, bool batch_major,
                    hipStream_t stream)
{
    // batch-major: a lane per kBatches batches; kBatchesShared of them where
    // one walk of the companion serves them all and there are more than
    // kBatches
    constexpr int kBatches = Op::kBatches;
    constexpr int kBatchesShared = Op::kBatchesShared;
    const bool shared = batch_major && p.bsc == 0;
    const int nb = !batch_major ? 1
                   : shared && n_batch > kBatches ? kBatchesShared : kBatches;
    ColumnParams q = p;
    if (batch_major)
        q.total = (n_batch + nb - 1) / nb * p.n_rows * p.k_inner;
    const dim3 grid = rowlane_grid(q.total);
    const bool narrow = narrow_index(p);
#define REMAP_COLUMNS_LAUNCH(IT, NB, SHARED)                                \
    hipLaunchKernelGGL((column_rowlane<Op, XT, CT, IT, NB, SHARED>), grid,  \
                       dim3(kBlock), 0, stream, q, n_batch)
    if (narrow && nb == kBatchesShared)
        REMAP_COLUMNS_LAUNCH(uint32_t, kBatchesShared, true);
    else if (narrow && shared)
        REMAP_COLUMNS_LAUNCH(uint32_t, kBatches, true);
    else if (narrow && batch_major)
        REMAP_COLUMNS_LAUNCH(uint32_t, kBatches, false);
    else if (narrow)
        REMAP_COLUMNS_LAUNCH(uint32_t, 1, false);
    else if (nb == kBatchesShared)
        REMAP_COLUMNS_LAUNCH(int64_t, kBatchesShared, true);
    else if (shared)
        REMAP_COLUMNS_LAUNCH(int64_t, kBatches, true);
    else if (batch_major)
        REMAP_COLUMNS_LAUNCH(int64_t, kBatches, false);
    else
        REMAP_COLUMNS_LAUNCH(int64_t, 1, false);
#undef REMAP_COLUMNS_LAUNCH
}

// What an entry point hands check_columns and apply_columns of its argument
// struct: the companion array under the pass's name for it, and what the
// outputs ask for.
struct Companion {
    const char *name;               // "z": z_dtype, z_outer_stride
    const char *arrays;             // "Z, T": the NULL check's message
    const void *C;
    int dtype;
    int64_t row_stride, batch_stride, outer_stride;
    const double *Q;
};

// The checks of remap_levels_args and remap_layers_args around those of
// rowpass::check_args, under the entry point's name `fn`; fills `p` but for
// its mode.  `mode_ok()`: the pass's own check, REMAP_OK or its fail(), in
// its place among the others.  `empty`: the arguments are fine and there is
// nothing to do.
template <typename Args, typename ModeOk>
int check_columns(const char *fn, const Args &a, const Companion &c,
                  ModeOk mode_ok, ColumnParams &p, bool &empty)
{
    if (a.n_levels < 1 || a.n_levels > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_levels %lld: expected >= 1", fn,
                    (long long)a.n_levels);
    if (c.dtype != REMAP_DTYPE_F64 && c.dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "%s: %s_dtype %d is no REMAP_DTYPE_*", fn,
                    c.name, c.dtype);
    const int mode_checked = mode_ok();
    if (mode_checked != REMAP_OK)
        return mode_checked;
    if (c.row_stride < 0 || c.batch_stride < 0)
        return fail(REMAP_ERR_ARG, "%s: a negative stride", fn);
    if (a.x_src_fold != 0 && c.outer_stride < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: x_src_fold = %lld with a negative %s_outer_stride",
                    fn, (long long)a.x_src_fold, c.name);
    const int checked = check_args(fn, a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a.A.nnz > 0 && (!p.col || !a.A.val)) || !a.X || !c.C ||
        !c.Q || !a.Y)
        return fail(REMAP_ERR_ARG, "%s: NULL rowptr, col, val, X, %s or Y",
                    fn, c.arrays);
    p.val = a.A.val;
    p.X = a.X;
    p.C = c.C;
    p.Q = c.Q;
    p.Y = a.Y;
    p.ldc = c.row_stride;
    p.bsc = c.batch_stride;
    p.c_outer = c.outer_stride;
    p.n_levels = static_cast<int32_t>(a.n_levels);
    p.thr = a.threshold;
    return REMAP_OK;
}

// The launch behind an entry point: Op's kernels for the dtypes of X and of
// the companion.
template <typename Op, typename Args>
int apply_columns(const Args &a, const Companion &c, const ColumnParams &p,
                  hipStream_t stream)
{
    // several batches whose rows lie closer than the batches: the lanes run
    // over the rows and outputs of one batch group
    const bool batch_major = a.n_batch > 1 &&
                             a.y_row_stride <= a.y_batch_stride;
    const bool x64 = a.x_dtype == REMAP_DTYPE_F64;
    const bool c64 = c.dtype == REMAP_DTYPE_F64;
    if (x64 && c64)
        launch_columns<Op, double, double>(p, a.n_batch, batch_major, stream);
    else if (x64)
        launch_columns<Op, double, float>(p, a.n_batch, batch_major, stream);
    else if (c64)
        launch_columns<Op, float, double>(p, a.n_batch, batch_major, stream);
    else
        launch_columns<Op, float, float>(p, a.n_batch, batch_major, stream);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace colpass
}  // namespace remap

#endif  // REMAP_COLPASS_H
