// remap_layers.hip -- columns averaged or integrated over depth ranges inside
// the apply (layer means, heat content): every entry of a row first reduces
// its source column over the range [A, B] -- the overlap of every layer with
// the range weighs the layer's value -- then enters the masked, renormalised
// sum, in one launch.  A column that ends above A is skipped exactly as a NaN
// is: the bathymetry mask falls out of the definition.  The vertical sibling
// of remap_levels.hip (the field AT a depth).
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.layers.apply
// is the same statement in numpy).  Depths are positive downward, from the
// top of each column's first layer.  For destination element (i, b, r) with
// [A, B] = [A_r, B_r] the row's entries j are walked in CSR order, two float64
// accumulators num and valid from +0.0; for each entry the source column
// c = cell(col_j) is walked k = 0 .. n_levels-1 ascending, from d = v = t =
// +0.0:
//
//   h = (double) H[c, b', k]
//   if !(h > 0): the layer is not there (NaN, zero, negative): skip it, d stays
//   top = d;  d = d + h
//   lo = top > A ? top : A;   hi = d < B ? d : B
//   if hi > lo:  o = hi - lo;  x = (double) X[c, b, k]
//                if x == x:  p = o * x;  v = v + p;  t = t + o
//   (the walk may stop once top >= B: nothing further can overlap)
//   the entry counts iff t > 0 and q is no NaN:  q = v / t (mean),  q = v (integral)
//   counts:  p = S_j * q;  num = num + p;  valid = valid + S_j      (every operation rounded on its own: no FMA contraction)
//   y = (valid > threshold) ? num / valid : NaN
//
// Comparisons with a NaN are false: a NaN bound gives an empty range; B = +inf
// is "to the bottom".  Every NaN written is the one quiet NaN
// 0x7ff8000000000000.
//
// One form, the shape of levels_rowlane: a lane per (row, b, r), r fastest, so
// neighbouring lanes walk the same source columns and share their lines; with
// several batches whose rows lie closer than the batches ((Time, nCells,
// nVertLevels)) the lanes run over (row, r) of ONE batch group and a lane
// serves kBatches batches with one fetch of the row's indices and weights
// (kBatchesShared where one walk of H serves them, below).  The walk reads a
// column's thicknesses kChunk levels at a time -- the indices clamped to the
// last level, so no load sits behind a branch; a clamped level is not there
// -- and gives the overlaps o_k of the chunk; X is read, kChunk levels
// clamped the same way, only for a chunk that has an overlap, and the walk
// ends with the chunk that starts at or below B.  The overlaps depend on H
// alone: with a time-invariant thickness (h_batch_stride == 0) one walk
// serves the batches of a lane.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace {

using namespace rowpass;

constexpr char kName[] = "remap_apply_layers";
constexpr int kUnroll = 4;          // (col, S) pairs fetched together
constexpr int kChunk = 8;           // levels of one step of the walk
constexpr int kBatches = 4;         // batches a lane serves (batch-major)
constexpr int kBatchesShared = 6;   // ... where one walk of H serves them all

struct LayersParams {               // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    const void *__restrict__ H;
    const double *__restrict__ bounds;
    double *__restrict__ Y;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner, k_inner = R
    int64_t ldx, bsx, ldy, bsy;
    int64_t ldh, bsh;               // H: row and batch stride (0: broadcast)
    int64_t src_outer, h_outer;
    uint32_t src_fold;
    int32_t n_levels;
    int32_t integral;               // reduce: 0 the mean, 1 the integral
    int64_t total;                  // n_rows * K
    double thr;
};

// element offsets of source cell a in X and in H, from one split
__device__ inline void cell_offsets(const LayersParams &p, int32_t a,
                                    int64_t &ox, int64_t &oh)
{
    int64_t o[2];
    rowpass::cell_offsets(p, a, {p.ldx, p.ldh}, {p.src_outer, p.h_outer}, o);
    ox = o[0];
    oh = o[1];
}

// The walk of the definition over one thickness column h of n levels, for the
// NW batches x, x + bsx, .. of which nw exist: v[w] and t[w] of every batch.
// (The overlaps are computed once; each batch adds its own layers in
// ascending k, as its own walk would.)
template <typename XT, typename HT, int NW>
__device__ inline void walk(const XT *__restrict__ x, int64_t bsx, int nw,
                            const HT *__restrict__ h, int32_t n, double A,
                            double B, double (&v)[NW], double (&t)[NW])
{
    const int32_t last = n - 1;
#pragma unroll
    for (int w = 0; w < NW; ++w)
        v[w] = t[w] = 0.0;
    double d = 0.0;
    for (int32_t k0 = 0; k0 < n; k0 += kChunk) {
        // (top >= B for this level and every one behind it)
        if (d >= B)
            break;
        int32_t ks[kChunk];
        double hs[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            ks[u] = k0 + u < last ? k0 + u : last;
            hs[u] = static_cast<double>(h[ks[u]]);
        }
        double o[kChunk];
        bool in[kChunk];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const bool there = k0 + u <= last && hs[u] > 0.0;
            const double top = d;
            const double below = d + hs[u];
            d = there ? below : d;
            const double lo = top > A ? top : A;
            const double hi = d < B ? d : B;
            o[u] = hi - lo;
            in[u] = there && hi > lo;
            any = any || in[u];
        }
        if (!any)
            continue;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (w < nw) {
                double xs[kChunk];
#pragma unroll
                for (int u = 0; u < kChunk; ++u)
                    xs[u] = static_cast<double>(x[w * bsx + ks[u]]);
#pragma unroll
                for (int u = 0; u < kChunk; ++u) {
                    if (in[u] && xs[u] == xs[u]) {
                        const double pu = o[u] * xs[u];
                        v[w] = v[w] + pu;
                        t[w] = t[w] + o[u];
                    }
                }
            }
        }
    }
}

struct Sums {
    double num, valid;
};

// an entry's column value enters the sums of its row
__device__ inline void add_entry(Sums &s, double a, double v, double t,
                                 bool integral)
{
    const double mean = v / t;
    const double q = integral ? v : mean;
    if (t > 0.0 && q == q) {
        const double pq = a * q;
        s.num = s.num + pq;
        s.valid = s.valid + a;
    }
}

// (a quotient that is itself a NaN -- inf / inf -- leaves as the same quiet
// NaN as a masked element: the bits of Y are defined)
__device__ inline double finish(const Sums &s, double thr)
{
    const double q = s.num / s.valid;
    return (s.valid > thr && q == q) ? q : __builtin_nan("");
}

// IT: the type the flat index is split in (rowpass::narrow_index).
// NB > 1 (batch-major): the lanes run over (row, r) of ONE batch group, r
// fastest, and a lane serves NB batches of its (row, r); a batch past the
// last is neither read nor stored.  NB == 1: the lanes run over (row, b, r).
// H_SHARED (batch-major only): h_batch_stride == 0, one walk of H serves the
// batches of the lane.
template <typename XT, typename HT, typename IT, int NB, bool H_SHARED>
__global__ __launch_bounds__(kBlock) void layers_rowlane(
    const LayersParams p, const int64_t n_batch)
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
    const double A = p.bounds[2 * static_cast<int64_t>(l)];
    const double B = p.bounds[2 * static_cast<int64_t>(l) + 1];
    const bool integral = p.integral != 0;
    const int64_t b0 = static_cast<int64_t>(b);
    const XT *__restrict__ X = static_cast<const XT *>(p.X) + b0 * p.bsx;
    const HT *__restrict__ H = static_cast<const HT *>(p.H) + b0 * p.bsh;
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
            int64_t ox, oh;
            cell_offsets(p, c[u], ox, oh);
            if constexpr (H_SHARED) {
                double v[NB], t[NB];
                walk<XT, HT, NB>(X + ox, p.bsx, nb, H + oh, p.n_levels, A, B,
                                 v, t);
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    if (n < nb)
                        add_entry(sum[n], a[u], v[n], t[n], integral);
            } else {
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    if (n < nb) {
                        double v[1], t[1];
                        walk<XT, HT, 1>(X + n * p.bsx + ox, 0, 1,
                                        H + n * p.bsh + oh, p.n_levels, A, B,
                                        v, t);
                        add_entry(sum[n], a[u], v[0], t[0], integral);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (n < nb)
            __builtin_nontemporal_store(finish(sum[n], p.thr),
                                        p.Y + o + n * p.bsy);
}

template <typename XT, typename HT>
int launch_layers(const LayersParams &p, int64_t n_batch, bool batch_major,
                  hipStream_t stream)
{
    // batch-major: a lane per kBatches batches; kBatchesShared of them where
    // one walk of H serves them all and there are more than kBatches
    const bool shared = batch_major && p.bsh == 0;
    const int nb = !batch_major ? 1
                   : shared && n_batch > kBatches ? kBatchesShared : kBatches;
    LayersParams q = p;
    if (batch_major)
        q.total = (n_batch + nb - 1) / nb * p.n_rows * p.k_inner;
    const dim3 grid = rowlane_grid(q.total);
    const bool narrow = narrow_index(p);
#define REMAP_LAYERS_LAUNCH(IT, NB, SHARED)                                 \
    hipLaunchKernelGGL((layers_rowlane<XT, HT, IT, NB, SHARED>), grid,      \
                       dim3(kBlock), 0, stream, q, n_batch)
    if (narrow && nb == kBatchesShared)
        REMAP_LAYERS_LAUNCH(uint32_t, kBatchesShared, true);
    else if (narrow && shared)
        REMAP_LAYERS_LAUNCH(uint32_t, kBatches, true);
    else if (narrow && batch_major)
        REMAP_LAYERS_LAUNCH(uint32_t, kBatches, false);
    else if (narrow)
        REMAP_LAYERS_LAUNCH(uint32_t, 1, false);
    else if (nb == kBatchesShared)
        REMAP_LAYERS_LAUNCH(int64_t, kBatchesShared, true);
    else if (shared)
        REMAP_LAYERS_LAUNCH(int64_t, kBatches, true);
    else if (batch_major)
        REMAP_LAYERS_LAUNCH(int64_t, kBatches, false);
    else
        REMAP_LAYERS_LAUNCH(int64_t, 1, false);
#undef REMAP_LAYERS_LAUNCH
    return REMAP_OK;
}

}  // namespace

int apply_layers(const remap_layers_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    // what the thicknesses and the reduction add to the shared checks
    if (a->n_levels < 1 || a->n_levels > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_levels %lld: expected >= 1", kName,
                    (long long)a->n_levels);
    if (a->h_dtype != REMAP_DTYPE_F64 && a->h_dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "%s: h_dtype %d is no REMAP_DTYPE_*",
                    kName, a->h_dtype);
    if (a->reduce != REMAP_REDUCE_MEAN && a->reduce != REMAP_REDUCE_INTEGRAL)
        return fail(REMAP_ERR_ARG, "%s: reduce %d is no REMAP_REDUCE_*",
                    kName, a->reduce);
    if (a->h_row_stride < 0 || a->h_batch_stride < 0)
        return fail(REMAP_ERR_ARG, "%s: a negative stride", kName);
    if (a->x_src_fold != 0 && a->h_outer_stride < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: x_src_fold = %lld with a negative h_outer_stride",
                    kName, (long long)a->x_src_fold);
    LayersParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a->A.nnz > 0 && (!p.col || !a->A.val)) || !a->X ||
        !a->H || !a->bounds || !a->Y)
        return fail(REMAP_ERR_ARG,
                    "%s: NULL rowptr, col, val, X, H, bounds or Y", kName);
    p.val = a->A.val;
    p.X = a->X;
    p.H = a->H;
    p.bounds = a->bounds;
    p.Y = a->Y;
    p.ldh = a->h_row_stride;
    p.bsh = a->h_batch_stride;
    p.h_outer = a->h_outer_stride;
    p.n_levels = static_cast<int32_t>(a->n_levels);
    p.integral = a->reduce == REMAP_REDUCE_INTEGRAL;
    p.thr = a->threshold;
    // several batches whose rows lie closer than the batches: the lanes run
    // over the rows and ranges of one batch group
    const bool batch_major = a->n_batch > 1 &&
                             a->y_row_stride <= a->y_batch_stride;
    const bool x64 = a->x_dtype == REMAP_DTYPE_F64;
    const bool h64 = a->h_dtype == REMAP_DTYPE_F64;
    int rc;
    if (x64 && h64)
        rc = launch_layers<double, double>(p, a->n_batch, batch_major, stream);
    else if (x64)
        rc = launch_layers<double, float>(p, a->n_batch, batch_major, stream);
    else if (h64)
        rc = launch_layers<float, double>(p, a->n_batch, batch_major, stream);
    else
        rc = launch_layers<float, float>(p, a->n_batch, batch_major, stream);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_apply_layers(const struct remap_layers_args *args, void *stream)
{
    return remap::apply_layers(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"
