// remap_levels.hip -- columns interpolated to target levels inside the apply
// (depth slices): every entry of a row first interpolates its source column
// to the target level, then enters the masked, renormalised sum, in one
// launch.  An entry whose column does not reach the level is skipped exactly
// as a NaN is: the bathymetry mask falls out of the definition.
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.levels.apply
// is the same statement in numpy).  For destination element (i, b, l) the
// row's entries j are walked in CSR order, two float64 accumulators from +0.0:
//
//   t = T[l];   z_k = (double) Z[cell(col_j), b', k];   x_k = (double) X[cell(col_j), b, k]
//   walk k = 0 .. n_levels-1 in ascending order and stop at the first hit:
//     node hit:      t == z_k:   v = x_k      (x_{k+1} is not looked at)
//     interior hit:  k+1 < n_levels and (z_k < t && t < z_{k+1}  or  z_k > t && t > z_{k+1}):
//                    w = (t - z_k) / (z_{k+1} - z_k);   v = x_k + w * (x_{k+1} - x_k)
//     no hit:        the column has no value at this level
//   the entry counts iff its column has a hit and v is no NaN
//   counts:  num += S_j * v;   valid += S_j      (every operation rounded on its own: no FMA contraction)
//   y = (valid > threshold) ? num / valid : NaN
//
// Comparisons with a NaN are false: a NaN in Z never brackets anything.
// Columns may rise or fall, nothing assumes that they are monotone, nothing
// is extrapolated.  Every NaN written is the one quiet NaN 0x7ff8000000000000.
//
// One form: a lane per (row, b, l), l fastest, so neighbouring lanes walk the
// same source columns and share their lines; with several batches whose rows
// lie closer than the batches ((Time, nCells, nVertLevels)) the lanes run
// over (row, l) of ONE batch and a lane serves kBatches batches with one
// fetch of the row's indices and weights, as sgs_rowlane does
// (kBatchesShared where one search serves them, below).  The search
// reads a column's coordinate kChunk + 1 levels at a time -- the indices
// clamped to the last level, so no load sits behind a branch: a clamped pair
// is (z, z), which brackets nothing, and a clamped node repeats one that was
// tested before it -- and takes the first hit of the chunk in the order of
// the definition; the one or two values of X are read after the hit.  The
// search reads Z alone and gives (level, weight): with a time-invariant
// coordinate (z_batch_stride == 0) one search serves the batches of a lane.
// No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace {

using namespace rowpass;

constexpr char kName[] = "remap_apply_levels";
constexpr int kUnroll = 4;          // (col, S) pairs fetched together
constexpr int kChunk = 16;          // levels of one step of the search
constexpr int kBatches = 4;         // batches a lane serves (batch-major)
constexpr int kBatchesShared = 12;  // ... where one search serves them all

struct LevelsParams {               // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    const void *__restrict__ Z;
    const double *__restrict__ T;
    double *__restrict__ Y;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner, k_inner = L
    int64_t ldx, bsx, ldy, bsy;
    int64_t ldz, bsz;               // Z: row and batch stride (0: broadcast)
    int64_t src_outer, z_outer;
    uint32_t src_fold;
    int32_t n_levels;
    int64_t total;                  // n_rows * K
    double thr;
};

// element offsets of source cell a in X and in Z, from one split
__device__ inline void cell_offsets(const LevelsParams &p, int32_t a,
                                    int64_t &ox, int64_t &oz)
{
    int64_t o[2];
    rowpass::cell_offsets(p, a, {p.ldx, p.ldz}, {p.src_outer, p.z_outer}, o);
    ox = o[0];
    oz = o[1];
}

// The search of the definition: the first hit of t in the coordinate column
// z of n levels.  kNone: the column has no value at this level; kNode: t ==
// z[k]; kInside: t lies strictly between z[k] and z[k + 1], w is its weight.
enum Hit : int { kNone = 0, kNode = 1, kInside = 2 };

template <typename ZT>
__device__ inline Hit locate(const ZT *__restrict__ z, int32_t n, double t,
                             int32_t &k, double &w)
{
    const int32_t last = n - 1;
    for (int32_t k0 = 0; k0 < n; k0 += kChunk) {
        double zs[kChunk + 1];
#pragma unroll
        for (int u = 0; u <= kChunk; ++u) {
            const int32_t ku = k0 + u < last ? k0 + u : last;
            zs[u] = static_cast<double>(z[ku]);
        }
        // one comparison each way per level; a pair brackets t where one
        // level lies above it and the next below, or the other way round
        bool above[kChunk + 1], below[kChunk + 1];
#pragma unroll
        for (int u = 0; u <= kChunk; ++u) {
            above[u] = zs[u] > t;
            below[u] = zs[u] < t;
        }
        // the first level of the chunk with a hit of either kind (a node
        // comes before the pair that starts at it, and excludes it)
        int hit = -1;
#pragma unroll
        for (int u = kChunk - 1; u >= 0; --u)
            if ((below[u] && above[u + 1]) || (above[u] && below[u + 1]) ||
                t == zs[u])
                hit = u;
        if (hit < 0)
            continue;
        // (a node hit of a clamped index repeats level `last`; an interior
        // hit has k + 1 <= last: a clamped pair is (z, z))
        const int32_t ku = k0 + hit;
        k = ku < last ? ku : last;
        const double z0 = static_cast<double>(z[k]);
        if (t == z0)
            return kNode;
        const double z1 = static_cast<double>(z[k + 1]);
        const double num = t - z0;
        const double den = z1 - z0;
        w = num / den;
        return kInside;
    }
    return kNone;
}

// The column value at a hit: X[k] at a node, the linear interpolant between
// X[k] and X[k + 1] inside (X[k + 1] is not looked at for a node).
template <typename XT>
__device__ inline double value_at(const XT *__restrict__ x, Hit hit,
                                  int32_t k, double w)
{
    const double x0 = static_cast<double>(x[k]);
    if (hit == kNode)
        return x0;
    const double x1 = static_cast<double>(x[k + 1]);
    const double dx = x1 - x0;
    const double wd = w * dx;
    return x0 + wd;
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
// Z_SHARED (batch-major only): z_batch_stride == 0, one search serves the
// batches of the lane.
template <typename XT, typename ZT, typename IT, int NB, bool Z_SHARED>
__global__ __launch_bounds__(kBlock) void levels_rowlane(
    const LevelsParams p, const int64_t n_batch)
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
    const double t = p.T[static_cast<int64_t>(l)];
    const int64_t b0 = static_cast<int64_t>(b);
    const XT *__restrict__ X = static_cast<const XT *>(p.X) + b0 * p.bsx;
    const ZT *__restrict__ Z = static_cast<const ZT *>(p.Z) + b0 * p.bsz;
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
            int64_t ox, oz;
            cell_offsets(p, c[u], ox, oz);
            Hit hit = kNone;
            int32_t k = 0;
            double w = 0.0;
            // (a time-invariant coordinate is searched once for the batches
            // of the lane)
            if constexpr (Z_SHARED)
                hit = locate(Z + oz, p.n_levels, t, k, w);
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                if (n < nb) {
                    if constexpr (!Z_SHARED)
                        hit = locate(Z + n * p.bsz + oz, p.n_levels, t, k, w);
                    if (hit != kNone) {
                        const double v = value_at(X + n * p.bsx + ox, hit, k,
                                                  w);
                        if (v == v) {
                            const double pn = a[u] * v;
                            sum[n].num = sum[n].num + pn;
                            sum[n].valid = sum[n].valid + a[u];
                        }
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

template <typename XT, typename ZT>
int launch_levels(const LevelsParams &p, int64_t n_batch, bool batch_major,
                  hipStream_t stream)
{
    // batch-major: a lane per kBatches batches; kBatchesShared of them where
    // one search serves them all and there are more than kBatches
    const bool shared = batch_major && p.bsz == 0;
    const int nb = !batch_major ? 1
                   : shared && n_batch > kBatches ? kBatchesShared : kBatches;
    LevelsParams q = p;
    if (batch_major)
        q.total = (n_batch + nb - 1) / nb * p.n_rows * p.k_inner;
    const dim3 grid = rowlane_grid(q.total);
    const bool narrow = narrow_index(p);
#define REMAP_LEVELS_LAUNCH(IT, NB, SHARED)                                 \
    hipLaunchKernelGGL((levels_rowlane<XT, ZT, IT, NB, SHARED>), grid,      \
                       dim3(kBlock), 0, stream, q, n_batch)
    if (narrow && nb == kBatchesShared)
        REMAP_LEVELS_LAUNCH(uint32_t, kBatchesShared, true);
    else if (narrow && shared)
        REMAP_LEVELS_LAUNCH(uint32_t, kBatches, true);
    else if (narrow && batch_major)
        REMAP_LEVELS_LAUNCH(uint32_t, kBatches, false);
    else if (narrow)
        REMAP_LEVELS_LAUNCH(uint32_t, 1, false);
    else if (nb == kBatchesShared)
        REMAP_LEVELS_LAUNCH(int64_t, kBatchesShared, true);
    else if (shared)
        REMAP_LEVELS_LAUNCH(int64_t, kBatches, true);
    else if (batch_major)
        REMAP_LEVELS_LAUNCH(int64_t, kBatches, false);
    else
        REMAP_LEVELS_LAUNCH(int64_t, 1, false);
#undef REMAP_LEVELS_LAUNCH
    return REMAP_OK;
}

}  // namespace

int apply_levels(const remap_levels_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    // what the level coordinate adds to the shared checks
    if (a->n_levels < 1 || a->n_levels > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_levels %lld: expected >= 1", kName,
                    (long long)a->n_levels);
    if (a->z_dtype != REMAP_DTYPE_F64 && a->z_dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "%s: z_dtype %d is no REMAP_DTYPE_*",
                    kName, a->z_dtype);
    if (a->z_row_stride < 0 || a->z_batch_stride < 0)
        return fail(REMAP_ERR_ARG, "%s: a negative stride", kName);
    if (a->x_src_fold != 0 && a->z_outer_stride < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: x_src_fold = %lld with a negative z_outer_stride",
                    kName, (long long)a->x_src_fold);
    LevelsParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a->A.nnz > 0 && (!p.col || !a->A.val)) || !a->X ||
        !a->Z || !a->T || !a->Y)
        return fail(REMAP_ERR_ARG,
                    "%s: NULL rowptr, col, val, X, Z, T or Y", kName);
    p.val = a->A.val;
    p.X = a->X;
    p.Z = a->Z;
    p.T = a->T;
    p.Y = a->Y;
    p.ldz = a->z_row_stride;
    p.bsz = a->z_batch_stride;
    p.z_outer = a->z_outer_stride;
    p.n_levels = static_cast<int32_t>(a->n_levels);
    p.thr = a->threshold;
    // several batches whose rows lie closer than the batches: the lanes run
    // over the rows and levels of one batch
    const bool batch_major = a->n_batch > 1 &&
                             a->y_row_stride <= a->y_batch_stride;
    const bool x64 = a->x_dtype == REMAP_DTYPE_F64;
    const bool z64 = a->z_dtype == REMAP_DTYPE_F64;
    int rc;
    if (x64 && z64)
        rc = launch_levels<double, double>(p, a->n_batch, batch_major, stream);
    else if (x64)
        rc = launch_levels<double, float>(p, a->n_batch, batch_major, stream);
    else if (z64)
        rc = launch_levels<float, double>(p, a->n_batch, batch_major, stream);
    else
        rc = launch_levels<float, float>(p, a->n_batch, batch_major, stream);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_apply_levels(const struct remap_levels_args *args, void *stream)
{
    return remap::apply_levels(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"
