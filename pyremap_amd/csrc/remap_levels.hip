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
// The lane form is colpass.h's.  The search reads a column's coordinate
// kChunk + 1 levels at a time -- the indices clamped to the last level, so no
// load sits behind a branch: a clamped pair is (z, z), which brackets nothing,
// and a clamped node repeats one that was tested before it -- and takes the
// first hit of the chunk in the order of the definition; the one or two
// values of X are read after the hit.  The search reads Z alone and gives
// (level, weight): with a time-invariant coordinate (z_batch_stride == 0) one
// search serves the batches of a lane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "colpass.h"
#include "remap_common.h"

namespace remap {
namespace {

using namespace colpass;

constexpr char kName[] = "remap_apply_levels";
constexpr int kChunk = 16;          // levels of one step of the search

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

struct LevelsOp {
    static constexpr int kBatches = 4;
    static constexpr int kBatchesShared = 12;

    __device__ static double query(const ColumnParams &p, int64_t l)
    {
        return p.Q[l];
    }

    template <typename XT, typename ZT, int NW>
    __device__ __forceinline__ static void entry(
        const XT *__restrict__ x, int64_t bsx, int nw,
        const ZT *__restrict__ z, int32_t n_levels, double t, bool,
        double a, Sums *sums)
    {
        int32_t k = 0;
        double w = 0.0;
        const Hit hit = locate(z, n_levels, t, k, w);
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            if (n < nw) {
                if (hit != kNone) {
                    const double v = value_at(x + n * bsx, hit, k, w);
                    if (v == v) {
                        const double pn = a * v;
                        sums[n].num = sums[n].num + pn;
                        sums[n].valid = sums[n].valid + a;
                    }
                }
            }
        }
    }
};

}  // namespace

int apply_levels(const remap_levels_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    const Companion c = {"z", "Z, T", a->Z, a->z_dtype, a->z_row_stride,
                         a->z_batch_stride, a->z_outer_stride, a->T};
    ColumnParams p;
    bool empty;
    const int checked = check_columns(
        kName, *a, c, [] { return int(REMAP_OK); }, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    p.mode = 0;
    return apply_columns<LevelsOp>(*a, c, p, stream);
}

}  // namespace remap

extern "C" {

int remap_apply_levels(const struct remap_levels_args *args, void *stream)
{
    return remap::apply_levels(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"
