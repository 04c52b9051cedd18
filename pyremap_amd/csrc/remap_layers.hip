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
// The lane form is colpass.h's.  The walk reads a column's thicknesses kChunk
// levels at a time -- the indices clamped to the last level, so no load sits
// behind a branch; a clamped level is not there -- and gives the overlaps o_k
// of the chunk; X is read, kChunk levels clamped the same way, only for a
// chunk that has an overlap, and the walk ends with the chunk that starts at
// or below B.  The overlaps depend on H alone: with a time-invariant
// thickness (h_batch_stride == 0) one walk serves the batches of a lane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "colpass.h"
#include "remap_common.h"

namespace remap {
namespace {

using namespace colpass;

constexpr char kName[] = "remap_apply_layers";
constexpr int kChunk = 8;           // levels of one step of the walk

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

struct Range {
    double A, B;
};

struct LayersOp {
    static constexpr int kBatches = 4;
    static constexpr int kBatchesShared = 6;

    __device__ static Range query(const ColumnParams &p, int64_t r)
    {
        return {p.Q[2 * r], p.Q[2 * r + 1]};
    }

    template <typename XT, typename HT, int NW>
    __device__ __forceinline__ static void entry(
        const XT *__restrict__ x, int64_t bsx, int nw,
        const HT *__restrict__ h, int32_t n_levels, const Range &range,
        bool integral, double a, Sums *sums)
    {
        double v[NW], t[NW];
        walk<XT, HT, NW>(x, bsx, nw, h, n_levels, range.A, range.B, v, t);
#pragma unroll
        for (int n = 0; n < NW; ++n)
            if (n < nw)
                add_entry(sums[n], a, v[n], t[n], integral);
    }
};

}  // namespace

int apply_layers(const remap_layers_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    const Companion c = {"h", "H, bounds", a->H, a->h_dtype, a->h_row_stride,
                         a->h_batch_stride, a->h_outer_stride, a->bounds};
    const auto reduce_ok = [a] {
        if (a->reduce != REMAP_REDUCE_MEAN &&
            a->reduce != REMAP_REDUCE_INTEGRAL)
            return fail(REMAP_ERR_ARG, "%s: reduce %d is no REMAP_REDUCE_*",
                        kName, a->reduce);
        return int(REMAP_OK);
    };
    ColumnParams p;
    bool empty;
    const int checked = check_columns(kName, *a, c, reduce_ok, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    p.mode = a->reduce == REMAP_REDUCE_INTEGRAL;
    return apply_columns<LayersOp>(*a, c, p, stream);
}

}  // namespace remap

extern "C" {

int remap_apply_layers(const struct remap_layers_args *args, void *stream)
{
    return remap::apply_layers(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"

