// remap_sgs.hip -- sub-gridscale fraction weighting of the apply path: the
// field is multiplied by a fraction before the map and divided by the
// remapped fraction after it, in one launch (NCO's `ncremap --sgs_frc`).
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.sgs.apply is
// the same statement in numpy).  For destination element (i, b, k) the row's
// entries are walked in CSR order, three float64 accumulators from +0.0:
//   x = (double)X[cell(col), b, k];  f = (double)F[cell(col), b', k']
//   the entry counts iff neither is a NaN; then
//   t = f * x;  num += S * t;  den += S * f;  valid += S
//   y = (valid > threshold && den > 0) ? num / den : NaN
// Every product and every sum rounds on its own (the library is built with
// -ffp-contract=off, and nothing here asks for an fma); an entry that does
// not count is skipped, not added as a zero.  Every NaN written is the one
// quiet NaN 0x7ff8000000000000.
//
// Two forms, as remap_limit.hip has them.  Runs of at least a wave's width
// (k_inner >= 64) take a wave per (row, chunk of columns), sgs_rowwave below.
// Everything else takes one lane per (row, column), sgs_rowlane: a lane walks
// its row kUnroll entries at a time, the (col, S) pairs fetched together
// (index clamped to the row's last entry: no load sits behind a branch), then
// the source values and fractions together, then the sums in CSR order.
// Columns run fastest across the lanes; with several batches ((Time, nCells)
// and (Time, nCells, nCategories)) the columns of ONE batch do, then the
// rows -- for k_inner == 1 neighbouring lanes hold neighbouring rows -- and a
// lane serves four batches with one fetch of the row's indices and weights.
// No LDS, no atomics.  The pass moves what a REMAP_MODE_MASKED apply moves
// plus the fraction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace {

using namespace rowpass;

constexpr char kName[] = "remap_apply_sgs";
constexpr int kUnroll = 8;

struct SgsParams {                  // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    const void *__restrict__ F;
    double *__restrict__ Y;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner
    int64_t ldx, bsx, ldy, bsy;
    int64_t ldf, bsf, isf;          // F: row, batch and inner (0 | 1) stride
    int64_t src_outer, f_outer;
    uint32_t src_fold;
    int64_t total;                  // n_rows * K
    double thr;
};

// element offsets of source cell a in X and in F, from one split
__device__ inline void cell_offsets(const SgsParams &p, int32_t a,
                                    int64_t &ox, int64_t &of)
{
    int64_t o[2];
    rowpass::cell_offsets(p, a, {p.ldx, p.ldf}, {p.src_outer, p.f_outer}, o);
    ox = o[0];
    of = o[1];
}

struct Sums {
    double num, den, valid;
};

// one entry of the definition
__device__ inline void add_entry(Sums &s, double a, double x, double f)
{
    if (x == x && f == f) {
        const double t = f * x;
        const double pn = a * t;
        const double pd = a * f;
        s.num = s.num + pn;
        s.den = s.den + pd;
        s.valid = s.valid + a;
    }
}

// (a quotient that is itself a NaN -- inf / inf, a NaN weight -- leaves as
// the same quiet NaN as a masked element: the bits of Y are defined)
__device__ inline double finish(const Sums &s, double thr)
{
    const double q = s.num / s.den;
    return (s.valid > thr && s.den > 0.0 && q == q) ? q : __builtin_nan("");
}

// IT: the type the flat index is split in (rowpass::narrow_index).
// BATCH_MAJOR (several batches whose rows lie closer than the batches: (Time,
// nCells[, nCategories])): the lanes run over (row, k) of ONE batch, k
// fastest -- for k_inner == 1 neighbouring lanes hold neighbouring rows, and
// in every case a wave's Y is one contiguous piece -- and a lane serves
// kBatches batches of its (row, k): the row's indices and weights are fetched
// once for them.  (A batch past the last is served as a copy of the last and
// not stored.)
constexpr int kBatches = 4;

template <typename XT, typename FT, typename IT, bool BATCH_MAJOR>
__global__ __launch_bounds__(kBlock) void sgs_rowlane(const SgsParams p,
                                                      const int64_t n_batch)
{
    constexpr int NB = BATCH_MAJOR ? kBatches : 1;
    constexpr int UNR = BATCH_MAJOR ? kUnroll / 2 : kUnroll;
    const int64_t gid64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid64 >= p.total)
        return;
    const IT gid = static_cast<IT>(gid64);
    const IT ki = static_cast<IT>(p.k_inner);
    IT r, b, k;
    if constexpr (BATCH_MAJOR) {
        const IT per = static_cast<IT>(p.n_rows) * ki;
        const IT bg = gid / per;
        const IT rem = gid - bg * per;
        r = rem / ki;
        k = rem - r * ki;
        b = bg * NB;
    } else {
        const IT K = static_cast<IT>(p.K);
        r = gid / K;
        const IT kf = gid - r * K;
        b = kf / ki;
        k = kf - b * ki;
    }
    const int64_t i = p.row_begin + static_cast<int64_t>(r);
    const XT *__restrict__ X[NB];
    const FT *__restrict__ F[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        int64_t bn = static_cast<int64_t>(b) + n;
        if (bn > n_batch - 1)
            bn = n_batch - 1;
        X[n] = static_cast<const XT *>(p.X) + bn * p.bsx +
               static_cast<int64_t>(k);
        F[n] = static_cast<const FT *>(p.F) + bn * p.bsf +
               static_cast<int64_t>(k) * p.isf;
    }
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    Sums sum[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
        sum[n] = {0.0, 0.0, 0.0};
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double a[UNR];
        XT xs[UNR][NB];
        FT fs[UNR][NB];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            a[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            int64_t ox, of;
            cell_offsets(p, c[u], ox, of);
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                xs[u][n] = X[n][ox];
                fs[u][n] = F[n][of];
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e) {
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    add_entry(sum[n], a[u], static_cast<double>(xs[u][n]),
                              static_cast<double>(fs[u][n]));
            }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (static_cast<int64_t>(b) + n < n_batch)
            __builtin_nontemporal_store(finish(sum[n], p.thr),
                                        p.Y + o + n * p.bsy);
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns, as limit_rowwave -- for runs of >= kWave columns; the
// work list and VEC are rowpass.h's.  The row is the same in every lane, so
// the row pointers, the column indices and the weights are scalar loads, the
// loop over the row's entries is wave-uniform and reads exactly the row's
// entries, UNR source runs in flight at a time.  Y is written once
// (store_once).
//
// F_UNI (f_inner_stride == 0, the common case: a (Time, nCells) fraction for
// (Time, nCells, nCategories) fields): the fraction of an entry is the same
// in every lane and is loaded once per entry.  As long as no lane of the wave
// has met a NaN in X, den and valid are the same in every lane too and are
// kept ONCE (the first loop below); the first group of entries with a NaN in
// some lane hands them to per-lane copies and the second loop finishes the
// row.  Every lane performs the same additions in the same order either way:
// the bits do not depend on which loop served an entry.
// ---------------------------------------------------------------------------
template <typename XT, typename FT, int VEC, bool F_UNI>
__global__ __launch_bounds__(kBlock) void sgs_rowwave(const SgsParams p,
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
    // (F_UNI: the same address in every lane)
    const FT *__restrict__ F = static_cast<const FT *>(p.F) + b * p.bsf +
                               (F_UNI ? 0 : k);
    const int64_t o = i * p.ldy + b * p.bsy + k;
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    using PX = Pack<XT, VEC>;
    using PF = Pack<FT, F_UNI ? 1 : VEC>;
    Sums sum[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        sum[v] = {0.0, 0.0, 0.0};
    int64_t j = s;
    if constexpr (F_UNI) {
        // den and valid once for the wave, while X shows no NaN
        double den = 0.0, valid = 0.0;
        for (; j + UNR <= e; j += UNR) {
            PX xs[UNR];
            double a[UNR], f[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                int64_t ox, of;
                cell_offsets(p, p.col[j + u], ox, of);
                a[u] = p.val[j + u];
                xs[u] = *reinterpret_cast<const PX *>(X + ox);
                f[u] = static_cast<double>(F[of]);
            }
            bool nan = false;
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    nan = nan || xs[u].v[v] != xs[u].v[v];
            if (__builtin_amdgcn_ballot_w64(nan) != 0)
                break;                          // (wave-uniform)
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (f[u] == f[u]) {             // (wave-uniform)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const double t =
                            f[u] * static_cast<double>(xs[u].v[v]);
                        const double pn = a[u] * t;
                        sum[v].num = sum[v].num + pn;
                    }
                    const double pd = a[u] * f[u];
                    den = den + pd;
                    valid = valid + a[u];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            sum[v].den = den;
            sum[v].valid = valid;
        }
    }
    for (; j + UNR <= e; j += UNR) {
        PX xs[UNR];
        PF fs[UNR];
        double a[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            int64_t ox, of;
            cell_offsets(p, p.col[j + u], ox, of);
            a[u] = p.val[j + u];
            xs[u] = *reinterpret_cast<const PX *>(X + ox);
            fs[u] = *reinterpret_cast<const PF *>(F + of);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                add_entry(sum[v], a[u], static_cast<double>(xs[u].v[v]),
                          static_cast<double>(fs[u].v[F_UNI ? 0 : v]));
    }
    for (; j < e; ++j) {
        int64_t ox, of;
        cell_offsets(p, p.col[j], ox, of);
        const double a = p.val[j];
        const PX x = *reinterpret_cast<const PX *>(X + ox);
        const PF f = *reinterpret_cast<const PF *>(F + of);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            add_entry(sum[v], a, static_cast<double>(x.v[v]),
                      static_cast<double>(f.v[F_UNI ? 0 : v]));
    }
    Pack<double, VEC> y;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        y.v[v] = finish(sum[v], p.thr);
    store_once<VEC>(p.Y + o, y);
}

template <typename XT, typename FT>
int launch_rowwave(const SgsParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool f_uni = p.isf == 0;
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16) &&
                      (f_uni || (p.ldf % 2 == 0 && p.bsf % 2 == 0 &&
                                 p.f_outer % 2 == 0 &&
                                 aligned_to(p.F, 2 * sizeof(FT))));
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even && f_uni)
        hipLaunchKernelGGL((sgs_rowwave<XT, FT, 2, true>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    else if (even)
        hipLaunchKernelGGL((sgs_rowwave<XT, FT, 2, false>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    else if (f_uni)
        hipLaunchKernelGGL((sgs_rowwave<XT, FT, 1, true>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    else
        hipLaunchKernelGGL((sgs_rowwave<XT, FT, 1, false>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    return REMAP_OK;
}

template <typename XT, typename FT>
int launch_sgs(const SgsParams &p, int64_t n_batch, bool batch_major,
               hipStream_t stream)
{
    if (p.k_inner >= kWave)
        // runs of a wave's width and more: a wave per (row, chunk)
        return launch_rowwave<XT, FT>(p, n_batch, stream);
    SgsParams q = p;
    if (batch_major)                // (a lane per kBatches batches)
        q.total = (n_batch + kBatches - 1) / kBatches * p.n_rows * p.k_inner;
    const dim3 grid = rowlane_grid(q.total);
    const bool narrow = narrow_index(p);
    if (narrow && batch_major)
        hipLaunchKernelGGL((sgs_rowlane<XT, FT, uint32_t, true>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (narrow)
        hipLaunchKernelGGL((sgs_rowlane<XT, FT, uint32_t, false>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (batch_major)
        hipLaunchKernelGGL((sgs_rowlane<XT, FT, int64_t, true>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else
        hipLaunchKernelGGL((sgs_rowlane<XT, FT, int64_t, false>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    return REMAP_OK;
}

}  // namespace

int apply_sgs(const remap_sgs_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    // what the fraction adds to the shared checks
    if (a->f_dtype != REMAP_DTYPE_F64 && a->f_dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "%s: f_dtype %d is no REMAP_DTYPE_*",
                    kName, a->f_dtype);
    if (a->f_row_stride < 0 || a->f_batch_stride < 0)
        return fail(REMAP_ERR_ARG, "%s: a negative stride", kName);
    if (a->f_inner_stride != 0 && a->f_inner_stride != 1)
        return fail(REMAP_ERR_ARG,
                    "%s: f_inner_stride %lld: expected 0 (broadcast) or 1",
                    kName, (long long)a->f_inner_stride);
    if (a->x_src_fold != 0 && a->f_outer_stride < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: x_src_fold = %lld with a negative f_outer_stride",
                    kName, (long long)a->x_src_fold);
    SgsParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a->A.nnz > 0 && (!p.col || !a->A.val)) || !a->X ||
        !a->F || !a->Y)
        return fail(REMAP_ERR_ARG, "%s: NULL rowptr, col, val, X, F or Y",
                    kName);
    p.val = a->A.val;
    p.X = a->X;
    p.F = a->F;
    p.Y = a->Y;
    p.ldf = a->f_row_stride;
    p.bsf = a->f_batch_stride;
    p.isf = a->f_inner_stride;
    p.f_outer = a->f_outer_stride;
    p.thr = a->threshold;
    // several batches whose rows lie closer than the batches: the lanes run
    // over the rows and columns of one batch
    const bool batch_major = a->n_batch > 1 &&
                             a->y_row_stride <= a->y_batch_stride;
    const bool x64 = a->x_dtype == REMAP_DTYPE_F64;
    const bool f64 = a->f_dtype == REMAP_DTYPE_F64;
    int rc;
    if (x64 && f64)
        rc = launch_sgs<double, double>(p, a->n_batch, batch_major, stream);
    else if (x64)
        rc = launch_sgs<double, float>(p, a->n_batch, batch_major, stream);
    else if (f64)
        rc = launch_sgs<float, double>(p, a->n_batch, batch_major, stream);
    else
        rc = launch_sgs<float, float>(p, a->n_batch, batch_major, stream);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_apply_sgs(const struct remap_sgs_args *args, void *stream)
{
    return remap::apply_sgs(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"
