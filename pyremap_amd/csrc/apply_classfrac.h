// apply_classfrac.h -- REMAP_MODE_CLASSFRAC of remap_apply_f64: sub-grid
// composition.  Largest area fraction (apply_laf.h) says which class takes the
// most of a destination cell; this mode says what share of the cell every
// class takes -- percent cover per land-cover type, elevation or depth bands
// (a histogram of a continuous field whose values were turned into bin
// indices), fractional region masks.  LAF is the argmax of exactly these
// sums.  Included by remap_spmm.hip; stands on rowpass.h; the two forms are
// apply_laf.h's.
//
// Definition (include/remap_hip.h has the contract;
// pyremap_amd.classfrac.class_fractions is the same statement in numpy).  X is
// ONE batch of class indices held as numbers; n_batch is the number of
// classes C and the batches of Y are the classes.  For destination element
// (i, k) the entries j of row i are walked in CSR order:
//   x = (double) X[cell(col_j), k]
//   the entry counts iff x is no NaN; then valid = valid + S_j
//   a counted entry belongs to class c iff x == (double) c for an integer c
//   in [0, C); -0.0 is class 0; a non-integer, +-inf or a value outside the
//   range counts in valid alone
//   w_c = w_c + S_j for the entry's class and for no other
//   valid and every w_c start at +0.0; every sum rounded, in CSR order
//   y_c = valid > threshold ? w_c / valid : NaN, for every c: one division
//   a NaN quotient is written as the canonical NaN 0x7ff8000000000000
// Sums of the row's weights, comparisons and one division per output: nothing
// that could be contracted, so two runs and the two forms below give the same
// bytes.
//
// Class tile.  An element keeps the sums of T <= kTile consecutive classes in
// registers: the loops over them are unrolled and every access is a
// compare-and-select under a compile-time index, so nothing is indexed at run
// time and nothing goes to scratch.  T is 4, 8 or kTile, the least that holds
// C (a map of four classes does not pay for sixteen).  With C > kTile the row
// is walked again for every further tile -- its entries come from L1 -- so X
// is gathered ceil(C / kTile) times, not C times; `valid` is added up again in
// every walk, by the same adds in the same order.  An entry's place in the
// tile is found without converting a value that has none: d = x - tile_base is
// compared with [0, T) first (a NaN, an infinity or 1e300 fails there), only
// then converted, and the result compared back with d, which a non-integer
// fails.  (x - tile_base is exact: the tile base is 0, or x lies in
// [base, 2 * base).)
//
// Two forms, as apply_laf.h has them:
//   rowlane  one lane per (row, column), for k_inner < kWave: a block is
//            rows_per_block rows of k_inner columns, columns fastest (k_inner
//            = 1, a static 2-D field: a lane per row);
//   rowwave  one wave per (row, chunk of kWave * VEC columns) for
//            k_inner >= kWave: col and val are wave-uniform scalar loads.
// Registers and global memory only: no workgroup memory, no read-modify-write
// of memory, every element of Y written once, through store_once, by the lane
// that owns it.
#ifndef REMAP_APPLY_CLASSFRAC_H
#define REMAP_APPLY_CLASSFRAC_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace classfrac {

using namespace rowpass;

constexpr char kName[] = "remap_apply_f64";
constexpr int kTile = 16;             // classes an element keeps in registers
constexpr int64_t kMaxClasses = 256;  // (8-bit rasters; a Y of (C, n_b, k))

struct FracParams {                 // (rowpass.h: P)
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
    int64_t K, k_inner;             // K = n_classes * k_inner
    int64_t ldx, bsx, ldy, bsy;     // bsx = 0; bsy: from class to class
    int64_t src_outer;
    uint32_t src_fold;
    int64_t total;                  // n_rows * K
    int32_t n_classes;
    uint32_t rows_per_block;        // rowlane: the lanes of a block are
                                    // rows_per_block rows of k_inner columns
};

__device__ inline bool gate_closed(const FracParams &p)
{
    return p.gate != nullptr && *p.gate != p.gate_value;
}

__device__ inline double quiet_nan()
{
    return __longlong_as_double(0x7ff8000000000000LL);
}

// element offset of source cell a in X
__device__ inline int64_t x_offset(const FracParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// The sums of one element for the classes [base, base + T).  (Arrays under
// unrolled loops: every index is a constant once unrolled.)
template <int T>
struct Sums {
    double w[T];
    double valid;
};

template <int T>
__device__ inline void clear(Sums<T> &t)
{
#pragma unroll
    for (int c = 0; c < T; ++c)
        t.w[c] = 0.0;
    t.valid = 0.0;
}

template <int T>
__device__ inline void count(Sums<T> &t, double x, double s, double base)
{
    if (!(x == x))
        return;
    t.valid = t.valid + s;
    const double d = x - base;
    const bool inside = d >= 0.0 && d < static_cast<double>(T);
    const int r = static_cast<int>(inside ? d : 0.0);   // (-0.0: class 0)
    const bool whole = inside && static_cast<double>(r) == d;
#pragma unroll
    for (int c = 0; c < T; ++c) {
        const double sum = t.w[c] + s;
        t.w[c] = (whole && r == c) ? sum : t.w[c];
    }
}

// what class slot c of the tile writes
template <int T>
__device__ inline double fraction(const Sums<T> &t, int c, double thr)
{
    const double q = t.w[c] / t.valid;
    return (t.valid > thr && q == q) ? q : quiet_nan();
}

// ---------------------------------------------------------------------------
// rowlane: one lane per (row, column); the block is rows_per_block rows of
// k_inner columns.  32-bit divisions only.
// ---------------------------------------------------------------------------
template <typename XT, int T>
__global__ __launch_bounds__(kBlock) void classfrac_rowlane(const FracParams p)
{
    constexpr int UNR = 4;
    if (gate_closed(p))
        return;
    const uint32_t ki = static_cast<uint32_t>(p.k_inner);
    const uint32_t rl = threadIdx.x / ki;
    const uint32_t k = threadIdx.x - rl * ki;
    const int64_t r = (int64_t)blockIdx.x * p.rows_per_block + rl;
    if (rl >= p.rows_per_block || r >= p.n_rows)
        return;
    const int64_t i = p.row_begin + r;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) +
                               static_cast<int64_t>(k);
    const int64_t o = i * p.ldy + static_cast<int64_t>(k);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    for (int base = 0; base < p.n_classes; base += T) {
        Sums<T> t;
        clear(t);
        for (int64_t j0 = s; j0 < e; j0 += UNR) {
            int32_t c[UNR];
            double w[UNR];
            XT xs[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t jj = j0 + u < e ? j0 + u : e - 1;
                c[u] = p.col[jj];
                w[u] = p.val[jj];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                xs[u] = X[x_offset(p, c[u])];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                if (j0 + u < e)
                    count(t, static_cast<double>(xs[u]), w[u],
                          static_cast<double>(base));
        }
#pragma unroll
        for (int c = 0; c < T; ++c) {
            if (base + c < p.n_classes) {
                const int64_t oc = o +
                                   static_cast<int64_t>(base + c) * p.bsy;
                Pack<double, 1> y;
                y.v[0] = fraction(t, c, p.thr);
                store_once<1>(p.Y + oc, y);
                if (p.mask_out)
                    p.mask_out[oc] = y.v[0] == y.v[0] ? 0 : 1;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns; the work list and VEC are rowpass.h's (one batch: X has
// one).  The row is the same in every lane: the row pointers, the column
// indices and the weights are scalar loads and the loops over the row's
// entries and over the class tiles are wave-uniform.
// ---------------------------------------------------------------------------
template <typename XT, int VEC, int T>
__global__ __launch_bounds__(kBlock) void classfrac_rowwave(
    const FracParams p, const int64_t n_waves, const int64_t chunks,
    const int64_t per_xcd)
{
    constexpr int UNR = 4;
    if (gate_closed(p))
        return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = rowwave_place(per_xcd);
    if (w >= n_waves)
        return;
    const int64_t chunk = w / p.n_rows;         // chunk-major
    const int64_t r = w - chunk * p.n_rows;
    const int64_t k = chunk * (kWave * VEC) + (int64_t)lane * VEC;
    if (k >= p.k_inner)                         // (VEC = 2: k_inner is even)
        return;
    const int64_t i = p.row_begin + r;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) + k;
    const int64_t o = i * p.ldy + k;
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    using PX = Pack<XT, VEC>;
    for (int base = 0; base < p.n_classes; base += T) {
        const double fbase = static_cast<double>(base);
        Sums<T> t[VEC];
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
                    count(t[v], static_cast<double>(xs[u].v[v]), ws[u],
                          fbase);
        }
        for (; j < e; ++j) {
            const PX x = *reinterpret_cast<const PX *>(
                X + x_offset(p, p.col[j]));
            const double ws = p.val[j];
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                count(t[v], static_cast<double>(x.v[v]), ws, fbase);
        }
#pragma unroll
        for (int c = 0; c < T; ++c) {
            if (base + c < p.n_classes) {
                const int64_t oc = o +
                                   static_cast<int64_t>(base + c) * p.bsy;
                Pack<double, VEC> y;
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    y.v[v] = fraction(t[v], c, p.thr);
                store_once<VEC>(p.Y + oc, y);
                if (p.mask_out) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v)
                        p.mask_out[oc + v] = y.v[v] == y.v[v] ? 0 : 1;
                }
            }
        }
    }
}

template <typename XT, int T>
int launch_rowwave(const FracParams &p, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, 1, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((classfrac_rowwave<XT, 2, T>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    else
        hipLaunchKernelGGL((classfrac_rowwave<XT, 1, T>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    return REMAP_OK;
}

template <typename XT, int T>
int launch(FracParams &p, hipStream_t stream)
{
    if (p.k_inner >= kWave)
        return launch_rowwave<XT, T>(p, stream);
    p.rows_per_block = kBlock / static_cast<uint32_t>(p.k_inner);
    // (n_rows < 2^31: the blocks fit grid.x)
    const dim3 grid(static_cast<unsigned>(
        (p.n_rows + p.rows_per_block - 1) / p.rows_per_block));
    hipLaunchKernelGGL((classfrac_rowlane<XT, T>), grid, dim3(kBlock), 0,
                       stream, p);
    return REMAP_OK;
}

template <typename XT>
int launch_tile(FracParams &p, hipStream_t stream)
{
    if (p.n_classes <= 4)
        return launch<XT, 4>(p, stream);
    if (p.n_classes <= 8)
        return launch<XT, 8>(p, stream);
    return launch<XT, kTile>(p, stream);
}

// remap_apply_f64 with mode == REMAP_MODE_CLASSFRAC, behind its argument
// checks
inline int apply(const remap_apply_args *a, hipStream_t stream)
{
    FracParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (a->x_batch_stride != 0)
        return fail(REMAP_ERR_ARG,
                    "%s: REMAP_MODE_CLASSFRAC reads ONE batch of class "
                    "indices: x_batch_stride is %lld, expected 0 (n_batch is "
                    "the number of classes)", kName,
                    (long long)a->x_batch_stride);
    if (a->n_batch > kMaxClasses)
        return fail(REMAP_ERR_ARG,
                    "%s: REMAP_MODE_CLASSFRAC serves 1 to %lld classes "
                    "(n_batch), not %lld", kName, (long long)kMaxClasses,
                    (long long)a->n_batch);
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
    p.n_classes = static_cast<int32_t>(a->n_batch);
    p.rows_per_block = 0;
    const int rc = a->x_dtype == REMAP_DTYPE_F64
                       ? launch_tile<double>(p, stream)
                       : launch_tile<float>(p, stream);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace classfrac
}  // namespace remap

#endif  // REMAP_APPLY_CLASSFRAC_H
