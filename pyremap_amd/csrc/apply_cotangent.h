// apply_cotangent.h -- REMAP_MODE_COTAN_FRACB and REMAP_MODE_COTAN_MASKED of
// remap_apply_f64: the cotangent of the division, the first step of the
// adjoint apply.  The forward modes end in one division per destination
// element, y = num / den; what reaches num from a cotangent G of y is G / den
// where the forward divided and nothing where it wrote NaN.  The transposed
// sum that follows is REMAP_MODE_RAW applied with the plan of S^T
// (engine.RemapPlan.transposed), which the SpMM families serve as they serve
// S; the one thing they cannot do is give the masked mode's denominator apart
// from the quotient, and that is this file.  Included by remap_spmm.hip;
// stands on rowpass.h; the forms and the launch decisions are apply_rowstat.h's.
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.adjoint is the
// same statement in numpy).  S is the plan's CSR, X the forward's field, G the
// cotangent in the layout of the forward's result, T what this pass leaves in
// its place.  For destination element (i, b, k):
//   REMAP_MODE_COTAN_FRACB (forward REMAP_MODE_FRACB):
//   T = frac_b_i > 0 ? G / frac_b_i : +0.0
//   REMAP_MODE_COTAN_MASKED (forward REMAP_MODE_MASKED):
//   den starts at +0.0; for the entries j of row i, in CSR order,
//   den = den + S_j iff X[cell(col_j), b, k] is no NaN, each sum rounded
//   (the forward's own den)
//   T = den > threshold ? G / den : +0.0, one IEEE division
//   a masked element is a selection, not a product: where the forward wrote
//   NaN, G is not looked at, even if it is NaN
// (Forward REMAP_MODE_RAW: T = G, no pass.)  The transposed sum, for source
// element (j, b, k) over the entries i of row j of S^T in ascending i:
//   acc starts at +0.0; acc = acc + (S_ij * T_i), the product rounded, then
//   the sum; no FMA; an empty column gives +0.0
// and, behind a masked forward, gX = +0.0 where X is NaN.
//
// The arguments are read in their own way: Y holds G on entry and T on exit,
// every element read once and then written once by the lane that owns it; X
// is read for NaN only (mode 16 does not read it).  Nothing is multiplied: a
// sum of the row's weights, a comparison and one division, so two runs and the
// two forms give the same bytes.
//
// Two forms, as apply_rowstat.h has them:
//   rowlane  one lane per (row, column), for runs shorter than a wave,
//            columns fastest across the lanes, or rows for runs shorter than
//            kRowsFastRun in several batches;
//   rowwave  one wave per (row, chunk of kWave * VEC columns) for
//            k_inner >= kWave: col and val are wave-uniform scalar loads, G
//            comes in through load_once and T leaves through store_once, 16
//            bytes a lane where strides and pointers are even.
// Registers and global memory only: no workgroup memory, no read-modify-write
// of memory beyond the element's own load and store.
#ifndef REMAP_APPLY_COTANGENT_H
#define REMAP_APPLY_COTANGENT_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace cotangent {

using namespace rowpass;

constexpr char kName[] = "remap_apply_f64";
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)
constexpr unsigned kMaxGridY = 65535;

struct CotanParams {                // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ X;
    double *Y;                      // G in, T out
    const double *__restrict__ frac_b;
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

__device__ inline bool gate_closed(const CotanParams &p)
{
    return p.gate != nullptr && *p.gate != p.gate_value;
}

// element offset of source cell a in X
__device__ inline int64_t x_offset(const CotanParams &p, int32_t a)
{
    int64_t o[1];
    cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

// The forward's den of VEC neighbouring elements over entries [s, e), four
// gathers in flight.  (The index of a gather past the end is the last
// entry's: one code path for every length, nothing read outside the row.)
template <typename XT, int VEC>
__device__ inline void denominator(const CotanParams &p,
                                   const XT *__restrict__ X, int64_t s,
                                   int64_t e, double (&den)[VEC])
{
    constexpr int UNR = 4;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        den[v] = 0.0;
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double w[UNR];
        Pack<XT, VEC> xs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            w[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            xs[u] = *reinterpret_cast<const Pack<XT, VEC> *>(
                X + x_offset(p, c[u]));
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const XT x = xs[u].v[v];
                    const double sum = den[v] + w[u];
                    den[v] = x == x ? sum : den[v];
                }
            }
    }
}

// What VEC neighbouring elements of row i divide by, and above what: MASKED
// the forward's den and the threshold, else frac_b_i and 0.
template <bool MASKED, typename XT, int VEC>
__device__ inline void divisor(const CotanParams &p, const XT *__restrict__ X,
                               int64_t i, double (&den)[VEC], double &above)
{
    if constexpr (MASKED) {
        denominator<XT, VEC>(p, X, p.rowptr[i], p.rowptr[i + 1], den);
        above = p.thr;
    } else {
        const double f = p.frac_b[i];
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            den[v] = f;
        above = 0.0;
    }
}

// G -> T at Y + o
template <int VEC>
__device__ inline void divide(double *y, const double (&den)[VEC],
                              double above)
{
    const Pack<double, VEC> g = load_once<VEC>(y);
    Pack<double, VEC> t;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const double q = g.v[v] / den[v];
        t.v[v] = den[v] > above ? q : 0.0;
    }
    store_once<VEC>(y, t);
}

// ---------------------------------------------------------------------------
// rowlane: one lane per (row, column).  ROWS_FAST: thread -> row, blockIdx.y
// (and a loop) -> flat column; else the block is rows_per_block rows of
// cols_per_block columns, blockIdx.y (and a loop) the column tile.
// ---------------------------------------------------------------------------
template <bool MASKED, typename XT>
__device__ inline void lane_element(const CotanParams &p, int64_t i,
                                    uint32_t kf)
{
    const uint32_t ki = static_cast<uint32_t>(p.k_inner);
    const uint32_t b = kf / ki;
    const uint32_t k = kf - b * ki;
    const XT *__restrict__ X = static_cast<const XT *>(p.X) +
                               static_cast<int64_t>(b) * p.bsx +
                               static_cast<int64_t>(k);
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    double den[1], above;
    divisor<MASKED, XT, 1>(p, X, i, den, above);
    divide<1>(p.Y + o, den, above);
}

template <bool MASKED, typename XT, bool ROWS_FAST>
__global__ __launch_bounds__(kBlock) void cotan_rowlane(const CotanParams p)
{
    if (gate_closed(p))
        return;
    const uint32_t K = static_cast<uint32_t>(p.K);
    if constexpr (ROWS_FAST) {
        const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (r >= p.n_rows)
            return;
        for (uint32_t kf = blockIdx.y; kf < K; kf += gridDim.y)
            lane_element<MASKED, XT>(p, p.row_begin + r, kf);
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
            lane_element<MASKED, XT>(p, p.row_begin + r,
                                     static_cast<uint32_t>(kf));
    }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns; the work list and VEC are rowpass.h's.  The row is the
// same in every lane: the row pointers, the column indices, the weights and
// frac_b are scalar loads and the loop over the row's entries is wave-uniform.
// ---------------------------------------------------------------------------
template <bool MASKED, typename XT, int VEC>
__global__ __launch_bounds__(kBlock) void cotan_rowwave(const CotanParams p,
                                                        const int64_t n_waves,
                                                        const int64_t chunks,
                                                        const int64_t per_xcd)
{
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
    double den[VEC], above;
    divisor<MASKED, XT, VEC>(p, X, i, den, above);
    divide<VEC>(p.Y + o, den, above);
}

template <bool MASKED, typename XT>
int launch_rowwave(const CotanParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((cotan_rowwave<MASKED, XT, 2>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    else
        hipLaunchKernelGGL((cotan_rowwave<MASKED, XT, 1>), g.grid,
                           dim3(kBlock), 0, stream, p, g.n_waves, g.chunks,
                           g.per_xcd);
    return REMAP_OK;
}

template <bool MASKED, typename XT>
void launch_rowlane(CotanParams &p, bool rows_fast, hipStream_t stream)
{
    if (rows_fast) {
        const dim3 grid(
            static_cast<unsigned>((p.n_rows + kBlock - 1) / kBlock),
            static_cast<unsigned>(p.K < kMaxGridY ? p.K : kMaxGridY));
        hipLaunchKernelGGL((cotan_rowlane<MASKED, XT, true>), grid,
                           dim3(kBlock), 0, stream, p);
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
    hipLaunchKernelGGL((cotan_rowlane<MASKED, XT, false>), grid, dim3(kBlock),
                       0, stream, p);
}

template <bool MASKED, typename XT>
int launch(CotanParams &p, const remap_apply_args *a, hipStream_t stream)
{
    if (a->k_inner >= kWave)
        return launch_rowwave<MASKED, XT>(p, a->n_batch, stream);
    // short runs in several batches whose rows lie closer than its batches:
    // neighbouring lanes take neighbouring rows
    const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                           a->y_row_stride <= a->y_batch_stride;
    launch_rowlane<MASKED, XT>(p, rows_fast, stream);
    return REMAP_OK;
}

// remap_apply_f64 with mode REMAP_MODE_COTAN_FRACB or _COTAN_MASKED, behind
// its argument checks
inline int apply(const remap_apply_args *a, hipStream_t stream)
{
    CotanParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    const bool masked = a->mode == REMAP_MODE_COTAN_MASKED;
    if (a->mask_out)
        return fail(REMAP_ERR_ARG,
                    "%s: mode %d (a cotangent) writes no mask: mask_out must "
                    "be NULL", kName, a->mode);
    if (!masked && !a->frac_b)
        return fail(REMAP_ERR_ARG,
                    "%s: REMAP_MODE_COTAN_FRACB needs frac_b", kName);
    // (n_rows < 2^31: the blocks of either form fit grid.x)
    if (p.K >= (int64_t(1) << 31))
        return fail(REMAP_ERR_ARG,
                    "%s: %lld x %lld columns are more than one launch "
                    "serves", kName, (long long)a->n_batch,
                    (long long)a->k_inner);
    p.val = a->A.val;
    p.X = a->X;
    p.Y = a->Y;
    p.frac_b = a->frac_b;
    p.gate = a->gate;
    p.gate_value = a->gate_value;
    p.thr = a->threshold;
    p.cols_per_block = p.rows_per_block = 0;
    int rc = REMAP_OK;
    if (!masked) {
        // a scaled copy: X is not read, its strides decide nothing
        p.X = nullptr;
        p.ldx = p.bsx = p.src_outer = 0;
        p.src_fold = 0;
        rc = launch<false, double>(p, a, stream);
    } else if (a->x_dtype == REMAP_DTYPE_F64) {
        rc = launch<true, double>(p, a, stream);
    } else {
        rc = launch<true, float>(p, a, stream);
    }
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace cotangent
}  // namespace remap

#endif  // REMAP_APPLY_COTANGENT_H
