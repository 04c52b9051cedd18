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

namespace remap {
namespace {

constexpr int kUnroll = 8;
constexpr int64_t kRowsFastRun = 4;   // (engine.CELL_MAX_RUN)

struct LimitParams {
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

// element offset of source cell a (remap_limit_args.x_src_fold)
__device__ inline int64_t cell_offset(const LimitParams &p, int32_t a)
{
    if (p.src_fold == 0)
        return static_cast<int64_t>(a) * p.ldx;
    const uint32_t y = static_cast<uint32_t>(a) / p.src_fold;
    const uint32_t x = static_cast<uint32_t>(a) - y * p.src_fold;
    return static_cast<int64_t>(y) * p.src_outer +
           static_cast<int64_t>(x) * p.ldx;
}

// IT: the type the flat index is split in (32 bits where total fits: the
// 64-bit division is a long instruction sequence)
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
            xs[u] = X[cell_offset(p, c[u])];
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
// across the columns, as spmm_rowwave.h -- for runs of >= kWave columns.  The
// row is the same in every lane, so the row pointers and the column indices
// are scalar loads, the loop over the row's entries is wave-uniform and reads
// exactly the row's entries (no clamped duplicates), UNR source runs in
// flight at a time; VEC = 2: 16-byte loads and stores of fp64 (even strides
// and run lengths, aligned pointers).  The waves of a block hold adjacent
// rows of one chunk (chunk-major work list): they share source cells in L1;
// blocks are dealt round-robin over the 8 XCDs, so blockIdx % 8 labels the
// XCD and every label takes a contiguous range of the work list: the rows
// one L2 sees are neighbours too.  Y, lo and hi are touched once: they are
// read and written past the caches' keep (non-temporal), as the apply
// kernels write Y.
// ---------------------------------------------------------------------------
template <typename XT, int VEC>
struct alignas(sizeof(XT) * VEC) Pack {
    XT v[VEC];
};

struct Bounds {
    double lo, hi;
    bool has;
};

typedef double Double2 __attribute__((ext_vector_type(2)));

template <int VEC>
__device__ inline Pack<double, VEC> load_once(const double *ptr)
{
    Pack<double, VEC> out;
    if constexpr (VEC == 2) {
        const Double2 t = __builtin_nontemporal_load(
            reinterpret_cast<const Double2 *>(ptr));
        out.v[0] = t.x;
        out.v[1] = t.y;
    } else {
        out.v[0] = __builtin_nontemporal_load(ptr);
    }
    return out;
}

template <int VEC>
__device__ inline void store_once(double *ptr, const Pack<double, VEC> &v)
{
    if constexpr (VEC == 2) {
        Double2 t;
        t.x = v.v[0];
        t.y = v.v[1];
        __builtin_nontemporal_store(t, reinterpret_cast<Double2 *>(ptr));
    } else {
        __builtin_nontemporal_store(v.v[0], ptr);
    }
}

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
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // physical block -> logical block: a contiguous range for every XCD
    const int64_t L = (int64_t)(blockIdx.x & (kXcds - 1)) * per_xcd +
                      (blockIdx.x >> 3);
    const int64_t w = L * kWavesPerBlock + wave;
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
                X + cell_offset(p, p.col[j + u]));
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                widen(bd[v], static_cast<double>(xs[u].v[v]));
    }
    for (; j < e; ++j) {
        const PX x = *reinterpret_cast<const PX *>(
            X + cell_offset(p, p.col[j]));
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

inline bool aligned_to(const void *ptr, size_t bytes)
{
    return ptr == nullptr || reinterpret_cast<uintptr_t>(ptr) % bytes == 0;
}

template <typename XT>
int launch_rowwave(const LimitParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = p.k_inner % 2 == 0 && p.ldx % 2 == 0 &&
                      p.bsx % 2 == 0 && p.ldy % 2 == 0 && p.bsy % 2 == 0 &&
                      p.src_outer % 2 == 0 &&
                      aligned_to(p.X, 2 * sizeof(XT)) &&
                      aligned_to(p.Y, 16) && aligned_to(p.lo, 16) &&
                      aligned_to(p.hi, 16);
    const int vec = even ? 2 : 1;
    const int64_t chunks = (p.k_inner + kWave * vec - 1) / (kWave * vec);
    // (n_rows * n_batch * k_inner was checked against INT64_MAX / kBlock)
    const int64_t n_waves = p.n_rows * n_batch * chunks;
    const int64_t n_blocks = (n_waves + kWavesPerBlock - 1) / kWavesPerBlock;
    // (whole rounds of the 8 XCDs; the waves past n_waves leave at once)
    const int64_t per_xcd = (n_blocks + kXcds - 1) / kXcds;
    if (per_xcd * kXcds > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: %lld elements are more than one "
                    "launch serves", (long long)p.total);
    const dim3 grid(static_cast<unsigned>(per_xcd * kXcds));
    if (even)
        hipLaunchKernelGGL((limit_rowwave<XT, 2>), grid, dim3(kBlock), 0,
                           stream, p, n_waves, chunks, per_xcd);
    else
        hipLaunchKernelGGL((limit_rowwave<XT, 1>), grid, dim3(kBlock), 0,
                           stream, p, n_waves, chunks, per_xcd);
    return REMAP_OK;
}

template <typename XT, typename IT>
void launch_limit(const LimitParams &p, bool rows_fast, unsigned n_blocks,
                  hipStream_t stream)
{
    if (rows_fast)
        hipLaunchKernelGGL((limit_rowlane<XT, IT, true>), dim3(n_blocks),
                           dim3(kBlock), 0, stream, p);
    else
        hipLaunchKernelGGL((limit_rowlane<XT, IT, false>), dim3(n_blocks),
                           dim3(kBlock), 0, stream, p);
}

}  // namespace

int limit_rows(const remap_limit_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "remap_limit_rows: NULL args");
    const remap_csr &A = a->A;
    if (A.n_rows < 0 || A.n_cols < 0 || A.nnz < 0 ||
        A.n_cols > INT32_MAX || A.n_rows > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: a (%lld, %lld) matrix of %lld "
                    "entries: expected sizes in [0, 2^31)",
                    (long long)A.n_rows, (long long)A.n_cols,
                    (long long)A.nnz);
    if (a->row_begin < 0 || a->row_end < a->row_begin ||
        a->row_end > A.n_rows)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: rows [%lld, %lld) are not inside "
                    "[0, %lld]", (long long)a->row_begin,
                    (long long)a->row_end, (long long)A.n_rows);
    if (a->n_batch < 0 || a->k_inner < 0)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: n_batch %lld, k_inner %lld: expected "
                    ">= 0", (long long)a->n_batch, (long long)a->k_inner);
    if (a->x_dtype != REMAP_DTYPE_F64 && a->x_dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "remap_limit_rows: x_dtype %d is no "
                                   "REMAP_DTYPE_*", a->x_dtype);
    if (a->x_row_stride < 0 || a->x_batch_stride < 0 ||
        a->y_row_stride < 0 || a->y_batch_stride < 0)
        return fail(REMAP_ERR_ARG, "remap_limit_rows: a negative stride");
    if (a->x_src_fold < 0 || a->x_src_fold >= (int64_t(1) << 31) ||
        (a->x_src_fold != 0 &&
         (a->x_outer_stride < 0 || A.n_cols % a->x_src_fold != 0)))
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: x_src_fold = %lld does not divide the "
                    "%lld source cells", (long long)a->x_src_fold,
                    (long long)A.n_cols);
    const int64_t n_rows = a->row_end - a->row_begin;
    if (n_rows == 0 || a->n_batch == 0 || a->k_inner == 0)
        return REMAP_OK;
    const int64_t K = a->n_batch > INT32_MAX || a->k_inner > INT32_MAX
                          ? INT64_MAX : a->n_batch * a->k_inner;
    if (K > (INT64_MAX / kBlock) / n_rows)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: %lld rows of %lld x %lld columns are "
                    "more than one launch serves", (long long)n_rows,
                    (long long)a->n_batch, (long long)a->k_inner);
    if (!A.rowptr || (A.nnz > 0 && !A.col) || !a->X || !a->Y)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: NULL rowptr, col, X or Y");
    const int64_t total = n_rows * K;
    const int64_t n_blocks = (total + kBlock - 1) / kBlock;
    if (n_blocks > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_limit_rows: %lld elements are more than one "
                    "launch serves", (long long)total);
    LimitParams p;
    p.rowptr = A.rowptr;
    p.col = A.col;
    p.X = a->X;
    p.Y = a->Y;
    p.lo = a->lo;
    p.hi = a->hi;
    p.row_begin = a->row_begin;
    p.n_rows = n_rows;
    p.K = K;
    p.k_inner = a->k_inner;
    p.ldx = a->x_row_stride;
    p.bsx = a->x_batch_stride;
    p.ldy = a->y_row_stride;
    p.bsy = a->y_batch_stride;
    p.src_outer = a->x_outer_stride;
    p.src_fold = static_cast<uint32_t>(a->x_src_fold);
    p.total = total;
    // short runs in several batches whose rows lie closer than its batches:
    // neighbouring lanes take neighbouring rows
    const bool rows_fast = a->k_inner < kRowsFastRun && a->n_batch > 1 &&
                           a->y_row_stride <= a->y_batch_stride;
    const bool narrow = total <= static_cast<int64_t>(UINT32_MAX);
    const unsigned nb = static_cast<unsigned>(n_blocks);
    if (a->k_inner >= kWave) {
        // runs of a wave's width and more: a wave per (row, chunk)
        const int rc = a->x_dtype == REMAP_DTYPE_F64
                           ? launch_rowwave<double>(p, a->n_batch, stream)
                           : launch_rowwave<float>(p, a->n_batch, stream);
        if (rc != REMAP_OK)
            return rc;
    } else if (a->x_dtype == REMAP_DTYPE_F64) {
        if (narrow)
            launch_limit<double, uint32_t>(p, rows_fast, nb, stream);
        else
            launch_limit<double, int64_t>(p, rows_fast, nb, stream);
    } else {
        if (narrow)
            launch_limit<float, uint32_t>(p, rows_fast, nb, stream);
        else
            launch_limit<float, int64_t>(p, rows_fast, nb, stream);
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

}  // extern "C"
