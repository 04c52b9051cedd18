// rowpass.h -- what the passes that walk the rows of the plan's CSR beside
// the SpMM apply share (remap_limit.hip, remap_sgs.hip, remap_vector.hip,
// remap_levels.hip, remap_layers.hip, and apply_laf.h, apply_rowstat.h,
// apply_classfrac.h and apply_cotangent.h, the
// modes of the apply itself that are such passes): the checks of their
// argument structs, the addressing of a source cell, the packed loads and
// stores, and the work list of the rowwave form.  A pass comes in two forms
// (remap_levels.hip and
// remap_layers.hip have the first alone, and have it, their parameters and
// their launch from colpass.h, which stands on this header):
//   rowlane  one lane per (row, column), for runs shorter than a wave;
//   rowwave  one wave per (row, chunk of kWave * VEC contiguous columns),
//            lanes across the columns, for runs of >= kWave columns.  The
//            waves of a block hold adjacent rows of one chunk (chunk-major
//            work list): they share source cells in L1; blocks are dealt
//            round-robin over the 8 XCDs, so blockIdx % 8 labels the XCD and
//            every label takes a contiguous range of the work list: the rows
//            one L2 sees are neighbours too.  VEC = 2: 16-byte loads and
//            stores of fp64 (even strides and run lengths, aligned pointers).
#ifndef REMAP_ROWPASS_H
#define REMAP_ROWPASS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"

namespace remap {
namespace rowpass {

// P, below: a pass's kernel parameters, a struct with the members
//   const int64_t *rowptr;  const int32_t *col;
//   int64_t row_begin, n_rows;      rows [row_begin, row_begin + n_rows)
//   int64_t K, k_inner;             K = n_batch * k_inner
//   int64_t ldx, bsx, ldy, bsy;     row and batch strides of X and Y
//   int64_t src_outer;  uint32_t src_fold;      (x_outer_stride, x_src_fold)
//   int64_t total;                  n_rows * K
// among its own, in its own order.  (A base struct would state them once,
// but it moves them to the front of the kernel arguments, and the scalar
// registers the kernels take follow that layout.)

// The checks remap_limit_args, remap_sgs_args, remap_vector_args,
// remap_levels_args and remap_layers_args share, under the entry point's
// name `fn`; fills `p`.  `empty`: the arguments are
// fine and there is nothing to do.
template <typename Args, typename P>
int check_args(const char *fn, const Args &a, P &p, bool &empty)
{
    const remap_csr &A = a.A;
    empty = false;
    if (A.n_rows < 0 || A.n_cols < 0 || A.nnz < 0 ||
        A.n_cols > INT32_MAX || A.n_rows > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "%s: a (%lld, %lld) matrix of %lld entries: expected "
                    "sizes in [0, 2^31)", fn, (long long)A.n_rows,
                    (long long)A.n_cols, (long long)A.nnz);
    if (a.row_begin < 0 || a.row_end < a.row_begin || a.row_end > A.n_rows)
        return fail(REMAP_ERR_ARG,
                    "%s: rows [%lld, %lld) are not inside [0, %lld]", fn,
                    (long long)a.row_begin, (long long)a.row_end,
                    (long long)A.n_rows);
    if (a.n_batch < 0 || a.k_inner < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: n_batch %lld, k_inner %lld: expected >= 0", fn,
                    (long long)a.n_batch, (long long)a.k_inner);
    if (a.x_dtype != REMAP_DTYPE_F64 && a.x_dtype != REMAP_DTYPE_F32)
        return fail(REMAP_ERR_ARG, "%s: x_dtype %d is no REMAP_DTYPE_*", fn,
                    a.x_dtype);
    if (a.x_row_stride < 0 || a.x_batch_stride < 0 || a.y_row_stride < 0 ||
        a.y_batch_stride < 0)
        return fail(REMAP_ERR_ARG, "%s: a negative stride", fn);
    if (a.x_src_fold < 0 || a.x_src_fold >= (int64_t(1) << 31) ||
        (a.x_src_fold != 0 &&
         (a.x_outer_stride < 0 || A.n_cols % a.x_src_fold != 0)))
        return fail(REMAP_ERR_ARG,
                    "%s: x_src_fold = %lld does not divide the %lld source "
                    "cells", fn, (long long)a.x_src_fold,
                    (long long)A.n_cols);
    const int64_t n_rows = a.row_end - a.row_begin;
    if (n_rows == 0 || a.n_batch == 0 || a.k_inner == 0) {
        empty = true;
        return REMAP_OK;
    }
    const int64_t K = a.n_batch > INT32_MAX || a.k_inner > INT32_MAX
                          ? INT64_MAX : a.n_batch * a.k_inner;
    if (K > (INT64_MAX / kBlock) / n_rows)
        return fail(REMAP_ERR_ARG,
                    "%s: %lld rows of %lld x %lld columns are more than one "
                    "launch serves", fn, (long long)n_rows,
                    (long long)a.n_batch, (long long)a.k_inner);
    const int64_t total = n_rows * K;
    if ((total + kBlock - 1) / kBlock > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "%s: %lld elements are more than one launch serves", fn,
                    (long long)total);
    p.rowptr = A.rowptr;
    p.col = A.col;
    p.row_begin = a.row_begin;
    p.n_rows = n_rows;
    p.K = K;
    p.k_inner = a.k_inner;
    p.ldx = a.x_row_stride;
    p.bsx = a.x_batch_stride;
    p.ldy = a.y_row_stride;
    p.bsy = a.y_batch_stride;
    p.src_outer = a.x_outer_stride;
    p.src_fold = static_cast<uint32_t>(a.x_src_fold);
    p.total = total;
    return REMAP_OK;
}

// blocks of the rowlane form: a lane per element
inline dim3 rowlane_grid(int64_t total)
{
    return dim3(static_cast<unsigned>((total + kBlock - 1) / kBlock));
}

// the type the rowlane form splits its flat index in: 32 bits where total
// fits (the 64-bit division is a long instruction sequence).
// REMAP_ROWPASS_WIDE_INDEX: the tests' build of the library
// (_build.build_wide_index_library), which takes the 64-bit instantiations on
// problems of any size; the product is built without it.
template <typename P>
inline bool narrow_index(const P &p)
{
#ifdef REMAP_ROWPASS_WIDE_INDEX
    (void)p;
    return false;
#else
    return p.total <= static_cast<int64_t>(UINT32_MAX);
#endif
}

// Element offsets of source cell a in N arrays of row strides ld and outer
// strides outer (x_src_fold of the argument structs: the cell is split into
// (a / fold, a % fold); fold == 0: one stride, no split).  One division
// serves every array that is addressed by source cell.
template <typename P, int N>
__device__ inline void cell_offsets(const P &p, int32_t a,
                                    const int64_t (&ld)[N],
                                    const int64_t (&outer)[N],
                                    int64_t (&off)[N])
{
    if (p.src_fold == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n)
            off[n] = static_cast<int64_t>(a) * ld[n];
        return;
    }
    const uint32_t y = static_cast<uint32_t>(a) / p.src_fold;
    const uint32_t x = static_cast<uint32_t>(a) - y * p.src_fold;
#pragma unroll
    for (int n = 0; n < N; ++n)
        off[n] = static_cast<int64_t>(y) * outer[n] +
                 static_cast<int64_t>(x) * ld[n];
}

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
    T v[VEC];
};

typedef double Double2 __attribute__((ext_vector_type(2)));

// Touched once: read and written past the caches' keep (non-temporal), as
// the apply kernels write Y.
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

// (a pointer that is not given is aligned)
inline bool aligned_to(const void *ptr, size_t bytes)
{
    return ptr == nullptr || reinterpret_cast<uintptr_t>(ptr) % bytes == 0;
}

// VEC = 2 as far as the shared strides decide it
template <typename P>
inline bool even_strides(const P &p)
{
    return p.k_inner % 2 == 0 && p.ldx % 2 == 0 && p.bsx % 2 == 0 &&
           p.ldy % 2 == 0 && p.bsy % 2 == 0 && p.src_outer % 2 == 0;
}

// the launch of the rowwave form
struct WaveGrid {
    int64_t n_waves, chunks, per_xcd;
    dim3 grid;
};

template <typename P>
inline int rowwave_grid(const char *fn, const P &p, int64_t n_batch,
                        int vec, WaveGrid &g)
{
    g.chunks = (p.k_inner + kWave * vec - 1) / (kWave * vec);
    // (n_rows * n_batch * k_inner was checked against INT64_MAX / kBlock)
    g.n_waves = p.n_rows * n_batch * g.chunks;
    const int64_t n_blocks = (g.n_waves + kWavesPerBlock - 1) /
                             kWavesPerBlock;
    // (whole rounds of the 8 XCDs; the waves past n_waves leave at once)
    g.per_xcd = (n_blocks + kXcds - 1) / kXcds;
    if (g.per_xcd * kXcds > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "%s: %lld elements are more than one launch serves", fn,
                    (long long)p.total);
    g.grid = dim3(static_cast<unsigned>(g.per_xcd * kXcds));
    return REMAP_OK;
}

// The calling wave's place w in the work list: physical block -> logical
// block, a contiguous range for every XCD.  Places from n_waves on hold
// nothing.  A kernel splits its place, chunk-major, into
//   cb = w / n_rows, r = w - cb * n_rows     row r (from row_begin)
//   b = cb / chunks, chunk = cb - b * chunks batch b
//   k = chunk * (kWave * VEC) + lane * VEC   columns [k, k + VEC)
// and leaves where k >= k_inner (VEC = 2: k_inner is even).  (The split
// stands in the kernels: behind a call, inlined or not, the compiler loads
// the kernel's parameters only after the two divisions.)
__device__ inline int64_t rowwave_place(int64_t per_xcd)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t L = (int64_t)(blockIdx.x & (kXcds - 1)) * per_xcd +
                      (blockIdx.x >> 3);
    return L * kWavesPerBlock + wave;
}

}  // namespace rowpass
}  // namespace remap

#endif  // REMAP_ROWPASS_H
