// The host toolkit of the weight kernels (remap_overlap.hip, remap_nearest.hip,
// remap_locate.hip, remap_quads.hip, remap_patch.hip, remap_conserve2nd.hip,
// remap_geometry.hip, remap_expand.hip, remap_tree.h): every launch, rocPRIM
// call, workspace pointer, read-back and phase timing of these files goes
// through the helpers below.  Each returns REMAP_OK or what fail() gave.
#ifndef REMAP_HOST_H
#define REMAP_HOST_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string.h>   // (rocPRIM calls the global memset)

#include <rocprim/rocprim.hpp>

#include "remap_common.h"

namespace remap {
namespace {

constexpr size_t kAlign = 256;
size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

uint32_t blocks(int64_t n, int per) { return static_cast<uint32_t>((n + per - 1) / per); }
// (no buffer and no rocPRIM call is sized 0)
size_t at_least_one(int64_t n) { return static_cast<size_t>(n > 0 ? n : 1); }

#define REMAP_TRY(expr)                                         \
    do {                                                        \
        const int rc__ = (expr);                                \
        if (rc__ != REMAP_OK)                                   \
            return rc__;                                        \
    } while (0)

// one lane per item in blocks of `block`; nothing to launch for no items
template <class... P, class... A>
int launch(void (*kernel)(P...), int64_t n_items, int block,
           hipStream_t stream, A... args)
{
    if (n_items <= 0)
        return REMAP_OK;
    hipLaunchKernelGGL(kernel, dim3(blocks(n_items, block)), dim3(block), 0,
                       stream, static_cast<P>(args)...);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

// n_blocks blocks of `block` lanes with lds_bytes of dynamic LDS each (a
// block that serves another number of items than it has lanes, a walk's
// stack); n_blocks >= 1 is the caller's
template <class... P, class... A>
int launch_blocks(void (*kernel)(P...), uint32_t n_blocks, int block,
                  size_t lds_bytes, hipStream_t stream, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(block), lds_bytes, stream,
                       static_cast<P>(args)...);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

template <class T>
T *at(char *ws, size_t off)
{
    return reinterpret_cast<T *>(ws + off);
}

// a word of a counter block as what a kernel writes there
template <class T, class U>
T *as(U *word)
{
    return reinterpret_cast<T *>(word);
}

// bytes from the device, waited for
int read_back(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    REMAP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost,
                                   stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    return REMAP_OK;
}

// the next field of a workspace layout: its offset, *off moved past it
size_t take(size_t *off, size_t bytes)
{
    const size_t at = *off;
    *off += align_up(bytes);
    return at;
}

// the refusal of a missing or short workspace
int need_workspace(const char *name, const void *workspace, size_t have,
                   size_t need)
{
    if (!workspace || have < need)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need %zu", name, have, need);
    return REMAP_OK;
}

// rocPRIM, typed; *_temp: the bytes of temporary storage n items need.  The
// sorts take the key bits [0, end_bit): every bit of the key type unless the
// caller knows its keys to be shorter
template <class T>
int exclusive_scan(void *temp, size_t temp_bytes, const T *in, T *out,
                   int64_t n, hipStream_t stream)
{
    REMAP_HIP_CHECK((rocprim::exclusive_scan(temp, temp_bytes, in, out, T(0),
                                             static_cast<size_t>(n),
                                             rocprim::plus<T>(), stream)));
    return REMAP_OK;
}

template <class T>
int scan_temp(size_t n, size_t *bytes)
{
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, *bytes, static_cast<const T *>(nullptr),
        static_cast<T *>(nullptr), T(0), n, rocprim::plus<T>())));
    return REMAP_OK;
}

// (templates, the keys' type included, so that a file holds the rocPRIM
// kernels of the calls it makes and no others)
template <class K>
int radix_sort_keys(void *temp, size_t temp_bytes, const K *in, K *out,
                    int64_t n, hipStream_t stream,
                    unsigned end_bit = 8 * sizeof(K))
{
    REMAP_HIP_CHECK((rocprim::radix_sort_keys(temp, temp_bytes, in, out,
                                              static_cast<size_t>(n), 0u,
                                              end_bit, stream)));
    return REMAP_OK;
}

template <class K = uint64_t>
int sort_keys_temp(size_t n, size_t *bytes, unsigned end_bit = 8 * sizeof(K))
{
    REMAP_HIP_CHECK((rocprim::radix_sort_keys(
        nullptr, *bytes, static_cast<const K *>(nullptr),
        static_cast<K *>(nullptr), n, 0u, end_bit)));
    return REMAP_OK;
}

// K: uint64_t or uint32_t keys; V: double (areas, values) or uint32_t
// (positions)
template <class K, class V>
int radix_sort_pairs(void *temp, size_t temp_bytes, const K *keys_in,
                     K *keys_out, const V *in, V *out, int64_t n,
                     hipStream_t stream, unsigned end_bit = 8 * sizeof(K))
{
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        temp, temp_bytes, keys_in, keys_out, in, out, static_cast<size_t>(n),
        0u, end_bit, stream)));
    return REMAP_OK;
}

template <class V, class K = uint64_t>
int sort_pairs_temp(size_t n, size_t *bytes, unsigned end_bit = 8 * sizeof(K))
{
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        nullptr, *bytes, static_cast<const K *>(nullptr),
        static_cast<K *>(nullptr), static_cast<const V *>(nullptr),
        static_cast<V *>(nullptr), n, 0u, end_bit)));
    return REMAP_OK;
}

template <class K>
int unique(void *temp, size_t temp_bytes, const K *in, K *out, K *n_unique,
           int64_t n, hipStream_t stream)
{
    REMAP_HIP_CHECK((rocprim::unique(temp, temp_bytes, in, out, n_unique,
                                     static_cast<size_t>(n),
                                     rocprim::equal_to<K>(), stream)));
    return REMAP_OK;
}

template <class K = uint64_t>
int unique_temp(size_t n, size_t *bytes)
{
    REMAP_HIP_CHECK((rocprim::unique(
        nullptr, *bytes, static_cast<const K *>(nullptr),
        static_cast<K *>(nullptr), static_cast<K *>(nullptr), n)));
    return REMAP_OK;
}

// run(ev) records N events around its N - 1 phases on its stream;
// phase_ms[k] is the time from ev[k] to ev[k + 1].  What run gave comes
// first, then the HIP error of the events
template <int N, class Run>
int timed_phases(float *phase_ms, Run run)
{
    hipEvent_t ev[N] = {};
    hipError_t err = hipSuccess;
    for (int k = 0; k < N && err == hipSuccess; ++k)
        err = hipEventCreate(&ev[k]);
    int rc = REMAP_OK;
    if (err == hipSuccess) {
        rc = run(ev);
        if (rc == REMAP_OK)
            err = hipEventSynchronize(ev[N - 1]);
        for (int k = 0; k < N - 1 && rc == REMAP_OK && err == hipSuccess; ++k)
            err = hipEventElapsedTime(&phase_ms[k], ev[k], ev[k + 1]);
    }
    for (int k = 0; k < N; ++k)
        if (ev[k])
            (void)hipEventDestroy(ev[k]);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(err);
    return REMAP_OK;
}

}  // namespace
}  // namespace remap

#endif  // REMAP_HOST_H
