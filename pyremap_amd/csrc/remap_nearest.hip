// remap_nearest.hip -- ESMF's `neareststod` search on the device: for every
// destination point the source point closest in 3-D Cartesian distance, the
// lowest source index on a tie, nobody left unmapped.
//
// Definition (exact, no tolerance).  src_xyz (n_src, 3) and dst_xyz
// (n_dst, 3) are fp64 and finite.  For destination i and source j
//   dx = src[j].x - dst[i].x   (likewise y, z)
//   d2(i, j) = (dx * dx + dy * dy) + dz * dz
// in IEEE fp64 in that order (the library is built -ffp-contract=off), and
// nearest[i] is the j that minimises (d2(i, j), j) lexicographically: the
// smallest d2, and among equal d2 bit patterns the lowest ORIGINAL index.
// The result is a pure function of the inputs; numpy reproduces it bit for
// bit.
//
// Pipeline (all on the caller's stream, nothing synchronises, no atomics):
//   morton_keys   63-bit Morton code of every source point over [-1, 1]^3
//                 (21 bits an axis, clamped: any finite input is served)
//   radix sort    rocPRIM radix_sort_pairs on (key, original index)
//   gather_sorted xyz into sorted order: a leaf's points are contiguous
//   leaf_boxes    level 0 of the tree: one axis-aligned box (lo, hi an axis)
//                 over every run of kLeaf consecutive sorted points
//   upper_boxes   one launch a level: a node's box over its kFan children,
//                 which are consecutive nodes of the level below
//   nearest_walk  one lane per destination point, 64-lane blocks: depth first
//                 from the root, the stack in LDS laid out [entry][lane].  At
//                 an inner node the children's bounds are sorted; the walk
//                 steps into the nearest and stacks the others, farthest
//                 first.  A node whose bound is strictly greater than the
//                 best d2 so far is skipped, when stacked and again when
//                 popped.  At a leaf every point is compared on (d2, index).
//
// Why the pruning is exact in floating point.  The bound of a box for the
// point p is (ex * ex + ey * ey) + ez * ez with ex = max(lo.x - p.x,
// p.x - hi.x, 0) (likewise y, z): d2's own operations in d2's own order.  For
// a source s inside the box lo.x <= s.x <= hi.x, and rounding is monotone, so
// fl(s.x - p.x) >= fl(lo.x - p.x) and fl(p.x - s.x) >= fl(p.x - hi.x); fp
// subtraction is exactly antisymmetric, hence |fl(s.x - p.x)| >= ex >= 0.
// Squaring and adding non-negative numbers keep the order under monotone
// rounding, so fl(bound) <= fl(d2(s)) for every s in the box.  A node is
// dropped only when bound > best (strict), so no point that would win or TIE
// is ever discarded, and the answer depends on neither the traversal order,
// the leaf size, the fan-out nor the sort: only the speed does.  The stack
// keeps a node's bound as a float rounded DOWN (<= the bound): the test at
// the pop prunes a little less than the fp64 bound would, never more.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "remap_common.h"
#include "remap_tree.h"

namespace remap {
namespace {

constexpr int kWalkBlock = 64;
// (kLeaf sorted points a leaf, kFan nodes below a node: remap_tree.h)
// the walk steps into one child and stacks at most kFan - 1 a level above
// level 0, so that bounds the stack whatever the points are.  The launch
// sizes the LDS by the tree at hand (8 bytes an entry and lane): the fewer
// levels, the more walking waves fit beside each other in a CU
constexpr int stack_depth(int levels) { return (kFan - 1) * (levels - 1); }
constexpr uint32_t kNone = 0xffffffffu;   // no node (levels end at 14)
// one walk launch: its block count stays far below the grid limit
constexpr int64_t kWalkChunk = int64_t(1) << 30;

static_assert(kFan == 4, "nearest_walk sorts four children by hand");
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 8 <= 64 * 1024,
              "the walk's stack must fit in a workgroup's LDS");

struct Layout {
    Tree tree;
    size_t keys_in, keys_out, idx_in, idx_out, xyz, boxes, temp, total;
    size_t temp_bytes;
};

int make_layout(int64_t n_src, Layout *lay)
{
    const size_t n = static_cast<size_t>(n_src);
    const int64_t nodes = make_tree(n_src, &lay->tree);
    size_t sort_bytes = 0;
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        nullptr, sort_bytes, static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr),
        static_cast<const uint32_t *>(nullptr),
        static_cast<uint32_t *>(nullptr), n, 0u, 63u)));
    lay->temp_bytes = sort_bytes;
    size_t off = 0;
    lay->keys_in = off;  off += align_up(n * 8);
    lay->keys_out = off; off += align_up(n * 8);
    lay->idx_in = off;   off += align_up(n * 4);
    lay->idx_out = off;  off += align_up(n * 4);
    lay->xyz = off;      off += align_up(n * 24);
    lay->boxes = off;    off += align_up(static_cast<size_t>(nodes) * 48);
    lay->temp = off;     off += align_up(lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

__global__ __launch_bounds__(kBlock) void morton_keys(
    int64_t n, const double *__restrict__ xyz, uint64_t *__restrict__ keys,
    uint32_t *__restrict__ idx)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    keys[k] = morton_key(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
    idx[k] = static_cast<uint32_t>(k);
}

__global__ __launch_bounds__(kBlock) void gather_sorted(
    int64_t n, const double *__restrict__ xyz,
    const uint32_t *__restrict__ idx, double *__restrict__ sorted)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n)
        return;
    const int64_t j = idx[k];
    sorted[3 * k] = xyz[3 * j];
    sorted[3 * k + 1] = xyz[3 * j + 1];
    sorted[3 * k + 2] = xyz[3 * j + 2];
}

// one lane per leaf: the box of its (at most kLeaf) points
__global__ __launch_bounds__(kBlock) void leaf_boxes(
    int64_t n, int64_t n_leaves, const double *__restrict__ sorted,
    double *__restrict__ boxes)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_leaves)
        return;
    const int64_t p0 = k * kLeaf;
    const int64_t p1 = p0 + kLeaf < n ? p0 + kLeaf : n;
    double lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        lo[a] = hi[a] = sorted[3 * p0 + a];
    for (int64_t p = p0 + 1; p < p1; ++p) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = sorted[3 * p + a];
            lo[a] = v < lo[a] ? v : lo[a];
            hi[a] = v > hi[a] ? v : hi[a];
        }
    }
    double *o = boxes + k * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = lo[a];
        o[3 + a] = hi[a];
    }
}

// (upper_boxes, a node's box over its kFan children: remap_tree.h)

// the least d2 any point inside the box can have (see the file's head)
__device__ inline double box_bound(const double *__restrict__ b, double px,
                                   double py, double pz)
{
    const double ex = fmax(fmax(b[0] - px, px - b[3]), 0.0);
    const double ey = fmax(fmax(b[1] - py, py - b[4]), 0.0);
    const double ez = fmax(fmax(b[2] - pz, pz - b[5]), 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}

__device__ inline void order2(double &ba, uint32_t &na, double &bb,
                              uint32_t &nb)
{
    if (bb < ba) {
        const double tb = ba;
        ba = bb;
        bb = tb;
        const uint32_t tn = na;
        na = nb;
        nb = tn;
    }
}

// one lane per destination point
__global__ __launch_bounds__(kWalkBlock) void nearest_walk(
    Tree T, int64_t n_src, const double *__restrict__ sorted,
    const uint32_t *__restrict__ orig, const double *__restrict__ boxes,
    int64_t n_dst, const double *__restrict__ dst,
    int32_t *__restrict__ nearest)
{
    // stack_depth(T.levels) entries a lane: nodes, then their bounds
    extern __shared__ uint32_t stack_lds[];
    uint32_t (*stack_node)[kWalkBlock] =
        reinterpret_cast<uint32_t (*)[kWalkBlock]>(stack_lds);
    float (*stack_bound)[kWalkBlock] = reinterpret_cast<float (*)[kWalkBlock]>(
        stack_lds + stack_depth(T.levels) * kWalkBlock);
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * kWalkBlock + lane;
    if (w >= n_dst)
        return;
    const double px = dst[3 * w], py = dst[3 * w + 1], pz = dst[3 * w + 2];
    double best = __builtin_huge_val();
    uint32_t best_i = 0xffffffffu;
    int top = 0;
    uint32_t cur = static_cast<uint32_t>(T.levels - 1) << kNodeBits;
    bool have = true;
    for (;;) {
        if (!have) {
            if (top == 0)
                break;
            --top;
            // (the float is at most the node's bound: see the file's head)
            if (static_cast<double>(stack_bound[top][lane]) > best)
                continue;
            cur = stack_node[top][lane];
        }
        have = false;
        const int l = static_cast<int>(cur >> kNodeBits);
        const int64_t k = cur & kNodeMask;
        if (l == 0) {
            const int64_t p0 = k * kLeaf;
            const int64_t p1 = p0 + kLeaf < n_src ? p0 + kLeaf : n_src;
            for (int64_t p = p0; p < p1; ++p) {
                const double dx = sorted[3 * p] - px;
                const double dy = sorted[3 * p + 1] - py;
                const double dz = sorted[3 * p + 2] - pz;
                const double d = (dx * dx + dy * dy) + dz * dz;
                const uint32_t i = orig[p];
                if (d < best || (d == best && i < best_i)) {
                    best = d;
                    best_i = i;
                }
            }
            continue;
        }
        const int64_t n_below = T.count[l - 1];
        const double *below = boxes + T.first[l - 1] * 6;
        const int64_t c0 = k * kFan;
        const uint32_t tag = static_cast<uint32_t>(l - 1) << kNodeBits;
        // a child is kept when its bound does not exceed the best so far;
        // one that is dropped, or that the level does not hold, sorts last
        double b[kFan];
        uint32_t kn[kFan];
#pragma unroll
        for (int q = 0; q < kFan; ++q) {
            const int64_t c = c0 + q;
            b[q] = __builtin_huge_val();
            kn[q] = kNone;
            if (c < n_below) {
                const double bound = box_bound(below + c * 6, px, py, pz);
                if (bound <= best) {
                    b[q] = bound;
                    kn[q] = tag | static_cast<uint32_t>(c);
                }
            }
        }
        order2(b[0], kn[0], b[1], kn[1]);
        order2(b[2], kn[2], b[3], kn[3]);
        order2(b[0], kn[0], b[2], kn[2]);
        order2(b[1], kn[1], b[3], kn[3]);
        order2(b[1], kn[1], b[2], kn[2]);
        // the nearest kept child is next, the others go onto the stack,
        // farthest first.  (A kept bound of +inf -- coordinates whose squares
        // overflow -- may sort behind a dropped child: hence the tests on kn,
        // not on the position.)
        int first = kFan;
#pragma unroll
        for (int q = kFan - 1; q >= 0; --q)
            if (kn[q] != kNone)
                first = q;
#pragma unroll
        for (int q = kFan - 1; q >= 0; --q) {
            if (kn[q] == kNone)
                continue;
            if (q == first) {
                cur = kn[q];
                have = true;
            } else {
                stack_node[top][lane] = kn[q];
                stack_bound[top][lane] = __double2float_rd(b[q]);
                ++top;
            }
        }
    }
    nearest[w] = static_cast<int32_t>(best_i);
}

int check_args(const double *src_xyz, int64_t n_src, const double *dst_xyz,
               int64_t n_dst, const int32_t *nearest_out)
{
    if (n_src < 1 || n_dst < 0 || n_src > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_nearest: n_src %lld (1 .. 2^31 - 1), n_dst %lld "
                    "(>= 0)", static_cast<long long>(n_src),
                    static_cast<long long>(n_dst));
    if (!src_xyz || (n_dst > 0 && (!dst_xyz || !nearest_out)))
        return fail(REMAP_ERR_ARG, "remap_nearest: NULL array");
    return REMAP_OK;
}

// the three phases; ev (NULL, or 4 events) is recorded around them
int run(const Layout &lay, const double *src_xyz, int64_t n_src,
        const double *dst_xyz, int64_t n_dst, int32_t *nearest_out,
        void *workspace, hipStream_t stream, hipEvent_t *ev)
{
    char *ws = static_cast<char *>(workspace);
    uint64_t *keys_in = reinterpret_cast<uint64_t *>(ws + lay.keys_in);
    uint64_t *keys_out = reinterpret_cast<uint64_t *>(ws + lay.keys_out);
    uint32_t *idx_in = reinterpret_cast<uint32_t *>(ws + lay.idx_in);
    uint32_t *idx_out = reinterpret_cast<uint32_t *>(ws + lay.idx_out);
    double *sorted = reinterpret_cast<double *>(ws + lay.xyz);
    double *boxes = reinterpret_cast<double *>(ws + lay.boxes);
    const Tree &T = lay.tree;

    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(morton_keys, dim3(blocks(n_src, kBlock)), dim3(kBlock),
                       0, stream, n_src, src_xyz, keys_in, idx_in);
    REMAP_HIP_CHECK(hipGetLastError());
    size_t tb = lay.temp_bytes;
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        ws + lay.temp, tb, static_cast<const uint64_t *>(keys_in), keys_out,
        static_cast<const uint32_t *>(idx_in), idx_out,
        static_cast<size_t>(n_src), 0u, 63u, stream)));
    hipLaunchKernelGGL(gather_sorted, dim3(blocks(n_src, kBlock)),
                       dim3(kBlock), 0, stream, n_src, src_xyz, idx_out,
                       sorted);
    REMAP_HIP_CHECK(hipGetLastError());
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(leaf_boxes, dim3(blocks(T.count[0], kBlock)),
                       dim3(kBlock), 0, stream, n_src, T.count[0], sorted,
                       boxes);
    REMAP_HIP_CHECK(hipGetLastError());
    for (int l = 1; l < T.levels; ++l) {
        hipLaunchKernelGGL(upper_boxes, dim3(blocks(T.count[l], kBlock)),
                           dim3(kBlock), 0, stream, T.count[l],
                           T.count[l - 1], boxes + T.first[l - 1] * 6,
                           boxes + T.first[l] * 6);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[2], stream));
    const size_t lds = size_t(stack_depth(T.levels)) * kWalkBlock * 8;
    for (int64_t at = 0; at < n_dst; at += kWalkChunk) {
        const int64_t m = n_dst - at < kWalkChunk ? n_dst - at : kWalkChunk;
        const dim3 grid(blocks(m, kWalkBlock)), block(kWalkBlock);
        hipLaunchKernelGGL(nearest_walk, grid, block, lds, stream, T, n_src,
                           sorted, idx_out, boxes, m, dst_xyz + 3 * at,
                           nearest_out + at);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    return REMAP_OK;
}

}  // namespace

int nearest_workspace(int64_t n_src, int64_t n_dst, size_t *bytes_out)
{
    if (!bytes_out || n_src < 1 || n_dst < 0 || n_src > INT32_MAX)
        return fail(REMAP_ERR_ARG, "remap_nearest_workspace: bad args");
    Layout lay;
    const int rc = make_layout(n_src, &lay);
    if (rc != REMAP_OK)
        return rc;
    *bytes_out = lay.total;
    return REMAP_OK;
}

int nearest(const double *src_xyz, int64_t n_src, const double *dst_xyz,
            int64_t n_dst, int32_t *nearest_out, void *workspace,
            size_t workspace_bytes, hipStream_t stream, float *phase_ms)
{
    int rc = check_args(src_xyz, n_src, dst_xyz, n_dst, nearest_out);
    if (rc != REMAP_OK)
        return rc;
    Layout lay;
    rc = make_layout(n_src, &lay);
    if (rc != REMAP_OK)
        return rc;
    if (!workspace || workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "remap_nearest: workspace of %zu bytes, need %zu",
                    workspace_bytes, lay.total);
    if (!phase_ms) {
        if (n_dst == 0)
            return REMAP_OK;
        return run(lay, src_xyz, n_src, dst_xyz, n_dst, nearest_out,
                   workspace, stream, nullptr);
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 4 && err == hipSuccess; ++k)
        err = hipEventCreate(&ev[k]);
    if (err == hipSuccess) {
        rc = run(lay, src_xyz, n_src, dst_xyz, n_dst, nearest_out, workspace,
                 stream, ev);
        if (rc == REMAP_OK)
            err = hipEventSynchronize(ev[3]);
        for (int k = 0; k < 3 && rc == REMAP_OK && err == hipSuccess; ++k)
            err = hipEventElapsedTime(&phase_ms[k], ev[k], ev[k + 1]);
    }
    for (int k = 0; k < 4; ++k)
        if (ev[k])
            (void)hipEventDestroy(ev[k]);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(err);
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_nearest_workspace(int64_t n_src, int64_t n_dst, size_t *bytes_out)
{
    return remap::nearest_workspace(n_src, n_dst, bytes_out);
}

int remap_nearest(const double *src_xyz, int64_t n_src, const double *dst_xyz,
                  int64_t n_dst, int32_t *nearest_out, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    return remap::nearest(src_xyz, n_src, dst_xyz, n_dst, nearest_out,
                          workspace, workspace_bytes,
                          static_cast<hipStream_t>(stream), nullptr);
}

int remap_nearest_timed(const double *src_xyz, int64_t n_src,
                        const double *dst_xyz, int64_t n_dst,
                        int32_t *nearest_out, void *workspace,
                        size_t workspace_bytes, float *phase_ms_out,
                        void *stream)
{
    if (!phase_ms_out)
        return remap::fail(REMAP_ERR_ARG, "remap_nearest_timed: NULL output");
    return remap::nearest(src_xyz, n_src, dst_xyz, n_dst, nearest_out,
                          workspace, workspace_bytes,
                          static_cast<hipStream_t>(stream), phase_ms_out);
}

}  // extern "C"
