// The Morton-sorted box tree remap_nearest.hip, remap_locate.hip and
// remap_quads.hip walk: the shape of its levels, the 63-bit key its leaves are
// sorted by, its place in a workspace (TreeLayout), the build from the
// including file's own key and leaf kernels (build_tree), the chunked launch
// of a walk (walk_chunks) and, on the device, the kernel that makes a level's
// boxes from the level below and the descent of a walk that looks for the
// boxes holding a point (in_box, push_children).  What a leaf holds (points,
// triangles, quads) and how its box is made is the including file's.
#ifndef REMAP_TREE_H
#define REMAP_TREE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "remap_common.h"
#include "remap_host.h"

namespace remap {
namespace {

constexpr int kLeaf = 8;       // sorted items a leaf
constexpr int kFan = 4;        // nodes below a node
// n <= 2^31 - 1 items: 2^28 leaves, a quarter as many nodes a level above
constexpr int kMaxLevels = 15;
// a node on a walk's stack: its level above kNodeBits, its index below
constexpr uint32_t kNodeBits = 28;
constexpr uint32_t kNodeMask = (1u << kNodeBits) - 1u;
// the bits of a Morton key: what the sort of the leaves looks at
constexpr unsigned kKeyBits = 63;
// a walk: one lane per point in blocks of kWalkBlock, at most kWalkChunk
// points a launch (its block count stays far below the grid limit)
constexpr int kWalkBlock = 64;
constexpr int64_t kWalkChunk = int64_t(1) << 30;

// level l holds count[l] nodes, its boxes (6 doubles each: lo, then hi, an
// axis) from node first[l]
struct Tree {
    int32_t levels;
    int64_t count[kMaxLevels];
    int64_t first[kMaxLevels];
};

// the levels over n items; returns the number of nodes of all levels
int64_t make_tree(int64_t n, Tree *tree)
{
    Tree &t = *tree;
    int64_t c = (n + kLeaf - 1) / kLeaf, nodes = 0;
    t.levels = 0;
    for (;;) {
        t.count[t.levels] = c;
        t.first[t.levels] = nodes;
        nodes += c;
        ++t.levels;
        if (c == 1)
            break;
        c = (c + kFan - 1) / kFan;
    }
    for (int l = t.levels; l < kMaxLevels; ++l)
        t.count[l] = t.first[l] = 0;
    return nodes;
}

// every third bit of the result holds a bit of v (21 of them)
__device__ inline uint64_t spread3(uint64_t v)
{
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

__device__ inline uint64_t quantise(double x)
{
    const double q = (x + 1.0) * 1048576.0;   // [-1, 1] -> [0, 2^21]
    if (!(q > 0.0))
        return 0;
    return q >= 2097151.0 ? 2097151ull : static_cast<uint64_t>(q);
}

// 63-bit Morton code over [-1, 1]^3 (21 bits an axis, clamped; NaN -> 0)
__device__ inline uint64_t morton_key(double x, double y, double z)
{
    return spread3(quantise(x)) << 2 | spread3(quantise(y)) << 1 |
           spread3(quantise(z));
}

// one lane per node of a level >= 1, the level below it complete
__global__ __launch_bounds__(kBlock) void upper_boxes(
    int64_t n_nodes, int64_t n_below, const double *__restrict__ below,
    double *__restrict__ boxes)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_nodes)
        return;
    const int64_t c0 = k * kFan;
    const int64_t c1 = c0 + kFan < n_below ? c0 + kFan : n_below;
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
        b[a] = below[c0 * 6 + a];
    for (int64_t c = c0 + 1; c < c1; ++c) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = below[c * 6 + a], h = below[c * 6 + 3 + a];
            b[a] = l < b[a] ? l : b[a];
            b[3 + a] = h > b[3 + a] ? h : b[3 + a];
        }
    }
    double *o = boxes + k * 6;
#pragma unroll
    for (int a = 0; a < 6; ++a)
        o[a] = b[a];
}

// whether the box b holds the point q (a struct of x, y, z)
template <class Point>
__device__ inline bool in_box(const double *__restrict__ b, const Point &q)
{
    return q.x >= b[0] && q.x <= b[3] && q.y >= b[1] && q.y <= b[4] &&
           q.z >= b[2] && q.z <= b[5];
}

// a walk for the boxes that hold q, at node k of level l >= 1: its children
// whose box holds q go onto the lane's stack (LDS, [entry][lane]), the last
// first
template <class Point>
__device__ inline void push_children(
    const Tree &T, const double *__restrict__ boxes, int l, int64_t k,
    const Point &q, uint32_t (*stack)[kWalkBlock], int lane, int &top)
{
    const int64_t n_below = T.count[l - 1];
    const double *below = boxes + T.first[l - 1] * 6;
    const int64_t c0 = k * kFan;
    const uint32_t tag = static_cast<uint32_t>(l - 1) << kNodeBits;
#pragma unroll
    for (int c = kFan - 1; c >= 0; --c)
        if (c0 + c < n_below && in_box(below + (c0 + c) * 6, q))
            stack[top++][lane] = tag | static_cast<uint32_t>(c0 + c);
}

// the tree over n items in a workspace: the keys and indices on both sides
// of the sort, what the leaves hold (payload, so many bytes an item, in
// sorted order), the boxes of every level, rocPRIM's scratch
struct TreeLayout {
    Tree tree;
    size_t keys_in, keys_out, idx_in, idx_out, payload, boxes, temp, total;
    size_t temp_bytes;
};

int make_tree_layout(int64_t n_items, size_t payload_bytes_per_item,
                     TreeLayout *lay)
{
    const size_t n = static_cast<size_t>(n_items);
    const int64_t nodes = make_tree(n_items, &lay->tree);
    REMAP_TRY(sort_pairs_temp<uint32_t>(n, &lay->temp_bytes, kKeyBits));
    size_t off = 0;
    lay->keys_in = take(&off, n * 8);
    lay->keys_out = take(&off, n * 8);
    lay->idx_in = take(&off, n * 4);
    lay->idx_out = take(&off, n * 4);
    lay->payload = take(&off, n * payload_bytes_per_item);
    lay->boxes = take(&off, static_cast<size_t>(nodes) * 48);
    lay->temp = take(&off, lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

// the arrays of a TreeLayout in a workspace; a walk reads orig (the sorted
// items' original indices), payload and boxes once build_tree() has run
struct TreeArrays {
    uint64_t *keys_in, *keys_out;
    uint32_t *idx_in, *orig;
    double *payload, *boxes;
};

TreeArrays tree_arrays(const TreeLayout &lay, void *workspace)
{
    char *ws = static_cast<char *>(workspace);
    return {at<uint64_t>(ws, lay.keys_in), at<uint64_t>(ws, lay.keys_out),
            at<uint32_t>(ws, lay.idx_in), at<uint32_t>(ws, lay.idx_out),
            at<double>(ws, lay.payload), at<double>(ws, lay.boxes)};
}

// the two phases before a walk.  Sort: keys() fills A.keys_in and A.idx_in
// for the n items, the pairs are sorted, sorted() runs what the file still
// counts to the sort (or nothing).  Boxes: leaves() writes level 0 of
// A.boxes (and the payload), upper_boxes the levels above.  ev (NULL, or at
// least 3 events) is recorded around the phases
template <class Keys, class Sorted, class Leaves>
int build_tree(const TreeLayout &lay, const TreeArrays &A, int64_t n,
               void *workspace, hipStream_t stream, hipEvent_t *ev, Keys keys,
               Sorted sorted, Leaves leaves)
{
    const Tree &T = lay.tree;
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[0], stream));
    REMAP_TRY(keys());
    REMAP_TRY(radix_sort_pairs(static_cast<char *>(workspace) + lay.temp,
                               lay.temp_bytes, A.keys_in, A.keys_out,
                               A.idx_in, A.orig, n, stream, kKeyBits));
    REMAP_TRY(sorted());
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[1], stream));
    REMAP_TRY(leaves());
    for (int l = 1; l < T.levels; ++l)
        REMAP_TRY(launch(upper_boxes, T.count[l], kBlock, stream, T.count[l],
                         T.count[l - 1], A.boxes + T.first[l - 1] * 6,
                         A.boxes + T.first[l] * 6));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[2], stream));
    return REMAP_OK;
}

// nothing between the sort and the leaves
inline int nothing_sorted() { return REMAP_OK; }

// a walk over n_pts points: walk(at, m) launches points [at, at + m)
template <class Walk>
int walk_chunks(int64_t n_pts, Walk walk)
{
    for (int64_t at = 0; at < n_pts; at += kWalkChunk) {
        const int64_t m = n_pts - at < kWalkChunk ? n_pts - at : kWalkChunk;
        REMAP_TRY(walk(at, m));
    }
    return REMAP_OK;
}

}  // namespace
}  // namespace remap

#endif  // REMAP_TREE_H
