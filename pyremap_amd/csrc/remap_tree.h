// The Morton-sorted box tree remap_nearest.hip and remap_locate.hip walk: the
// shape of its levels, the 63-bit key its leaves are sorted by, and the
// kernel that makes a level's boxes from the level below.  What a leaf holds
// (points, triangles) and how its box is made is the including file's.
#ifndef REMAP_TREE_H
#define REMAP_TREE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "remap_common.h"

namespace remap {
namespace {

constexpr size_t kAlign = 256;
constexpr int kLeaf = 8;       // sorted items a leaf
constexpr int kFan = 4;        // nodes below a node
// n <= 2^31 - 1 items: 2^28 leaves, a quarter as many nodes a level above
constexpr int kMaxLevels = 15;
// a node on a walk's stack: its level above kNodeBits, its index below
constexpr uint32_t kNodeBits = 28;
constexpr uint32_t kNodeMask = (1u << kNodeBits) - 1u;

size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

uint32_t blocks(int64_t n, int per)
{
    return static_cast<uint32_t>((n + per - 1) / per);
}

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

}  // namespace
}  // namespace remap

#endif  // REMAP_TREE_H
