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
//
// The k nearest (remap_nearest_k, 1 <= k <= REMAP_NEAREST_K_MAX).  Row i of
// the output holds the min(k, n_src) sources that come first in (d2(i, j), j)
// lexicographic order, ascending; the slots behind them hold index -1 and
// d2 = +inf.  k = 1 is remap_nearest's answer.  Everything before the walk
// is shared (build); nearest_k_walk is nearest_walk with "best" read as
// "k-th best":
//   * beside the stack a lane keeps its k best in LDS, [entry][lane], d2
//     (fp64) then index (int32), ascending in (d2, index).  Every slot starts
//     as (+inf, 0xffffffff), which sorts behind any source (an index is at
//     most 2^31 - 2) and IS the padding of the definition, so "the list is
//     full" needs no counter: until k sources are in, the k-th best d2 is
//     +inf and no bound exceeds it.
//   * the k-th best (d2, index) -- the last slot -- is mirrored in registers.
//     A source enters when it is lexicographically below it: it is put in
//     its place, the slots behind it move one down and the last drops out.
//   * a node is dropped only when its bound is STRICTLY greater than the
//     k-th best d2.  fl(bound) <= fl(d2(s)) for every s in the box (above),
//     so a dropped box holds only sources with d2 > the k-th best d2 at that
//     moment, and the k-th best only ever decreases: none of them belongs to
//     the final k.  A box whose bound EQUALS the k-th best d2 may hold a
//     source of that d2 with a lower index, so it is kept.  The final list
//     is therefore the k smallest of ALL (d2, j) pairs, whatever the
//     traversal order, the leaf size, the fan-out and the sort.
//   * the 64 lists of a block leave through LDS: the block's part of the
//     (n_dst, k) row-major outputs is contiguous, and lane t stores its
//     elements t, t + 64, ...
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_common.h"
#include "remap_tree.h"

namespace remap {
namespace {

// (kWalkBlock lanes a walking block, kWalkChunk points a launch,
// kLeaf sorted points a leaf, kFan nodes below a node: remap_tree.h)
// the walk steps into one child and stacks at most kFan - 1 a level above
// level 0, so that bounds the stack whatever the points are.  The launch
// sizes the LDS by the tree at hand (8 bytes an entry and lane): the fewer
// levels, the more walking waves fit beside each other in a CU
constexpr int stack_depth(int levels) { return (kFan - 1) * (levels - 1); }
constexpr uint32_t kNone = 0xffffffffu;   // no node (levels end at 14)

static_assert(kFan == 4, "nearest_walk sorts four children by hand");
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 8 <= 64 * 1024,
              "the walk's stack must fit in a workgroup's LDS");
// nearest_k_walk's list beside the stack: 12 bytes an entry and lane
constexpr size_t list_bytes(int k) { return size_t(k) * kWalkBlock * 12; }
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 8 +
                      list_bytes(REMAP_NEAREST_K_MAX) <= 64 * 1024,
              "the k-walk's stack and list must fit in a workgroup's LDS");

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

// (d, i) before (dq, iq) in the order of the definition
__device__ inline bool comes_first(double d, uint32_t i, double dq,
                                   uint32_t iq)
{
    return d < dq || (d == dq && i < iq);
}

// one lane per destination point: its k nearest (see the file's head).  The
// LDS holds the lists' d2 (k entries a lane), their indices, then the stack
// as in nearest_walk.
__global__ __launch_bounds__(kWalkBlock) void nearest_k_walk(
    Tree T, int64_t n_src, const double *__restrict__ sorted,
    const uint32_t *__restrict__ orig, const double *__restrict__ boxes,
    int64_t n_dst, const double *__restrict__ dst, int k,
    int32_t *__restrict__ idx_out, double *__restrict__ d2_out)
{
    extern __shared__ double list_lds[];
    double (*list_d)[kWalkBlock] =
        reinterpret_cast<double (*)[kWalkBlock]>(list_lds);
    uint32_t *words = reinterpret_cast<uint32_t *>(list_lds + k * kWalkBlock);
    uint32_t (*list_i)[kWalkBlock] =
        reinterpret_cast<uint32_t (*)[kWalkBlock]>(words);
    uint32_t (*stack_node)[kWalkBlock] =
        reinterpret_cast<uint32_t (*)[kWalkBlock]>(words + k * kWalkBlock);
    float (*stack_bound)[kWalkBlock] = reinterpret_cast<float (*)[kWalkBlock]>(
        words + (k + stack_depth(T.levels)) * kWalkBlock);
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kWalkBlock;
    const int64_t w = base + lane;
    if (w < n_dst) {
        const double px = dst[3 * w], py = dst[3 * w + 1], pz = dst[3 * w + 2];
        for (int q = 0; q < k; ++q) {
            list_d[q][lane] = __builtin_huge_val();
            list_i[q][lane] = 0xffffffffu;
        }
        // the k-th best so far: the list's last slot
        double kth = __builtin_huge_val();
        uint32_t kth_i = 0xffffffffu;
        int top = 0;
        uint32_t cur = static_cast<uint32_t>(T.levels - 1) << kNodeBits;
        bool have = true;
        for (;;) {
            if (!have) {
                if (top == 0)
                    break;
                --top;
                // (the float is at most the node's bound: the file's head)
                if (static_cast<double>(stack_bound[top][lane]) > kth)
                    continue;
                cur = stack_node[top][lane];
            }
            have = false;
            const int l = static_cast<int>(cur >> kNodeBits);
            const int64_t node = cur & kNodeMask;
            if (l == 0) {
                const int64_t p0 = node * kLeaf;
                const int64_t p1 = p0 + kLeaf < n_src ? p0 + kLeaf : n_src;
                for (int64_t p = p0; p < p1; ++p) {
                    const double dx = sorted[3 * p] - px;
                    const double dy = sorted[3 * p + 1] - py;
                    const double dz = sorted[3 * p + 2] - pz;
                    const double d = (dx * dx + dy * dy) + dz * dz;
                    const uint32_t i = orig[p];
                    if (!comes_first(d, i, kth, kth_i))
                        continue;
                    // into its place; the last slot drops out
                    int q = k - 1;
                    while (q > 0) {
                        const double dq = list_d[q - 1][lane];
                        const uint32_t iq = list_i[q - 1][lane];
                        if (!comes_first(d, i, dq, iq))
                            break;
                        list_d[q][lane] = dq;
                        list_i[q][lane] = iq;
                        --q;
                    }
                    list_d[q][lane] = d;
                    list_i[q][lane] = i;
                    kth = list_d[k - 1][lane];
                    kth_i = list_i[k - 1][lane];
                }
                continue;
            }
            const int64_t n_below = T.count[l - 1];
            const double *below = boxes + T.first[l - 1] * 6;
            const int64_t c0 = node * kFan;
            const uint32_t tag = static_cast<uint32_t>(l - 1) << kNodeBits;
            // a child is kept when its bound does not exceed the k-th best;
            // one that is dropped, or that the level does not hold, sorts
            // last
            double b[kFan];
            uint32_t kn[kFan];
#pragma unroll
            for (int q = 0; q < kFan; ++q) {
                const int64_t c = c0 + q;
                b[q] = __builtin_huge_val();
                kn[q] = kNone;
                if (c < n_below) {
                    const double bound = box_bound(below + c * 6, px, py, pz);
                    if (bound <= kth) {
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
            // (as in nearest_walk: the tests are on kn, not on the position)
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
    }
    // every lane of the block is here: the lists leave as whole rows, element
    // e of the block's part is slot e % k of lane e / k
    __syncthreads();
    const int64_t rest = n_dst - base;
    const int rows = rest < kWalkBlock ? static_cast<int>(rest) : kWalkBlock;
    const int64_t out = base * k;
    for (int e = lane; e < rows * k; e += kWalkBlock) {
        const int r = e / k, s = e - r * k;
        idx_out[out + e] = static_cast<int32_t>(list_i[s][r]);
        d2_out[out + e] = list_d[s][r];
    }
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

// a leaf holds its points' xyz, gathered into sorted order
constexpr size_t kPayload = 24;

// the two phases before a walk: sort (with the gather) and boxes; ev (NULL,
// or at least 3 events) is recorded around them
int build(const TreeLayout &lay, const TreeArrays &A, const double *src_xyz,
          int64_t n_src, void *workspace, hipStream_t stream, hipEvent_t *ev)
{
    return build_tree(
        lay, A, n_src, workspace, stream, ev,
        [&] {
            return launch(morton_keys, n_src, kBlock, stream, n_src, src_xyz,
                          A.keys_in, A.idx_in);
        },
        [&] {
            return launch(gather_sorted, n_src, kBlock, stream, n_src,
                          src_xyz, A.orig, A.payload);
        },
        [&] {
            const int64_t n_leaves = lay.tree.count[0];
            return launch(leaf_boxes, n_leaves, kBlock, stream, n_src,
                          n_leaves, A.payload, A.boxes);
        });
}

// the three phases; ev (NULL, or 4 events) is recorded around them
int run(const TreeLayout &lay, const double *src_xyz, int64_t n_src,
        const double *dst_xyz, int64_t n_dst, int32_t *nearest_out,
        void *workspace, hipStream_t stream, hipEvent_t *ev)
{
    const TreeArrays A = tree_arrays(lay, workspace);
    REMAP_TRY(build(lay, A, src_xyz, n_src, workspace, stream, ev));
    const Tree &T = lay.tree;
    const size_t lds = size_t(stack_depth(T.levels)) * kWalkBlock * 8;
    REMAP_TRY(walk_chunks(n_dst, [&](int64_t at, int64_t m) {
        return launch_blocks(nearest_walk, blocks(m, kWalkBlock), kWalkBlock,
                             lds, stream, T, n_src, A.payload, A.orig,
                             A.boxes, m, dst_xyz + 3 * at, nearest_out + at);
    }));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    return REMAP_OK;
}

// sort, boxes, then the k-walk
int run_k(const TreeLayout &lay, const double *src_xyz, int64_t n_src,
          const double *dst_xyz, int64_t n_dst, int k, int32_t *idx_out,
          double *d2_out, void *workspace, hipStream_t stream)
{
    const TreeArrays A = tree_arrays(lay, workspace);
    REMAP_TRY(build(lay, A, src_xyz, n_src, workspace, stream, nullptr));
    const Tree &T = lay.tree;
    const size_t lds = list_bytes(k) +
        size_t(stack_depth(T.levels)) * kWalkBlock * 8;
    return walk_chunks(n_dst, [&](int64_t at, int64_t m) {
        return launch_blocks(nearest_k_walk, blocks(m, kWalkBlock),
                             kWalkBlock, lds, stream, T, n_src, A.payload,
                             A.orig, A.boxes, m, dst_xyz + 3 * at, k,
                             idx_out + at * k, d2_out + at * k);
    });
}

}  // namespace

int nearest_workspace(int64_t n_src, int64_t n_dst, size_t *bytes_out)
{
    if (!bytes_out || n_src < 1 || n_dst < 0 || n_src > INT32_MAX)
        return fail(REMAP_ERR_ARG, "remap_nearest_workspace: bad args");
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_src, kPayload, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int nearest(const double *src_xyz, int64_t n_src, const double *dst_xyz,
            int64_t n_dst, int32_t *nearest_out, void *workspace,
            size_t workspace_bytes, hipStream_t stream, float *phase_ms)
{
    REMAP_TRY(check_args(src_xyz, n_src, dst_xyz, n_dst, nearest_out));
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_src, kPayload, &lay));
    REMAP_TRY(need_workspace("remap_nearest", workspace, workspace_bytes,
                             lay.total));
    if (!phase_ms) {
        if (n_dst == 0)
            return REMAP_OK;
        return run(lay, src_xyz, n_src, dst_xyz, n_dst, nearest_out,
                   workspace, stream, nullptr);
    }
    return timed_phases<4>(phase_ms, [&](hipEvent_t *ev) {
        return run(lay, src_xyz, n_src, dst_xyz, n_dst, nearest_out,
                   workspace, stream, ev);
    });
}

int nearest_k_workspace(int64_t n_src, int64_t n_dst, int32_t k,
                        size_t *bytes_out)
{
    if (!bytes_out || n_src < 1 || n_dst < 0 || n_src > INT32_MAX || k < 1 ||
        k > REMAP_NEAREST_K_MAX)
        return fail(REMAP_ERR_ARG, "remap_nearest_k_workspace: bad args");
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_src, kPayload, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int nearest_k(const double *src_xyz, int64_t n_src, const double *dst_xyz,
              int64_t n_dst, int32_t k, int32_t *idx_out, double *d2_out,
              void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (n_src < 1 || n_dst < 0 || n_src > INT32_MAX || k < 1 ||
        k > REMAP_NEAREST_K_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_nearest_k: n_src %lld (1 .. 2^31 - 1), n_dst %lld "
                    "(>= 0), k %d (1 .. %d)", static_cast<long long>(n_src),
                    static_cast<long long>(n_dst), static_cast<int>(k),
                    REMAP_NEAREST_K_MAX);
    if (!src_xyz || (n_dst > 0 && (!dst_xyz || !idx_out || !d2_out)))
        return fail(REMAP_ERR_ARG, "remap_nearest_k: NULL array");
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_src, kPayload, &lay));
    REMAP_TRY(need_workspace("remap_nearest_k", workspace, workspace_bytes,
                             lay.total));
    if (n_dst == 0)
        return REMAP_OK;
    return run_k(lay, src_xyz, n_src, dst_xyz, n_dst, k, idx_out, d2_out,
                 workspace, stream);
}

}  // namespace remap

extern "C" {

int remap_nearest_k_workspace(int64_t n_src, int64_t n_dst, int32_t k,
                              size_t *bytes_out)
{
    return remap::nearest_k_workspace(n_src, n_dst, k, bytes_out);
}

int remap_nearest_k(const double *src_xyz, int64_t n_src,
                    const double *dst_xyz, int64_t n_dst, int32_t k,
                    int32_t *idx_out, double *d2_out, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    return remap::nearest_k(src_xyz, n_src, dst_xyz, n_dst, k, idx_out,
                            d2_out, workspace, workspace_bytes,
                            static_cast<hipStream_t>(stream));
}

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
