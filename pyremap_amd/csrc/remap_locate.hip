// remap_locate.hip -- point location for `bilinear` maps from an MPAS mesh:
// for every destination point the triangle of the dual mesh that holds its
// central projection, the lowest triangle index where several do, and the
// barycentric weights of its corners.
//
// Definition (exact).  xyz (n_nodes, 3) fp64, tri (n_tri, 3) int32 node ids,
// points (n_pts, 3) fp64, tol >= 0.  Nodes and points are unit vectors to
// within 1e-6.  With
//   cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
//   dot(u, v)   = (u.x*v.x + u.y*v.y) + u.z*v.z
// in IEEE fp64 in that order (the library is built -ffp-contract=off), for
// the triangle t = (a, b, c) and the point q
//   D = dot(a, cross(b, c)),  s = -1 if D < 0, else +1
//   a triangle with D == 0, D not finite, or a node id outside [0, n_nodes)
//   holds nothing (and is never dereferenced)
//   w0 = s*dot(q, cross(b, c)), w1 = s*dot(q, cross(c, a)),
//   w2 = s*dot(q, cross(a, b)), tot = (w0 + w1) + w2
//   holds(q, t)  iff  tot > 0 and every w_k >= -tol*tot
//   found[q] = the LOWEST t that holds q, or -1
//   weights of the winner: v_k = w_k > 0 ? w_k : 0.0,
//   S_k = v_k / ((v0 + v1) + v2); zeros where found is -1.
// The result is a pure function of the inputs, independent of the triangles'
// orientation; numpy reproduces it bit for bit.
//
// Pipeline (all on the caller's stream, nothing synchronises, no atomics):
//   centroid_keys  63-bit Morton code of every triangle's centroid (a
//                  triangle that holds nothing: key 0)
//   radix sort     rocPRIM radix_sort_pairs on (key, original index)
//   setup          one lane per sorted triangle: its three s-signed normals
//                  s*cross(b, c), s*cross(c, a), s*cross(a, b) (zeros for a
//                  triangle that holds nothing) and its box; the boxes of the
//                  kLeaf triangles of a leaf are joined across lanes, which
//                  gives level 0 of the tree
//   upper_boxes    one launch a level (remap_tree.h)
//   locate_walk    one lane per point, 64-lane blocks, depth first, the stack
//                  in LDS laid out [entry][lane].  A node is entered only if
//                  q lies in its box.  At a leaf holds() is evaluated on the
//                  stored normals and the minimum original index kept.  The
//                  winner's weights are then computed from xyz and tri by
//                  the definition's own operations.
//
// The stored normals give holds() bit for bit: s is +-1, negation is exact
// and commutes with rounding to nearest, so dot(q, s*n) and s*dot(q, n) are
// the same number (up to the sign of a zero, which no comparison above
// sees).
//
// Why the pruning is exact.  The box of a triangle is the box of its corners
// widened on every side by
//   m_t = e_t^2/3 + 1e-5 + 32*tol + 2e-12/|D|
// (e_t its longest edge), and it is EVERYTHING unless m_t < 1.  A triangle
// may be skipped only if holds() rejects the point:
//  * In real arithmetic q = (w0*a + w1*b + w2*c)/|D| (the normals over D are
//    the rows of the inverse of the matrix of corners), so q = lambda*p with
//    p = sum_k beta_k corner_k, beta_k = w_k/tot, lambda = tot/|D|.
//  * The w_k are computed to 4e-15 absolute (components <= 1 + 1e-6, three
//    products and two sums a dot, two products and a difference a cross
//    component).  If the fp holds() accepts, the true w_k >= -tol*tot - eta
//    with eta = 5e-15.  |q| >= 1 - 1e-6 gives max_k |w_k| >= |D|/3.1, and for
//    |D| > 2e-12 (else m_t >= 1) that maximum is a positive w_k, hence
//    tot >= |D|/7 > 0 and beta_k >= -tau, tau = tol + 4e-14/|D|.
//  * p is then within 9*tau of a point p' of the flat triangle (clip the
//    negative beta_k, renormalise; the edges are <= 2 + 2e-6), and lambda > 0
//    makes |q - p| = ||q| - |p||.
//  * |p'| <= 1 + 1e-6 (convexity) and |p'|^2 >= (1 - 1e-6)^2 - e_t^2/3: the
//    point of the triangle closest to the origin is its circumcentre (radius
//    <= e_t/sqrt(3) when no angle is obtuse) or the midpoint of the longest
//    edge (e_t/2).  With 1 - sqrt(1 - x) <= x: ||q| - |p'|| <= e_t^2/3 + 3e-6.
//  * So every coordinate of q is within e_t^2/3 + 3e-6 + 18*tau of the
//    corners' box; m_t covers it with 7e-6 to spare for the roundings of
//    m_t, of the box's ends and of the pyramid (min and max are exact).
// The margin is the triangle's own, so the fine regions of a variable mesh
// are not widened by its coarsest cells; a sliver whose |D| drowns in the
// rounding of holds() is tested against every point instead of being trusted
// to a box.  Outside the 1e-6 contract the result is unspecified; the walk
// still ends (the stack is bounded by the tree's shape) and reads nothing
// outside its arrays (node ids are checked before any use).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_common.h"
#include "remap_sphere.h"
#include "remap_tree.h"

namespace remap {
namespace {

// (kWalkBlock lanes a walking block, kWalkChunk points a launch: remap_tree.h)
// every child whose box holds the point is stacked, then one is popped: at
// most kFan - 1 stay behind a level above level 0, and kFan at the last
constexpr int stack_depth(int levels) { return (kFan - 1) * (levels - 1) + 1; }
constexpr uint32_t kNoTriangle = 0xffffffffu;

static_assert(kBlock % kLeaf == 0 && kWave % kLeaf == 0 &&
              (kLeaf & (kLeaf - 1)) == 0,
              "setup joins a leaf's boxes across kLeaf neighbouring lanes");
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 4 <= 64 * 1024,
              "the walk's stack must fit in a workgroup's LDS");

// the corners of triangle t; false if one of its node ids is out of range
// (then nothing was read through them)
__device__ inline bool corners(int64_t t, int64_t n_nodes,
                               const double *__restrict__ xyz,
                               const int32_t *__restrict__ tri, V3 &a,
                               V3 &b, V3 &c)
{
    const int64_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
    if (ia < 0 || ia >= n_nodes || ib < 0 || ib >= n_nodes || ic < 0 ||
        ic >= n_nodes)
        return false;
    a = load3(xyz, ia);
    b = load3(xyz, ib);
    c = load3(xyz, ic);
    return true;
}

__device__ inline bool usable(double D)
{
    return D != 0.0 && D - D == 0.0;              // not 0, not Inf, not NaN
}

__global__ __launch_bounds__(kBlock) void centroid_keys(
    int64_t n_tri, int64_t n_nodes, const double *__restrict__ xyz,
    const int32_t *__restrict__ tri, uint64_t *__restrict__ keys,
    uint32_t *__restrict__ idx)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri)
        return;
    V3 a, b, c;
    uint64_t key = 0;
    if (corners(t, n_nodes, xyz, tri, a, b, c) &&
        usable(dot(a, cross(b, c))))
        key = morton_key((a.x + b.x + c.x) / 3.0, (a.y + b.y + c.y) / 3.0,
                         (a.z + b.z + c.z) / 3.0);
    keys[t] = key;
    idx[t] = static_cast<uint32_t>(t);
}

__device__ inline double min3(double a, double b, double c)
{
    return fmin(fmin(a, b), c);
}

__device__ inline double max3(double a, double b, double c)
{
    return fmax(fmax(a, b), c);
}

// one lane per sorted triangle; the lanes past the last triangle of the last
// leaf stay in for the joins with an empty box
__global__ __launch_bounds__(kBlock) void setup(
    int64_t n_tri, int64_t n_nodes, const double *__restrict__ xyz,
    const int32_t *__restrict__ tri, const uint32_t *__restrict__ orig,
    double tol, double *__restrict__ normals, double *__restrict__ boxes)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double inf = __builtin_huge_val();
    double box[6] = {inf, inf, inf, -inf, -inf, -inf};   // holds no point
    if (k < n_tri) {
        V3 a, b, c;
        V3 n0{0.0, 0.0, 0.0}, n1 = n0, n2 = n0;
        if (corners(orig[k], n_nodes, xyz, tri, a, b, c)) {
            const V3 bc = cross(b, c);
            const double D = dot(a, bc);
            if (usable(D)) {
                const double s = D < 0.0 ? -1.0 : 1.0;
                const V3 ca = cross(c, a), ab = cross(a, b);
                n0 = V3{s * bc.x, s * bc.y, s * bc.z};
                n1 = V3{s * ca.x, s * ca.y, s * ca.z};
                n2 = V3{s * ab.x, s * ab.y, s * ab.z};
                const double e2 = max3(edge2(a, b), edge2(b, c), edge2(c, a));
                const double m = e2 / 3.0 + 1e-5 + 32.0 * tol +
                                 2e-12 / fabs(D);
                if (m < 1.0) {
                    box[0] = min3(a.x, b.x, c.x) - m;
                    box[1] = min3(a.y, b.y, c.y) - m;
                    box[2] = min3(a.z, b.z, c.z) - m;
                    box[3] = max3(a.x, b.x, c.x) + m;
                    box[4] = max3(a.y, b.y, c.y) + m;
                    box[5] = max3(a.z, b.z, c.z) + m;
                } else {
                    box[0] = box[1] = box[2] = -inf;     // holds every point
                    box[3] = box[4] = box[5] = inf;
                }
            }
        }
        double *o = normals + k * 9;
        o[0] = n0.x; o[1] = n0.y; o[2] = n0.z;
        o[3] = n1.x; o[4] = n1.y; o[5] = n1.z;
        o[6] = n2.x; o[7] = n2.y; o[8] = n2.z;
    }
    // the leaf's box: kLeaf neighbouring lanes, every lane of the wave here
#pragma unroll
    for (int step = 1; step < kLeaf; step *= 2) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = __shfl_xor(box[a], step);
            const double h = __shfl_xor(box[3 + a], step);
            box[a] = l < box[a] ? l : box[a];
            box[3 + a] = h > box[3 + a] ? h : box[3 + a];
        }
    }
    if (k < n_tri && k % kLeaf == 0) {
        double *o = boxes + (k / kLeaf) * 6;
#pragma unroll
        for (int a = 0; a < 6; ++a)
            o[a] = box[a];
    }
}

// (in_box, push_children: remap_tree.h)

// one lane per point
__global__ __launch_bounds__(kWalkBlock) void locate_walk(
    Tree T, int64_t n_tri, const double *__restrict__ normals,
    const uint32_t *__restrict__ orig, const double *__restrict__ boxes,
    int64_t n_nodes, const double *__restrict__ xyz,
    const int32_t *__restrict__ tri, int64_t n_pts,
    const double *__restrict__ points, double tol,
    int32_t *__restrict__ found, double *__restrict__ weights)
{
    // stack_depth(T.levels) entries a lane
    extern __shared__ uint32_t stack_lds[];
    uint32_t (*stack)[kWalkBlock] =
        reinterpret_cast<uint32_t (*)[kWalkBlock]>(stack_lds);
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * kWalkBlock + lane;
    if (w >= n_pts)
        return;
    const V3 q = load3(points, w);
    uint32_t best = kNoTriangle;
    int top = 0;
    if (in_box(boxes + T.first[T.levels - 1] * 6, q))
        stack[top++][lane] = static_cast<uint32_t>(T.levels - 1) << kNodeBits;
    while (top > 0) {
        const uint32_t cur = stack[--top][lane];
        const int l = static_cast<int>(cur >> kNodeBits);
        const int64_t k = cur & kNodeMask;
        if (l == 0) {
            const int64_t p0 = k * kLeaf;
            const int64_t p1 = p0 + kLeaf < n_tri ? p0 + kLeaf : n_tri;
            for (int64_t p = p0; p < p1; ++p) {
                const uint32_t i = orig[p];
                if (i >= best)
                    continue;
                const double *n = normals + p * 9;
                const double w0 = dot(q, V3{n[0], n[1], n[2]});
                const double w1 = dot(q, V3{n[3], n[4], n[5]});
                const double w2 = dot(q, V3{n[6], n[7], n[8]});
                const double tot = (w0 + w1) + w2;
                const double least = -tol * tot;
                if (tot > 0.0 && w0 >= least && w1 >= least && w2 >= least)
                    best = i;
            }
            continue;
        }
        push_children(T, boxes, l, k, q, stack, lane, top);
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    V3 a, b, c;
    if (best != kNoTriangle && corners(best, n_nodes, xyz, tri, a, b, c)) {
        // the definition, on the winner alone
        const V3 bc = cross(b, c), ca = cross(c, a), ab = cross(a, b);
        const double s = dot(a, bc) < 0.0 ? -1.0 : 1.0;
        const double w0 = s * dot(q, bc), w1 = s * dot(q, ca),
                     w2 = s * dot(q, ab);
        const double v0 = w0 > 0.0 ? w0 : 0.0, v1 = w1 > 0.0 ? w1 : 0.0,
                     v2 = w2 > 0.0 ? w2 : 0.0;
        const double sum = (v0 + v1) + v2;
        S0 = v0 / sum;
        S1 = v1 / sum;
        S2 = v2 / sum;
    }
    found[w] = best == kNoTriangle ? -1 : static_cast<int32_t>(best);
    weights[3 * w] = S0;
    weights[3 * w + 1] = S1;
    weights[3 * w + 2] = S2;
}

int check_args(const double *xyz, int64_t n_nodes, const int32_t *tri,
               int64_t n_tri, const double *points, int64_t n_pts, double tol,
               const int32_t *found_out, const double *weights_out)
{
    if (n_nodes < 1 || n_tri < 1 || n_tri > INT32_MAX || n_pts < 0 ||
        !(tol >= 0.0))
        return fail(REMAP_ERR_ARG,
                    "remap_locate: n_nodes %lld (>= 1), n_tri %lld (1 .. "
                    "2^31 - 1), n_pts %lld (>= 0), tol %g (>= 0)",
                    static_cast<long long>(n_nodes),
                    static_cast<long long>(n_tri),
                    static_cast<long long>(n_pts), tol);
    if (!xyz || !tri ||
        (n_pts > 0 && (!points || !found_out || !weights_out)))
        return fail(REMAP_ERR_ARG, "remap_locate: NULL array");
    return REMAP_OK;
}

// a leaf holds its triangles' three edge normals
constexpr size_t kPayload = 72;

// the three phases; ev (NULL, or 4 events) is recorded around them
int run(const TreeLayout &lay, const double *xyz, int64_t n_nodes,
        const int32_t *tri, int64_t n_tri, const double *points,
        int64_t n_pts, double tol, int32_t *found_out, double *weights_out,
        void *workspace, hipStream_t stream, hipEvent_t *ev)
{
    const TreeArrays A = tree_arrays(lay, workspace);
    const Tree &T = lay.tree;
    REMAP_TRY(build_tree(
        lay, A, n_tri, workspace, stream, ev,
        [&] {
            return launch(centroid_keys, n_tri, kBlock, stream, n_tri,
                          n_nodes, xyz, tri, A.keys_in, A.idx_in);
        },
        nothing_sorted,
        [&] {
            return launch(setup, n_tri, kBlock, stream, n_tri, n_nodes, xyz,
                          tri, A.orig, tol, A.payload, A.boxes);
        }));
    const size_t lds = size_t(stack_depth(T.levels)) * kWalkBlock * 4;
    REMAP_TRY(walk_chunks(n_pts, [&](int64_t at, int64_t m) {
        return launch_blocks(locate_walk, blocks(m, kWalkBlock), kWalkBlock,
                             lds, stream, T, n_tri, A.payload, A.orig,
                             A.boxes, n_nodes, xyz, tri, m, points + 3 * at,
                             tol, found_out + at, weights_out + 3 * at);
    }));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    return REMAP_OK;
}

}  // namespace

int locate_workspace(int64_t n_nodes, int64_t n_tri, int64_t n_pts,
                     size_t *bytes_out)
{
    if (!bytes_out || n_nodes < 1 || n_tri < 1 || n_pts < 0 ||
        n_tri > INT32_MAX)
        return fail(REMAP_ERR_ARG, "remap_locate_workspace: bad args");
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_tri, kPayload, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int locate(const double *xyz, int64_t n_nodes, const int32_t *tri,
           int64_t n_tri, const double *points, int64_t n_pts, double tol,
           int32_t *found_out, double *weights_out, void *workspace,
           size_t workspace_bytes, hipStream_t stream, float *phase_ms)
{
    REMAP_TRY(check_args(xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                         found_out, weights_out));
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(n_tri, kPayload, &lay));
    REMAP_TRY(need_workspace("remap_locate", workspace, workspace_bytes,
                             lay.total));
    if (!phase_ms) {
        if (n_pts == 0)
            return REMAP_OK;
        return run(lay, xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                   found_out, weights_out, workspace, stream, nullptr);
    }
    return timed_phases<4>(phase_ms, [&](hipEvent_t *ev) {
        return run(lay, xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                   found_out, weights_out, workspace, stream, ev);
    });
}

}  // namespace remap

extern "C" {

int remap_locate_workspace(int64_t n_nodes, int64_t n_tri, int64_t n_pts,
                           size_t *bytes_out)
{
    return remap::locate_workspace(n_nodes, n_tri, n_pts, bytes_out);
}

int remap_locate(const double *xyz, int64_t n_nodes, const int32_t *tri,
                 int64_t n_tri, const double *points, int64_t n_pts,
                 double tol, int32_t *found_out, double *weights_out,
                 void *workspace, size_t workspace_bytes, void *stream)
{
    return remap::locate(xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                         found_out, weights_out, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream), nullptr);
}

int remap_locate_timed(const double *xyz, int64_t n_nodes, const int32_t *tri,
                       int64_t n_tri, const double *points, int64_t n_pts,
                       double tol, int32_t *found_out, double *weights_out,
                       void *workspace, size_t workspace_bytes,
                       float *phase_ms_out, void *stream)
{
    if (!phase_ms_out)
        return remap::fail(REMAP_ERR_ARG, "remap_locate_timed: NULL output");
    return remap::locate(xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                         found_out, weights_out, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream), phase_ms_out);
}

}  // extern "C"
