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

#include <rocprim/rocprim.hpp>

#include "remap_common.h"
#include "remap_tree.h"

namespace remap {
namespace {

constexpr int kWalkBlock = 64;
// every child whose box holds the point is stacked, then one is popped: at
// most kFan - 1 stay behind a level above level 0, and kFan at the last
constexpr int stack_depth(int levels) { return (kFan - 1) * (levels - 1) + 1; }
// one walk launch: its block count stays far below the grid limit
constexpr int64_t kWalkChunk = int64_t(1) << 30;
constexpr uint32_t kNoTriangle = 0xffffffffu;

static_assert(kBlock % kLeaf == 0 && kWave % kLeaf == 0 &&
              (kLeaf & (kLeaf - 1)) == 0,
              "setup joins a leaf's boxes across kLeaf neighbouring lanes");
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 4 <= 64 * 1024,
              "the walk's stack must fit in a workgroup's LDS");

struct Layout {
    Tree tree;
    size_t keys_in, keys_out, idx_in, idx_out, normals, boxes, temp, total;
    size_t temp_bytes;
};

int make_layout(int64_t n_tri, Layout *lay)
{
    const size_t n = static_cast<size_t>(n_tri);
    const int64_t nodes = make_tree(n_tri, &lay->tree);
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
    lay->normals = off;  off += align_up(n * 72);
    lay->boxes = off;    off += align_up(static_cast<size_t>(nodes) * 48);
    lay->temp = off;     off += align_up(lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

struct Vec3 {
    double x, y, z;
};

__device__ inline Vec3 load3(const double *__restrict__ p, int64_t i)
{
    return Vec3{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
}

__device__ inline Vec3 cross(const Vec3 &u, const Vec3 &v)
{
    return Vec3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z,
                u.x * v.y - u.y * v.x};
}

__device__ inline double dot(const Vec3 &u, const Vec3 &v)
{
    return (u.x * v.x + u.y * v.y) + u.z * v.z;
}

// the corners of triangle t; false if one of its node ids is out of range
// (then nothing was read through them)
__device__ inline bool corners(int64_t t, int64_t n_nodes,
                               const double *__restrict__ xyz,
                               const int32_t *__restrict__ tri, Vec3 &a,
                               Vec3 &b, Vec3 &c)
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
    Vec3 a, b, c;
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

__device__ inline double edge2(const Vec3 &u, const Vec3 &v)
{
    const double dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z;
    return (dx * dx + dy * dy) + dz * dz;
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
        Vec3 a, b, c;
        Vec3 n0{0.0, 0.0, 0.0}, n1 = n0, n2 = n0;
        if (corners(orig[k], n_nodes, xyz, tri, a, b, c)) {
            const Vec3 bc = cross(b, c);
            const double D = dot(a, bc);
            if (usable(D)) {
                const double s = D < 0.0 ? -1.0 : 1.0;
                const Vec3 ca = cross(c, a), ab = cross(a, b);
                n0 = Vec3{s * bc.x, s * bc.y, s * bc.z};
                n1 = Vec3{s * ca.x, s * ca.y, s * ca.z};
                n2 = Vec3{s * ab.x, s * ab.y, s * ab.z};
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

__device__ inline bool in_box(const double *__restrict__ b, const Vec3 &q)
{
    return q.x >= b[0] && q.x <= b[3] && q.y >= b[1] && q.y <= b[4] &&
           q.z >= b[2] && q.z <= b[5];
}

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
    const Vec3 q = load3(points, w);
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
                const double w0 = dot(q, Vec3{n[0], n[1], n[2]});
                const double w1 = dot(q, Vec3{n[3], n[4], n[5]});
                const double w2 = dot(q, Vec3{n[6], n[7], n[8]});
                const double tot = (w0 + w1) + w2;
                const double least = -tol * tot;
                if (tot > 0.0 && w0 >= least && w1 >= least && w2 >= least)
                    best = i;
            }
            continue;
        }
        const int64_t n_below = T.count[l - 1];
        const double *below = boxes + T.first[l - 1] * 6;
        const int64_t c0 = k * kFan;
        const uint32_t tag = static_cast<uint32_t>(l - 1) << kNodeBits;
#pragma unroll
        for (int c = kFan - 1; c >= 0; --c)
            if (c0 + c < n_below && in_box(below + (c0 + c) * 6, q))
                stack[top++][lane] = tag | static_cast<uint32_t>(c0 + c);
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    Vec3 a, b, c;
    if (best != kNoTriangle && corners(best, n_nodes, xyz, tri, a, b, c)) {
        // the definition, on the winner alone
        const Vec3 bc = cross(b, c), ca = cross(c, a), ab = cross(a, b);
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

// the three phases; ev (NULL, or 4 events) is recorded around them
int run(const Layout &lay, const double *xyz, int64_t n_nodes,
        const int32_t *tri, int64_t n_tri, const double *points,
        int64_t n_pts, double tol, int32_t *found_out, double *weights_out,
        void *workspace, hipStream_t stream, hipEvent_t *ev)
{
    char *ws = static_cast<char *>(workspace);
    uint64_t *keys_in = reinterpret_cast<uint64_t *>(ws + lay.keys_in);
    uint64_t *keys_out = reinterpret_cast<uint64_t *>(ws + lay.keys_out);
    uint32_t *idx_in = reinterpret_cast<uint32_t *>(ws + lay.idx_in);
    uint32_t *idx_out = reinterpret_cast<uint32_t *>(ws + lay.idx_out);
    double *normals = reinterpret_cast<double *>(ws + lay.normals);
    double *boxes = reinterpret_cast<double *>(ws + lay.boxes);
    const Tree &T = lay.tree;

    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(centroid_keys, dim3(blocks(n_tri, kBlock)),
                       dim3(kBlock), 0, stream, n_tri, n_nodes, xyz, tri,
                       keys_in, idx_in);
    REMAP_HIP_CHECK(hipGetLastError());
    size_t tb = lay.temp_bytes;
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        ws + lay.temp, tb, static_cast<const uint64_t *>(keys_in), keys_out,
        static_cast<const uint32_t *>(idx_in), idx_out,
        static_cast<size_t>(n_tri), 0u, 63u, stream)));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(setup, dim3(blocks(n_tri, kBlock)), dim3(kBlock), 0,
                       stream, n_tri, n_nodes, xyz, tri, idx_out, tol,
                       normals, boxes);
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
    const size_t lds = size_t(stack_depth(T.levels)) * kWalkBlock * 4;
    for (int64_t at = 0; at < n_pts; at += kWalkChunk) {
        const int64_t m = n_pts - at < kWalkChunk ? n_pts - at : kWalkChunk;
        const dim3 grid(blocks(m, kWalkBlock)), block(kWalkBlock);
        hipLaunchKernelGGL(locate_walk, grid, block, lds, stream, T, n_tri,
                           normals, idx_out, boxes, n_nodes, xyz, tri, m,
                           points + 3 * at, tol, found_out + at,
                           weights_out + 3 * at);
        REMAP_HIP_CHECK(hipGetLastError());
    }
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
    Layout lay;
    const int rc = make_layout(n_tri, &lay);
    if (rc != REMAP_OK)
        return rc;
    *bytes_out = lay.total;
    return REMAP_OK;
}

int locate(const double *xyz, int64_t n_nodes, const int32_t *tri,
           int64_t n_tri, const double *points, int64_t n_pts, double tol,
           int32_t *found_out, double *weights_out, void *workspace,
           size_t workspace_bytes, hipStream_t stream, float *phase_ms)
{
    int rc = check_args(xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                        found_out, weights_out);
    if (rc != REMAP_OK)
        return rc;
    Layout lay;
    rc = make_layout(n_tri, &lay);
    if (rc != REMAP_OK)
        return rc;
    if (!workspace || workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "remap_locate: workspace of %zu bytes, need %zu",
                    workspace_bytes, lay.total);
    if (!phase_ms) {
        if (n_pts == 0)
            return REMAP_OK;
        return run(lay, xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                   found_out, weights_out, workspace, stream, nullptr);
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 4 && err == hipSuccess; ++k)
        err = hipEventCreate(&ev[k]);
    if (err == hipSuccess) {
        rc = run(lay, xyz, n_nodes, tri, n_tri, points, n_pts, tol,
                 found_out, weights_out, workspace, stream, ev);
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
