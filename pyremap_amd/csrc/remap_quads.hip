// remap_quads.hip -- point location for `bilinear` maps from a grid given by
// 2-D arrays of cell centres: for every destination point the quad of four
// neighbouring centres whose bilinear patch the ray from the sphere's centre
// through the point meets, the lowest quad index where several do, and the
// patch's bilinear weights of its four corners.
//
// Definition (exact).  nodes (ny, nx, 3) fp64 unit vectors of the centres,
// ny >= 2, nx >= 2; periodic 0 or 1 (with 1 column nx-1 closes onto column
// 0); points (n_pts, 3) fp64; tol >= 0.  Nodes and points are unit vectors to
// within 1e-6.  nqx = nx - 1 + periodic, and quad k = j*nqx + i has the
// corners p0 = (j, i), p1 = (j, i1), p2 = (j+1, i1), p3 = (j+1, i) with
// i1 = (i+1) % nx.  With
//   cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
//   dot(u, v)   = (u.x*v.x + u.y*v.y) + u.z*v.z
// in IEEE fp64 in that order (the library is built -ffp-contract=off), the
// patch X(s, t) = c0 + s*c1 + t*c2 + s*t*c3 has, component by component,
//   c0 = 0.25*(((p0+p1)+p2)+p3)      c1 = 0.25*(((p1-p0)+p2)-p3)
//   c2 = 0.25*(((p2-p0)-p1)+p3)      c3 = 0.25*(((p0-p1)+p2)-p3)
// Newton on X(s, t) - r*q = 0, per point and per quad: start at s = t = 0,
// r = 1; at most 12 steps, each
//   F = (((c0 + s*c1) + t*c2) + (s*t)*c3) - r*q
//   a = c1 + t*c3,  b = c2 + s*c3,  bq = cross(b, q),  det = -dot(a, bq)
//   d0 = dot(F, bq)/det,  d1 = dot(a, cross(F, q))/det,
//   d2 = -dot(a, cross(b, F))/det
//   s += d0, t += d1, r += d2
//   !(|s| <= 50) or !(|t| <= 50): the quad holds nothing
//   an earlier step had max(|d0|, |d1|) <= 1e-8: this step was the polish,
//   the solve is DONE; otherwise a step with max(|d0|, |d1|) <= 1e-8 asks for
//   exactly one more step
// and a solve not done after 12 steps holds nothing.
//   holds(q, k)  iff  done, |s| <= 1 + tol, |t| <= 1 + tol and r > 0
//   a quad with a non-finite corner holds nothing
//   found[q] = the LOWEST k that holds q, or -1
//   weights of the winner, s and t clipped to [-1, 1]:
//   0.25*(1-s)*(1-t), 0.25*(1+s)*(1-t), 0.25*(1+s)*(1+t), 0.25*(1-s)*(1+t)
//   for p0..p3; zeros where found is -1.
// The result is a pure function of the inputs; numpy reproduces it bit for
// bit (weights.locate_in_quads).
//
// Pipeline (all on the caller's stream, nothing synchronises, no atomics):
//   centre_keys    63-bit Morton code of every quad's c0 (a quad with a
//                  non-finite corner: key 0)
//   radix sort     rocPRIM radix_sort_pairs on (key, original index)
//   setup          one lane per sorted quad: its c0..c3 (NaN for a quad that
//                  holds nothing: the Newton then leaves at its first step)
//                  and its box; the boxes of the kLeaf quads of a leaf are
//                  joined across lanes, which gives level 0 of the tree
//   upper_boxes    one launch a level (remap_tree.h)
//   quad_walk      one lane per point, 64-lane blocks, depth first, the stack
//                  in LDS laid out [entry][lane].  A node is entered only if
//                  q lies in its box.  At a leaf a quad numbered above the
//                  best so far is skipped unread; the others run the Newton
//                  above on the stored coefficients (the same operations on
//                  the same numbers as the definition's).  The winner's
//                  weights are then computed from `nodes` by the definition's
//                  own operations.
//
// Why the pruning is exact.  A quad may be skipped only if holds() rejects
// the point.  The box of a quad is the box of its four corners widened on
// every side by
//   m_k = d^2/2 + 2*d*(2*tol + tol^2) + 1e-5
// (d its diameter: the longest of four edges and two diagonals), and it is
// EVERYTHING unless m_k < 1 and the quad passes the shape test below.
//  * In real arithmetic a Newton step from (s', t', r') with the computed
//    (d0, d1, d2) leaves F(s, t, r) = F' + J'*d + d0*d1*c3 (X is bilinear,
//    F linear in r).  Where the solve of J'*d = -F' is accurate, the iterate
//    after a step of max(|d0|, |d1|) <= 1e-8 has |F| <= 1e-16*|c3| plus the
//    solve's residual, and the polish moves it by |F|*cond, where
//      cond = |a|*|b|*|q| / |dot(q, cross(a, b))|
//    is the condition of Cramer's rule on J = [a, b, -q].
//  * cross(a, b) = cross(c1, c2) + s*cross(c1, c3) + t*cross(c3, c2) and, at
//    a point of the ray, r*dot(q, cross(a, b)) = dot(X, cross(a, b)) =
//      g(s, t) = D0 + s*D1 + t*D2 - s*t*D3,
//      D0 = dot(c0, cross(c1, c2)), D1 = dot(c0, cross(c1, c3)),
//      D2 = dot(c0, cross(c3, c2)), D3 = dot(c3, cross(c1, c2)):
//    bilinear, so over the square |s|, |t| <= L it is bounded away from zero
//    by its values at the four corners of the square when these share a
//    sign.  (At L = 1 they are the triple products p0.(p1 x p3)/4, ...: the
//    quad seen from the centre is convex and not folded.)  The shape test:
//    with L = 1.25 + tol, A = |c1| + L*|c3| >= |a|, B = |c2| + L*|c3| >= |b|,
//    the four g(+-L, +-L) share a sign and min |g| * 1e3 >= A*B*(1 + 1e-6)
//    (|X| <= 1 + 1e-6 + stretch).  Then cond <= 1e3 on the whole square, a
//    residual of 1e-13 moves the polish by 1e-10 at most, and the iterate
//    that holds() sees is within 1e-9 of a true root (s*, t*, r*) with
//    |s*|, |t*| <= 1 + tol + 1e-9 and r* > 0: the 1e-5 of m_k has 7e-6 to
//    spare for it.  A polish of more than 0.25 from an iterate outside that
//    square would need a residual no accurate solve leaves; where the solve
//    is not accurate (cond above 1e3 somewhere on the square: a flat,
//    folded or collapsed quad) the quad is not trusted to a box and is
//    tested against every point.
//  * A true root with r* > 0 has q = X(s*, t*)/r*.  X(s*, t*) is within
//    e = (tol + 1e-9)*(|c1| + |c2|) + ((1 + tol + 1e-9)^2 - 1)*|c3| <=
//    d*(2*tol + tol^2/2) + 3e-9 (every |c_i| <= d/2) of p' = X(clipped s*,
//    clipped t*), a convex combination of the corners.
//  * |p'| <= 1 + 1e-6, and with p' = sum_k beta_k p_k: |p'|^2 = sum_k
//    beta_k |p_k|^2 - (1/2) sum_jk beta_j beta_k |p_j - p_k|^2 >=
//    (1 - 1e-6)^2 - d^2/2.  r* > 0 puts q on the ray of Y = X(s*, t*), so
//    |q - Y| = ||q| - |Y||, and with 1 - sqrt(1 - x) <= x:
//    |q - p'| <= d^2/2 + 3e-6 + 2*e.
//  * So every coordinate of q is within d^2/2 + 2*d*(2*tol + tol^2) + 3e-6 +
//    1e-8 of the corners' box; m_k covers it with the spare for its own
//    roundings, the box's ends and the pyramid's (min and max are exact).
// The margin is the quad's own, so a grid with one fine row is not widened
// by its coarse ones.  Outside the 1e-6 contract the result is unspecified;
// the walk still ends (the stack is bounded by the tree's shape, the Newton
// by its 12 steps) and reads nothing outside its arrays.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_common.h"
#include "remap_tree.h"

namespace remap {
namespace {

// (kWalkBlock lanes a walking block, kWalkChunk points a launch: remap_tree.h)
// every child whose box holds the point is stacked, then one is popped: at
// most kFan - 1 stay behind a level above level 0, and kFan at the last
constexpr int stack_depth(int levels) { return (kFan - 1) * (levels - 1) + 1; }
constexpr uint32_t kNoQuad = 0xffffffffu;
constexpr int kNewtonSteps = 12;

static_assert(kBlock % kLeaf == 0 && kWave % kLeaf == 0 &&
              (kLeaf & (kLeaf - 1)) == 0,
              "setup joins a leaf's boxes across kLeaf neighbouring lanes");
static_assert(stack_depth(kMaxLevels) * kWalkBlock * 4 <= 64 * 1024,
              "the walk's stack must fit in a workgroup's LDS");

// the grid: nqx quads a row, n_quads in all
struct Grid {
    int64_t ny, nx, nqx, n_quads;
};

// (ny, nx, periodic) checked: the grid, or false
bool make_grid(int64_t ny, int64_t nx, int32_t periodic, Grid *g)
{
    if (ny < 2 || nx < 2 || (periodic != 0 && periodic != 1) ||
        ny > INT32_MAX || nx > INT32_MAX - 1)
        return false;
    g->ny = ny;
    g->nx = nx;
    g->nqx = nx - 1 + periodic;
    g->n_quads = (ny - 1) * g->nqx;            // < 2^62
    return g->n_quads <= INT32_MAX;
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

__device__ inline bool finite3(const Vec3 &u)
{
    return u.x - u.x == 0.0 && u.y - u.y == 0.0 && u.z - u.z == 0.0;
}

struct Patch {
    Vec3 c0, c1, c2, c3;
};

// the corners of quad k (0 <= k < n_quads); false if one is not finite
__device__ inline bool corners(const Grid &G, int64_t k,
                               const double *__restrict__ nodes, Vec3 &p0,
                               Vec3 &p1, Vec3 &p2, Vec3 &p3)
{
    const int64_t j = k / G.nqx, i = k - j * G.nqx;
    const int64_t i1 = i + 1 == G.nx ? 0 : i + 1;
    p0 = load3(nodes, j * G.nx + i);
    p1 = load3(nodes, j * G.nx + i1);
    p2 = load3(nodes, (j + 1) * G.nx + i1);
    p3 = load3(nodes, (j + 1) * G.nx + i);
    return finite3(p0) && finite3(p1) && finite3(p2) && finite3(p3);
}

__device__ inline Patch patch_of(const Vec3 &p0, const Vec3 &p1,
                                 const Vec3 &p2, const Vec3 &p3)
{
    Patch P;
#define REMAP_QUADS_AXIS(a)                                                  \
    P.c0.a = 0.25 * (((p0.a + p1.a) + p2.a) + p3.a);                         \
    P.c1.a = 0.25 * (((p1.a - p0.a) + p2.a) - p3.a);                         \
    P.c2.a = 0.25 * (((p2.a - p0.a) - p1.a) + p3.a);                         \
    P.c3.a = 0.25 * (((p0.a - p1.a) + p2.a) - p3.a);
    REMAP_QUADS_AXIS(x)
    REMAP_QUADS_AXIS(y)
    REMAP_QUADS_AXIS(z)
#undef REMAP_QUADS_AXIS
    return P;
}

// the definition's Newton: whether the solve is done, and its (s, t, r)
__device__ inline bool solve(const Patch &P, const Vec3 &q, double &s,
                             double &t, double &r)
{
    s = 0.0;
    t = 0.0;
    r = 1.0;
    bool polish = false;
#pragma unroll 1
    for (int step = 0; step < kNewtonSteps; ++step) {
        const double st = s * t;
        const Vec3 F{
            (((P.c0.x + s * P.c1.x) + t * P.c2.x) + st * P.c3.x) - r * q.x,
            (((P.c0.y + s * P.c1.y) + t * P.c2.y) + st * P.c3.y) - r * q.y,
            (((P.c0.z + s * P.c1.z) + t * P.c2.z) + st * P.c3.z) - r * q.z};
        const Vec3 a{P.c1.x + t * P.c3.x, P.c1.y + t * P.c3.y,
                     P.c1.z + t * P.c3.z};
        const Vec3 b{P.c2.x + s * P.c3.x, P.c2.y + s * P.c3.y,
                     P.c2.z + s * P.c3.z};
        const Vec3 bq = cross(b, q);
        const double det = -dot(a, bq);
        const double d0 = dot(F, bq) / det;
        const double d1 = dot(a, cross(F, q)) / det;
        const double d2 = -dot(a, cross(b, F)) / det;
        s += d0;
        t += d1;
        r += d2;
        if (!(fabs(s) <= 50.0) || !(fabs(t) <= 50.0))
            return false;
        if (polish)
            return true;
        polish = fabs(d0) <= 1e-8 && fabs(d1) <= 1e-8;
    }
    return false;
}

__device__ inline bool holds(const Patch &P, const Vec3 &q, double tol,
                             double &s, double &t)
{
    double r;
    const double lim = 1.0 + tol;
    return solve(P, q, s, t, r) && fabs(s) <= lim && fabs(t) <= lim &&
           r > 0.0;
}

__global__ __launch_bounds__(kBlock) void centre_keys(
    Grid G, const double *__restrict__ nodes, uint64_t *__restrict__ keys,
    uint32_t *__restrict__ idx)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= G.n_quads)
        return;
    Vec3 p0, p1, p2, p3;
    uint64_t key = 0;
    if (corners(G, k, nodes, p0, p1, p2, p3)) {
        const Patch P = patch_of(p0, p1, p2, p3);
        key = morton_key(P.c0.x, P.c0.y, P.c0.z);
    }
    keys[k] = key;
    idx[k] = static_cast<uint32_t>(k);
}

__device__ inline double min4(double a, double b, double c, double d)
{
    return fmin(fmin(a, b), fmin(c, d));
}

__device__ inline double max4(double a, double b, double c, double d)
{
    return fmax(fmax(a, b), fmax(c, d));
}

__device__ inline double edge2(const Vec3 &u, const Vec3 &v)
{
    const double dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// the shape test of the file's head: whether the box of this quad may stand
// for it (any NaN answers no)
__device__ inline bool trusted(const Patch &P, double tol)
{
    const double L = 1.25 + tol;
    const Vec3 n12 = cross(P.c1, P.c2);
    const double D0 = dot(P.c0, n12), D1 = dot(P.c0, cross(P.c1, P.c3)),
                 D2 = dot(P.c0, cross(P.c3, P.c2)), D3 = dot(P.c3, n12);
    const double LL = L * L;
    const double g0 = (D0 - L * D1 - L * D2) - LL * D3;     // (-L, -L)
    const double g1 = (D0 + L * D1 - L * D2) + LL * D3;     // ( L, -L)
    const double g2 = (D0 + L * D1 + L * D2) - LL * D3;     // ( L,  L)
    const double g3 = (D0 - L * D1 + L * D2) + LL * D3;     // (-L,  L)
    const bool pos = g0 > 0.0 && g1 > 0.0 && g2 > 0.0 && g3 > 0.0;
    const bool neg = g0 < 0.0 && g1 < 0.0 && g2 < 0.0 && g3 < 0.0;
    if (!pos && !neg)
        return false;
    const double least = fmin(fmin(fabs(g0), fabs(g1)),
                              fmin(fabs(g2), fabs(g3)));
    const double l3 = L * sqrt(dot(P.c3, P.c3));
    const double A = sqrt(dot(P.c1, P.c1)) + l3;
    const double B = sqrt(dot(P.c2, P.c2)) + l3;
    return least * 1e3 >= A * B * (1.0 + 1e-6);
}

// one lane per sorted quad; the lanes past the last quad of the last leaf
// stay in for the joins with an empty box
__global__ __launch_bounds__(kBlock) void setup(
    Grid G, const double *__restrict__ nodes,
    const uint32_t *__restrict__ orig, double tol, double *__restrict__ coef,
    double *__restrict__ boxes)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double inf = __builtin_huge_val();
    double box[6] = {inf, inf, inf, -inf, -inf, -inf};   // holds no point
    if (k < G.n_quads) {
        const double nan = __builtin_nan("");
        Patch P{Vec3{nan, nan, nan}, Vec3{nan, nan, nan},
                Vec3{nan, nan, nan}, Vec3{nan, nan, nan}};
        Vec3 p0, p1, p2, p3;
        const int64_t id = orig[k];
        if (id < G.n_quads && corners(G, id, nodes, p0, p1, p2, p3)) {
            P = patch_of(p0, p1, p2, p3);
            const double d2 = fmax(
                max4(edge2(p0, p1), edge2(p1, p2), edge2(p2, p3),
                     edge2(p3, p0)),
                fmax(edge2(p0, p2), edge2(p1, p3)));
            const double m = 0.5 * d2 +
                             2.0 * sqrt(d2) * (2.0 * tol + tol * tol) + 1e-5;
            if (m < 1.0 && trusted(P, tol)) {
                box[0] = min4(p0.x, p1.x, p2.x, p3.x) - m;
                box[1] = min4(p0.y, p1.y, p2.y, p3.y) - m;
                box[2] = min4(p0.z, p1.z, p2.z, p3.z) - m;
                box[3] = max4(p0.x, p1.x, p2.x, p3.x) + m;
                box[4] = max4(p0.y, p1.y, p2.y, p3.y) + m;
                box[5] = max4(p0.z, p1.z, p2.z, p3.z) + m;
            } else {
                box[0] = box[1] = box[2] = -inf;         // holds every point
                box[3] = box[4] = box[5] = inf;
            }
        }
        double *o = coef + k * 12;
        o[0] = P.c0.x; o[1] = P.c0.y; o[2] = P.c0.z;
        o[3] = P.c1.x; o[4] = P.c1.y; o[5] = P.c1.z;
        o[6] = P.c2.x; o[7] = P.c2.y; o[8] = P.c2.z;
        o[9] = P.c3.x; o[10] = P.c3.y; o[11] = P.c3.z;
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
    if (k < G.n_quads && k % kLeaf == 0) {
        double *o = boxes + (k / kLeaf) * 6;
#pragma unroll
        for (int a = 0; a < 6; ++a)
            o[a] = box[a];
    }
}

// (in_box, push_children: remap_tree.h)

// one lane per point
__global__ __launch_bounds__(kWalkBlock) void quad_walk(
    Tree T, Grid G, const double *__restrict__ coef,
    const uint32_t *__restrict__ orig, const double *__restrict__ boxes,
    const double *__restrict__ nodes, int64_t n_pts,
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
    uint32_t best = kNoQuad;
    int top = 0;
    if (in_box(boxes + T.first[T.levels - 1] * 6, q))
        stack[top++][lane] = static_cast<uint32_t>(T.levels - 1) << kNodeBits;
    while (top > 0) {
        const uint32_t cur = stack[--top][lane];
        const int l = static_cast<int>(cur >> kNodeBits);
        const int64_t k = cur & kNodeMask;
        if (l == 0) {
            const int64_t e0 = k * kLeaf;
            const int64_t e1 = e0 + kLeaf < G.n_quads ? e0 + kLeaf
                                                      : G.n_quads;
#pragma unroll 1
            for (int64_t e = e0; e < e1; ++e) {
                const uint32_t id = orig[e];
                if (id >= best)
                    continue;
                const double *c = coef + e * 12;
                const Patch P{Vec3{c[0], c[1], c[2]}, Vec3{c[3], c[4], c[5]},
                              Vec3{c[6], c[7], c[8]},
                              Vec3{c[9], c[10], c[11]}};
                double s, t;
                if (holds(P, q, tol, s, t))
                    best = id;
            }
            continue;
        }
        push_children(T, boxes, l, k, q, stack, lane, top);
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0;
    int32_t out = -1;
    Vec3 p0, p1, p2, p3;
    if (best < G.n_quads && corners(G, best, nodes, p0, p1, p2, p3)) {
        // the definition, on the winner alone
        double s, t;
        if (holds(patch_of(p0, p1, p2, p3), q, tol, s, t)) {
            s = fmin(fmax(s, -1.0), 1.0);
            t = fmin(fmax(t, -1.0), 1.0);
            S0 = 0.25 * (1.0 - s) * (1.0 - t);
            S1 = 0.25 * (1.0 + s) * (1.0 - t);
            S2 = 0.25 * (1.0 + s) * (1.0 + t);
            S3 = 0.25 * (1.0 - s) * (1.0 + t);
            out = static_cast<int32_t>(best);
        }
    }
    found[w] = out;
    weights[4 * w] = S0;
    weights[4 * w + 1] = S1;
    weights[4 * w + 2] = S2;
    weights[4 * w + 3] = S3;
}

int check_args(const char *what, int64_t ny, int64_t nx, int32_t periodic,
               int64_t n_pts, Grid *g)
{
    if (!make_grid(ny, nx, periodic, g) || n_pts < 0)
        return fail(REMAP_ERR_ARG,
                    "%s: ny %lld, nx %lld (>= 2, at most 2^31 - 1 quads), "
                    "periodic %d (0 or 1), n_pts %lld (>= 0)", what,
                    static_cast<long long>(ny), static_cast<long long>(nx),
                    static_cast<int>(periodic),
                    static_cast<long long>(n_pts));
    return REMAP_OK;
}

// a leaf holds its quads' four bilinear coefficients
constexpr size_t kPayload = 96;

// the three phases; ev (NULL, or 4 events) is recorded around them
int run(const TreeLayout &lay, const Grid &G, const double *nodes,
        const double *points, int64_t n_pts, double tol, int32_t *found_out,
        double *weights_out, void *workspace, hipStream_t stream,
        hipEvent_t *ev)
{
    const TreeArrays A = tree_arrays(lay, workspace);
    const Tree &T = lay.tree;
    const int64_t n = G.n_quads;
    REMAP_TRY(build_tree(
        lay, A, n, workspace, stream, ev,
        [&] {
            return launch(centre_keys, n, kBlock, stream, G, nodes, A.keys_in,
                          A.idx_in);
        },
        nothing_sorted,
        [&] {
            return launch(setup, n, kBlock, stream, G, nodes, A.orig, tol,
                          A.payload, A.boxes);
        }));
    const size_t lds = size_t(stack_depth(T.levels)) * kWalkBlock * 4;
    REMAP_TRY(walk_chunks(n_pts, [&](int64_t at, int64_t m) {
        return launch_blocks(quad_walk, blocks(m, kWalkBlock), kWalkBlock,
                             lds, stream, T, G, A.payload, A.orig, A.boxes,
                             nodes, m, points + 3 * at, tol, found_out + at,
                             weights_out + 4 * at);
    }));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    return REMAP_OK;
}

}  // namespace

int quads_workspace(int64_t ny, int64_t nx, int32_t periodic, int64_t n_pts,
                    size_t *bytes_out)
{
    if (!bytes_out)
        return fail(REMAP_ERR_ARG, "remap_quads_workspace: NULL output");
    Grid G;
    REMAP_TRY(check_args("remap_quads_workspace", ny, nx, periodic, n_pts,
                         &G));
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(G.n_quads, kPayload, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int quads(const double *nodes, int64_t ny, int64_t nx, int32_t periodic,
          const double *points, int64_t n_pts, double tol, int32_t *found_out,
          double *weights_out, void *workspace, size_t workspace_bytes,
          hipStream_t stream, float *phase_ms)
{
    Grid G;
    REMAP_TRY(check_args("remap_quads", ny, nx, periodic, n_pts, &G));
    if (!(tol >= 0.0))
        return fail(REMAP_ERR_ARG, "remap_quads: tol %g (>= 0)", tol);
    if (!nodes || (n_pts > 0 && (!points || !found_out || !weights_out)))
        return fail(REMAP_ERR_ARG, "remap_quads: NULL array");
    TreeLayout lay;
    REMAP_TRY(make_tree_layout(G.n_quads, kPayload, &lay));
    REMAP_TRY(need_workspace("remap_quads", workspace, workspace_bytes,
                             lay.total));
    if (!phase_ms) {
        if (n_pts == 0)
            return REMAP_OK;
        return run(lay, G, nodes, points, n_pts, tol, found_out, weights_out,
                   workspace, stream, nullptr);
    }
    return timed_phases<4>(phase_ms, [&](hipEvent_t *ev) {
        return run(lay, G, nodes, points, n_pts, tol, found_out, weights_out,
                   workspace, stream, ev);
    });
}

}  // namespace remap

extern "C" {

int remap_quads_workspace(int64_t ny, int64_t nx, int32_t periodic,
                          int64_t n_pts, size_t *bytes_out)
{
    return remap::quads_workspace(ny, nx, periodic, n_pts, bytes_out);
}

int remap_quads(const double *nodes, int64_t ny, int64_t nx, int32_t periodic,
                const double *points, int64_t n_pts, double tol,
                int32_t *found_out, double *weights_out, void *workspace,
                size_t workspace_bytes, void *stream)
{
    return remap::quads(nodes, ny, nx, periodic, points, n_pts, tol,
                        found_out, weights_out, workspace, workspace_bytes,
                        static_cast<hipStream_t>(stream), nullptr);
}

int remap_quads_timed(const double *nodes, int64_t ny, int64_t nx,
                      int32_t periodic, const double *points, int64_t n_pts,
                      double tol, int32_t *found_out, double *weights_out,
                      void *workspace, size_t workspace_bytes,
                      float *phase_ms_out, void *stream)
{
    if (!phase_ms_out)
        return remap::fail(REMAP_ERR_ARG, "remap_quads_timed: NULL output");
    return remap::quads(nodes, ny, nx, periodic, points, n_pts, tol,
                        found_out, weights_out, workspace, workspace_bytes,
                        static_cast<hipStream_t>(stream), phase_ms_out);
}

}  // extern "C"
