// What the overlap kernels (remap_overlap.hip) and the overlap moments
// (remap_conserve2nd.hip) share: a cell's prepared ring (finish_ring), the
// convexity test of a clipper (convex_cell) and the clip -- a polygon in the
// gnomonic plane of a centre, in one lane's LDS ring [buffer][vertex][lane]
// (ping-pong), cut by one directed edge at a time.  One set of device
// functions, so a prepared cell and a clipped polygon have the same corners
// wherever they are made.
#ifndef REMAP_CLIP_H
#define REMAP_CLIP_H

#include <hip/hip_runtime.h>

#include "remap_hip.h"
#include "remap_sphere.h"

namespace remap {

// the largest nEdgesOnCell this build serves (MPAS meshes have at most 9 or
// so)
constexpr int kMaxEdges = REMAP_OVERLAP_MAX_EDGES;
// lanes of a clip block: one pair each
constexpr int kClipBlock = 64;
// every vertex of a pair must be within acos(kMinCos) ~ 84 deg of the
// subject's centre for the gnomonic projection (REMAP_OVERLAP_ERR_HEMISPHERE)
constexpr double kMinCos = 0.1;

// the tangent plane at a centre: great circles are straight lines in it
struct Tangent {
    V3 cc, e1, e2;
    // (x, y) of p in the plane and t, the cosine of its angle to the centre
    // (the projection reaches t >= kMinCos)
    __device__ void project(V3 p, double *x, double *y, double *t) const
    {
        *t = dot(p, cc);
        *x = dot(p, e1) / *t;
        *y = dot(p, e2) / *t;
    }
};

__device__ inline Tangent tangent_at(V3 cc)
{
    const V3 ref = fabs(cc.z) < 0.9 ? V3{0.0, 0.0, 1.0} : V3{1.0, 0.0, 0.0};
    const V3 e1 = normalized(cross(ref, cc));
    return {cc, e1, cross(cc, e1)};
}

// the subject: a prepared cell's nv vertices (v: its row of cell_xyz) into
// buffer 0 of the ring; false when one is beyond the projection's reach
template <int kCap>
__device__ inline bool load_ring(const Tangent &T, const double *v, int nv,
                                 double (&px)[2][kCap][kClipBlock],
                                 double (&py)[2][kCap][kClipBlock], int lane)
{
    bool bad = false;
    for (int k = 0; k < kMaxEdges; ++k) {
        if (k < nv) {
            double x, y, t;
            T.project({v[3 * k], v[3 * k + 1], v[3 * k + 2]}, &x, &y, &t);
            bad |= !(t >= kMinCos);
            px[0][k][lane] = x;
            py[0][k][lane] = y;
        }
    }
    return !bad;
}

// One Sutherland-Hodgman pass: the n vertices of buffer cur against the
// half-plane left of the edge from (ax, ay) along (dx, dy), into the other
// buffer.  Returns the new count m; no slot at or past kCap is written, and
// m > kCap is the caller's kErrClip.
template <int kCap>
__device__ inline int clip_edge(double (&px)[2][kCap][kClipBlock],
                                double (&py)[2][kCap][kClipBlock], int lane,
                                int cur, int n, double ax, double ay,
                                double dx, double dy)
{
    const int nxt = cur ^ 1;
    int m = 0;
    double sx = px[cur][n - 1][lane], sy = py[cur][n - 1][lane];
    double ss = dx * (sy - ay) - dy * (sx - ax);
    for (int k = 0; k < n; ++k) {
        const double ex = px[cur][k][lane], ey = py[cur][k][lane];
        const double se = dx * (ey - ay) - dy * (ex - ax);
        if ((se >= 0.0) != (ss >= 0.0)) {
            if (m < kCap) {
                const double t = ss / (ss - se);
                px[nxt][m][lane] = sx + t * (ex - sx);
                py[nxt][m][lane] = sy + t * (ey - sy);
            }
            ++m;
        }
        if (se >= 0.0) {
            if (m < kCap) {
                px[nxt][m][lane] = ex;
                py[nxt][m][lane] = ey;
            }
            ++m;
        }
        sx = ex;
        sy = ey;
        ss = se;
    }
    return m;
}

// a cell's vertices in one lane's LDS slots (vertex k at [k * stride])
struct Ring {
    double *x, *y, *z;
    int stride;
    __device__ V3 operator[](int k) const
    {
        return {x[k * stride], y[k * stride], z[k * stride]};
    }
    __device__ void set(int k, V3 p) const
    {
        x[k * stride] = p.x;
        y[k * stride] = p.y;
        z[k * stride] = p.z;
    }
};

// A ring whose consecutive duplicates are dropped already: the closing
// duplicate dropped too, turned counter-clockwise, its area (the fan from
// vertex 0) and its centre.  Returns the error bits; *nv is 0 on an error.
__device__ inline int finish_ring(Ring xyz, int *nv_io, V3 *centre, double *area)
{
    int nv = *nv_io;
    *nv_io = 0;
    *area = 0.0;
    while (nv > 1 && xyz[nv - 1].x == xyz[0].x && xyz[nv - 1].y == xyz[0].y &&
           xyz[nv - 1].z == xyz[0].z)
        --nv;
    if (nv < 3)
        return REMAP_OVERLAP_ERR_VERTEX;
    double a = 0.0;
    for (int k = 1; k + 1 < nv; ++k)
        a += tri_area(xyz[0], xyz[k], xyz[k + 1]);
    if (a < 0.0) {
        for (int k = 1, l = nv - 1; k < l; ++k, --l) {
            const V3 t = xyz[k];
            xyz.set(k, xyz[l]);
            xyz.set(l, t);
        }
        a = -a;
    }
    *area = a;
    *nv_io = nv;
    V3 s = {0.0, 0.0, 0.0};
    for (int k = 0; k < nv; ++k)
        s = {s.x + xyz[k].x, s.y + xyz[k].y, s.z + xyz[k].z};
    *centre = normalized(s);
    return 0;
}

// a clipper vertex may lie this far (x the cell's longest edge) on the wrong
// side of another edge's great circle: collinear vertices, rounded
constexpr double kConvexTol = 1e-9;

// a prepared polygon in global memory (cell_xyz of one cell)
struct CellRing {
    const double *p;
    __device__ V3 operator[](int k) const
    {
        return {p[3 * k], p[3 * k + 1], p[3 * k + 2]};
    }
};

// every vertex on the left of every edge's great circle (counter-clockwise),
// within kConvexTol of the longest edge
template <class R>
__device__ bool convex_cell(const R &v, int nv)
{
    double len = 0.0;
    for (int k = 0; k < nv; ++k) {
        const V3 d = sub(v[k + 1 < nv ? k + 1 : 0], v[k]);
        len = fmax(len, sqrt(dot(d, d)));
    }
    for (int e = 0; e < nv; ++e) {
        const int f = e + 1 < nv ? e + 1 : 0;
        const V3 n = cross(v[e], v[f]);
        const double lim = -kConvexTol * len * sqrt(dot(n, n));
        for (int k = 0; k < nv; ++k)
            if (k != e && k != f && dot(n, v[k]) < lim)
                return false;
    }
    return true;
}

}  // namespace remap

#endif  // REMAP_CLIP_H
