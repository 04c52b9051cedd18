// remap_overlap.hip -- first-order conservative overlaps between an MPAS cell
// mesh and a lat-lon grid (what ESMF_RegridWeightGen --method conserve
// computes for pyremap's MPAS <-> lat-lon maps).
//
// Geometry (ESMF's convention): every cell is a spherical polygon with
// great-circle edges, lat-lon cells included -- their "lat lines" are the
// great-circle arcs between their corners.  Corners at a pole coincide, so
// the polar rows' cells are triangles (a repeated corner is a zero-length
// edge, which clips nothing and adds no area).  A_ij = spherical area of
// (mesh cell n lat-lon cell); polygon areas come from the same formula.
//
// Pipeline (all on the caller's stream, fp64 throughout, no float atomics):
//   cell_prep      one lane per mesh cell: vertices -> unit xyz (consecutive
//                  duplicates dropped, turned counter-clockwise seen from
//                  outside), the cell's own area, its centre and its
//                  (lat, lon) box -- latitude extrema of the great-circle
//                  arcs included, the poles' cells reaching +-90 deg over the
//                  whole circle -- as rows and column ranges of the grid
//   grid_area      one lane per lat-lon cell: its area
//   exclusive scan rocPRIM over the candidate counts
//   fill_pairs     one lane per mesh cell: key = mesh << 32 | grid cell
//   clip_pairs     one lane per candidate: gnomonic projection about the
//                  mesh cell's centre (great circles -> straight lines),
//                  Sutherland-Hodgman of the mesh polygon by the lat-lon
//                  cell's four edges in that plane, area of the result from
//                  its 3-D vertices (fan of Van Oosterom-Strackee triangles)
//   flag / scan / scatter  keep A_ij > kSliver * A_dst; re-key (dst, src)
//   radix sort     rocPRIM radix_sort_pairs on (dst << 32 | src, A)
//   dst_sums       one lane per destination cell: its entries summed in that
//                  order -> frac_b = min(sum / A_dst, 1)
// The polygons being clipped live in per-lane LDS slots (runtime-indexed
// private arrays would go to scratch on gfx950).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "remap_common.h"

namespace remap {
namespace {

// the largest nEdgesOnCell this build serves (MPAS meshes have at most 9 or
// so); one clip by a half-plane adds at most one vertex: four lat-lon edges.
// Rounding can break that bound where mesh vertices lie on a lat-lon edge
// (their signs alternate along it); a polygon that would outgrow kMaxOut is
// an error (kErrClip), never truncated
constexpr int kMaxEdges = REMAP_OVERLAP_MAX_EDGES;
constexpr int kMaxOut = kMaxEdges + 4;
// the status bit of that error, next to REMAP_OVERLAP_ERR_* (the bits stay
// inside the library: callers see REMAP_ERR_UNSUPPORTED and the message)
constexpr int kErrClip = 16;
constexpr int kClipBlock = 64;
constexpr int kPrepBlock = 64;
// every vertex of a pair must be within acos(kMinCos) ~ 84 deg of the mesh
// cell's centre for the gnomonic projection (REMAP_OVERLAP_ERR_HEMISPHERE)
constexpr double kMinCos = 0.1;
// entries with A_ij <= kSliver * A_dst are dropped: touching along an edge
// or at a corner leaves rounding-level areas, not overlaps
constexpr double kSliver = 1e-14;
// slack of the boxes, radians (rounding of the corners' lat / lon)
constexpr double kBoxEps = 1e-9;
constexpr double kPi = 3.14159265358979323846;
constexpr double kHalfPi = 0.5 * kPi;
constexpr double kTwoPi = 2.0 * kPi;

constexpr size_t kAlign = 256;
size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct V3 {
    double x, y, z;
};

__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z,
            a.x * b.y - a.y * b.x};
}
__device__ inline V3 normalized(V3 a)
{
    const double r = sqrt(dot(a, a));
    return {a.x / r, a.y / r, a.z / r};
}

// a pole is exactly (0, 0, +-1): every corner at +-90 deg is the same point
__device__ inline V3 unit_latlon(double lat, double lon)
{
    if (lat >= kHalfPi)
        return {0.0, 0.0, 1.0};
    if (lat <= -kHalfPi)
        return {0.0, 0.0, -1.0};
    const double c = cos(lat);
    return {c * cos(lon), c * sin(lon), sin(lat)};
}

// signed area of the spherical triangle (a, b, c) (Van Oosterom-Strackee;
// the triple product from the edge vectors at a keeps its relative accuracy
// for small triangles)
__device__ inline double tri_area(V3 a, V3 b, V3 c)
{
    const double num = dot(a, cross(sub(b, a), sub(c, a)));
    const double den = 1.0 + dot(a, b) + dot(b, c) + dot(c, a);
    return 2.0 * atan2(num, den);
}

// the lat-lon cell with 0-based index g = j * n_lon + i, corners SW, SE, NE,
// NW (swapped to SW, NW, NE, SE when exactly one axis descends, so that the
// order is counter-clockwise seen from outside)
struct Quad {
    V3 p[4];
};

__device__ inline Quad grid_cell(const double *lat_c, const double *lon_c,
                                 int64_t n_lon, int64_t g, bool swap)
{
    const int64_t j = g / n_lon, i = g - j * n_lon;
    const double s = lat_c[j], n = lat_c[j + 1];
    const double w = lon_c[i], e = lon_c[i + 1];
    Quad q;
    q.p[0] = unit_latlon(s, w);
    q.p[1] = unit_latlon(swap ? n : s, swap ? w : e);
    q.p[2] = unit_latlon(n, e);
    q.p[3] = unit_latlon(swap ? s : n, swap ? e : w);
    return q;
}

__device__ inline double quad_area(const Quad &q)
{
    return tri_area(q.p[0], q.p[1], q.p[2]) + tri_area(q.p[0], q.p[2], q.p[3]);
}

// index k of the interval [e_k, e_{k+1}] (edges monotone, either way) that
// holds x; -1 / n past the ends
__device__ inline int64_t locate(const double *e, int64_t n, double x)
{
    const bool desc = e[n] < e[0];
    if (desc ? x > e[0] : x < e[0])
        return -1;
    if (desc ? x < e[n] : x > e[n])
        return n;
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (desc ? e[mid] >= x : e[mid] <= x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// cells [k0, k1] of the edges e (n cells) that meet the value range [x0, x1]
// (x0 <= x1); false if none
__device__ inline bool cells_in(const double *e, int64_t n, double x0,
                                double x1, int32_t *k0, int32_t *k1)
{
    const double lo = fmin(e[0], e[n]), hi = fmax(e[0], e[n]);
    if (x1 < lo || x0 > hi)
        return false;
    int64_t a = locate(e, n, fmax(x0, lo)), b = locate(e, n, fmin(x1, hi));
    a = a < 0 ? 0 : (a >= n ? n - 1 : a);
    b = b < 0 ? 0 : (b >= n ? n - 1 : b);
    *k0 = static_cast<int32_t>(a < b ? a : b);
    *k1 = static_cast<int32_t>(a < b ? b : a);
    return true;
}

struct Geom {
    int64_t n_cells, n_vertices, n_lat, n_lon;
    int32_t max_edges;
    double lat_slack;
    const int32_t *voc, *noc;
    const double *lat_v, *lon_v, *lat_c, *lon_c;
};

// the box of one cell as grid index ranges: rows [r0, r1], columns
// [a0, a1] and [b0, b1] (b empty when b0 > b1)
struct Box {
    int32_t r0, r1, a0, a1, b0, b1;
};

__device__ inline int64_t box_count(const Box &b)
{
    if (b.r0 > b.r1 || b.a0 > b.a1)
        return 0;
    const int64_t cols = (b.a1 - b.a0 + 1) + (b.b0 <= b.b1 ? b.b1 - b.b0 + 1 : 0);
    return static_cast<int64_t>(b.r1 - b.r0 + 1) * cols;
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

// One mesh cell: its vertices (deduplicated, counter-clockwise) into xyz,
// its centre, area and box.  Returns the error bits.
__device__ int prep_cell(const Geom &G, int64_t c, Ring xyz, int *nv_out,
                         V3 *centre, double *area, Box *box)
{
    *nv_out = 0;
    *area = 0.0;
    *box = {0, -1, 0, -1, 0, -1};
    const int ne = G.noc[c];
    if (ne > kMaxEdges || ne > G.max_edges)
        return REMAP_OVERLAP_ERR_EDGES;
    if (ne < 3)
        return REMAP_OVERLAP_ERR_VERTEX;
    const int32_t *row = G.voc + c * G.max_edges;
    int nv = 0;
    for (int k = 0; k < ne; ++k) {
        const int32_t v = row[k] - 1;
        if (v < 0 || v >= G.n_vertices)
            return REMAP_OVERLAP_ERR_VERTEX;
        const V3 p = unit_latlon(G.lat_v[v], G.lon_v[v]);
        if (nv > 0) {
            const V3 q = xyz[nv - 1];
            if (p.x == q.x && p.y == q.y && p.z == q.z)
                continue;
        }
        xyz.set(nv++, p);
    }
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
    *nv_out = nv;
    V3 s = {0.0, 0.0, 0.0};
    for (int k = 0; k < nv; ++k)
        s = {s.x + xyz[k].x, s.y + xyz[k].y, s.z + xyz[k].z};
    const V3 cc = normalized(s);
    *centre = cc;

    // latitude: the vertices, the arcs' extrema, the poles inside
    double zmin = 1.0, zmax = -1.0;
    bool north = true, south = true, at_pole = false;
    for (int k = 0; k < nv; ++k) {
        const V3 p = xyz[k], q = xyz[k + 1 < nv ? k + 1 : 0];
        zmin = fmin(zmin, p.z);
        zmax = fmax(zmax, p.z);
        at_pole |= p.x == 0.0 && p.y == 0.0;
        const V3 n = cross(p, q);
        // the poles are left of every (counter-clockwise) edge when inside
        north &= n.z >= 0.0;
        south &= n.z <= 0.0;
        const double nn = dot(n, n);
        if (nn < 1e-300)
            continue;
        // the point of the arc's great circle farthest north: z minus its
        // component along the normal
        V3 top = {-n.z * n.x / nn, -n.z * n.y / nn, 1.0 - n.z * n.z / nn};
        const double tt = dot(top, top);
        if (tt < 1e-300)
            continue;
        top = normalized(top);
        const V3 bot = {-top.x, -top.y, -top.z};
        if (dot(cross(p, top), n) > 0.0 && dot(cross(top, q), n) > 0.0)
            zmax = fmax(zmax, top.z);
        if (dot(cross(p, bot), n) > 0.0 && dot(cross(bot, q), n) > 0.0)
            zmin = fmin(zmin, bot.z);
    }
    double lat0 = asin(fmax(-1.0, fmin(1.0, zmin)));
    double lat1 = asin(fmax(-1.0, fmin(1.0, zmax)));
    bool full = false;
    if (north || (at_pole && zmax >= 1.0)) {
        lat1 = kHalfPi;
        full = true;
    }
    if (south || (at_pole && zmin <= -1.0)) {
        lat0 = -kHalfPi;
        full = true;
    }
    lat0 -= G.lat_slack + kBoxEps;
    lat1 += G.lat_slack + kBoxEps;
    Box b = {0, -1, 0, -1, 0, -1};
    if (!cells_in(G.lat_c, G.n_lat, lat0, lat1, &b.r0, &b.r1)) {
        *box = b;
        return 0;
    }

    // longitude: away from the poles an arc's longitude runs monotonically
    // between its ends, so the vertices span the box
    const double lon_c0 = atan2(cc.y, cc.x);
    double d0 = 0.0, d1 = 0.0;
    if (!full) {
        d0 = kPi;
        d1 = -kPi;
        for (int k = 0; k < nv; ++k) {
            double d = atan2(xyz[k].y, xyz[k].x) - lon_c0;
            d -= kTwoPi * floor((d + kPi) / kTwoPi);
            d0 = fmin(d0, d);
            d1 = fmax(d1, d);
        }
        full = d1 - d0 >= kPi;
    }
    const double L0 = fmin(G.lon_c[0], G.lon_c[G.n_lon]);
    const double L1 = fmax(G.lon_c[0], G.lon_c[G.n_lon]);
    if (full) {
        // every column (a regional grid: those it has)
        b.a0 = 0;
        b.a1 = static_cast<int32_t>(G.n_lon - 1);
        *box = b;
        return 0;
    }
    double lo = lon_c0 + d0 - kBoxEps, hi = lon_c0 + d1 + kBoxEps;
    const double shift = L0 + (lo - L0 - kTwoPi * floor((lo - L0) / kTwoPi)) - lo;
    lo += shift;
    hi += shift;   // lo in [L0, L0 + 2 pi)
    bool has_a = cells_in(G.lon_c, G.n_lon, lo, fmin(hi, L1), &b.a0, &b.a1);
    bool has_b = hi - kTwoPi >= L0 &&
                 cells_in(G.lon_c, G.n_lon, L0, fmin(hi - kTwoPi, L1), &b.b0,
                          &b.b1);
    if (!has_a && has_b) {
        b.a0 = b.b0;
        b.a1 = b.b1;
        has_a = true;
        has_b = false;
    }
    if (!has_a) {
        b.r1 = b.r0 - 1;
    } else if (has_b) {
        if ((b.a0 > b.b0 ? b.a0 : b.b0) <= (b.a1 < b.b1 ? b.a1 : b.b1) + 1) {
            // the two ranges touch: one
            b.a0 = b.a0 < b.b0 ? b.a0 : b.b0;
            b.a1 = b.a1 > b.b1 ? b.a1 : b.b1;
            b.b0 = 0;
            b.b1 = -1;
        }
    } else {
        b.b0 = 0;
        b.b1 = -1;
    }
    *box = b;
    return 0;
}

__global__ __launch_bounds__(kPrepBlock) void cell_prep(
    Geom G, double *__restrict__ cell_xyz, int32_t *__restrict__ cell_nv,
    double *__restrict__ cell_centre, double *__restrict__ mesh_area,
    Box *__restrict__ boxes, uint64_t *__restrict__ counts,
    unsigned long long *__restrict__ total, int32_t *__restrict__ status)
{
    __shared__ double sx[kMaxEdges][kPrepBlock], sy[kMaxEdges][kPrepBlock],
        sz[kMaxEdges][kPrepBlock];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kPrepBlock + lane;
    if (c >= G.n_cells)
        return;
    const Ring xyz = {&sx[0][lane], &sy[0][lane], &sz[0][lane], kPrepBlock};
    int nv;
    V3 cc;
    double area;
    Box b;
    const int err = prep_cell(G, c, xyz, &nv, &cc, &area, &b);
    if (err)
        atomicOr(status, err);
    const uint64_t cnt = err ? 0 : static_cast<uint64_t>(box_count(b));
    if (total) {   // the count-only pass of remap_overlap_latlon_sizes
        if (cnt)
            atomicAdd(total, static_cast<unsigned long long>(cnt));
        return;
    }
    for (int k = 0; k < nv; ++k) {
        const V3 v = xyz[k];
        double *o = cell_xyz + (c * G.max_edges + k) * 3;
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
    }
    cell_nv[c] = err ? 0 : nv;
    cell_centre[c * 3 + 0] = cc.x;
    cell_centre[c * 3 + 1] = cc.y;
    cell_centre[c * 3 + 2] = cc.z;
    mesh_area[c] = area;
    boxes[c] = b;
    counts[c] = cnt;
}

__global__ __launch_bounds__(kBlock) void grid_area(Geom G, bool swap,
                                                   double *__restrict__ area)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= G.n_lat * G.n_lon)
        return;
    area[g] = fabs(quad_area(grid_cell(G.lat_c, G.lon_c, G.n_lon, g, swap)));
}

__global__ __launch_bounds__(kBlock) void fill_pairs(
    Geom G, const Box *__restrict__ boxes, const uint64_t *__restrict__ offs,
    int64_t capacity, uint64_t *__restrict__ keys, int32_t *__restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= G.n_cells)
        return;
    const Box b = boxes[c];
    const int64_t cnt = box_count(b);
    int64_t o = static_cast<int64_t>(offs[c]);
    if (o + cnt > capacity) {
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
        return;
    }
    if (c == G.n_cells - 1 && o + cnt != capacity)
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
    const uint64_t hi = static_cast<uint64_t>(c) << 32;
    for (int32_t r = b.r0; r <= b.r1; ++r) {
        const uint64_t base = static_cast<uint64_t>(r) * G.n_lon;
        for (int32_t i = b.a0; i <= b.a1; ++i)
            keys[o++] = hi | (base + i);
        for (int32_t i = b.b0; i <= b.b1; ++i)
            keys[o++] = hi | (base + i);
    }
}

// one lane per candidate pair: the overlap area
__global__ __launch_bounds__(kClipBlock) void clip_pairs(
    Geom G, bool swap, int64_t n_pairs, const uint64_t *__restrict__ keys,
    const double *__restrict__ cell_xyz, const int32_t *__restrict__ cell_nv,
    const double *__restrict__ cell_centre, double *__restrict__ area,
    int32_t *__restrict__ status)
{
    // the polygon being clipped, ping-pong: [buffer][vertex][lane]
    __shared__ double px[2][kMaxOut][kClipBlock];
    __shared__ double py[2][kMaxOut][kClipBlock];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kClipBlock + lane;
    if (p >= n_pairs)
        return;
    const uint64_t key = keys[p];
    const int64_t c = static_cast<int64_t>(key >> 32);
    const int64_t g = static_cast<int64_t>(key & 0xffffffffull);
    if (c >= G.n_cells || g >= G.n_lat * G.n_lon) {
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
        area[p] = 0.0;
        return;
    }
    const int nv = cell_nv[c];
    const V3 cc = {cell_centre[c * 3], cell_centre[c * 3 + 1],
                   cell_centre[c * 3 + 2]};
    // tangent-plane basis at the centre
    const V3 ref = fabs(cc.z) < 0.9 ? V3{0.0, 0.0, 1.0} : V3{1.0, 0.0, 0.0};
    const V3 e1 = normalized(cross(ref, cc));
    const V3 e2 = cross(cc, e1);
    bool bad = false;
    for (int k = 0; k < kMaxEdges; ++k) {
        if (k < nv) {
            const double *v = cell_xyz + (c * G.max_edges + k) * 3;
            const V3 q = {v[0], v[1], v[2]};
            const double t = dot(q, cc);
            bad |= !(t >= kMinCos);
            px[0][k][lane] = dot(q, e1) / t;
            py[0][k][lane] = dot(q, e2) / t;
        }
    }
    const Quad quad = grid_cell(G.lat_c, G.lon_c, G.n_lon, g, swap);
    double qx[4], qy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t = dot(quad.p[k], cc);
        bad |= !(t >= kMinCos);
        qx[k] = dot(quad.p[k], e1) / t;
        qy[k] = dot(quad.p[k], e2) / t;
    }
    if (bad) {
        atomicOr(status, REMAP_OVERLAP_ERR_HEMISPHERE);
        area[p] = 0.0;
        return;
    }
    int n = nv, cur = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double ax = qx[e], ay = qy[e];
        const double dx = qx[(e + 1) & 3] - ax, dy = qy[(e + 1) & 3] - ay;
        if (n == 0 || (dx == 0.0 && dy == 0.0))
            continue;    // (a repeated pole corner: no edge)
        const int nxt = cur ^ 1;
        int m = 0;
        double sx = px[cur][n - 1][lane], sy = py[cur][n - 1][lane];
        double ss = dx * (sy - ay) - dy * (sx - ax);
        for (int k = 0; k < n; ++k) {
            const double ex = px[cur][k][lane], ey = py[cur][k][lane];
            const double se = dx * (ey - ay) - dy * (ex - ax);
            if ((se >= 0.0) != (ss >= 0.0)) {
                if (m < kMaxOut) {
                    const double t = ss / (ss - se);
                    px[nxt][m][lane] = sx + t * (ex - sx);
                    py[nxt][m][lane] = sy + t * (ey - sy);
                }
                ++m;
            }
            if (se >= 0.0) {
                if (m < kMaxOut) {
                    px[nxt][m][lane] = ex;
                    py[nxt][m][lane] = ey;
                }
                ++m;
            }
            sx = ex;
            sy = ey;
            ss = se;
        }
        if (m > kMaxOut) {
            atomicOr(status, kErrClip);
            area[p] = 0.0;
            return;
        }
        n = m;
        cur = nxt;
    }
    double a = 0.0;
    if (n >= 3) {
        auto lift = [&](int k) {
            const double x = px[cur][k][lane], y = py[cur][k][lane];
            return normalized(V3{cc.x + x * e1.x + y * e2.x,
                                 cc.y + x * e1.y + y * e2.y,
                                 cc.z + x * e1.z + y * e2.z});
        };
        const V3 v0 = lift(0);
        V3 prev = lift(1);
        for (int k = 2; k < n; ++k) {
            const V3 v = lift(k);
            a += tri_area(v0, prev, v);
            prev = v;
        }
    }
    area[p] = a > 0.0 ? a : 0.0;
}

__global__ __launch_bounds__(kBlock) void flag_kept(
    int64_t n_pairs, int64_t n_cells, int64_t n_grid, bool dst_is_mesh,
    const uint64_t *__restrict__ keys,
    const double *__restrict__ area, const double *__restrict__ mesh_area,
    const double *__restrict__ grid_area, uint32_t *__restrict__ head)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs)
        return;
    const uint64_t key = keys[p];
    const int64_t c = static_cast<int64_t>(key >> 32);
    const int64_t g = static_cast<int64_t>(key & 0xffffffffull);
    if (c >= n_cells || g >= n_grid) {   // (flagged by clip_pairs)
        head[p] = 0u;
        return;
    }
    const double ad = dst_is_mesh ? mesh_area[c] : grid_area[g];
    head[p] = area[p] > kSliver * ad ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void scatter_kept(
    int64_t n_pairs, bool dst_is_mesh, const uint64_t *__restrict__ keys,
    const double *__restrict__ area, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ slot, uint64_t *__restrict__ keys_out,
    double *__restrict__ area_out, int64_t *__restrict__ n_kept)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs)
        return;
    if (p == n_pairs - 1)
        *n_kept = static_cast<int64_t>(slot[p]) + head[p];
    if (!head[p])
        return;
    const uint64_t key = keys[p];
    keys_out[slot[p]] = dst_is_mesh ? key : (key << 32) | (key >> 32);
    area_out[slot[p]] = area[p];
}

__global__ __launch_bounds__(kBlock) void split_keys(
    const int64_t *__restrict__ n_kept, int64_t cap,
    const uint64_t *__restrict__ keys, int32_t *__restrict__ dst,
    int32_t *__restrict__ src)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= *n_kept || p >= cap)
        return;
    dst[p] = static_cast<int32_t>(keys[p] >> 32);
    src[p] = static_cast<int32_t>(keys[p] & 0xffffffffull);
}

// frac_b of every destination cell: its entries (sorted by source) summed
// in that order
__global__ __launch_bounds__(kBlock) void dst_sums(
    int64_t n_dst, const int64_t *__restrict__ n_kept,
    const int32_t *__restrict__ dst, const double *__restrict__ area,
    const double *__restrict__ dst_area, double *__restrict__ frac_b)
{
    const int64_t d = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (d >= n_dst)
        return;
    const int64_t n = *n_kept;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (dst[mid] < d)
            lo = mid + 1;
        else
            hi = mid;
    }
    double s = 0.0;
    for (int64_t k = lo; k < n && dst[k] == d; ++k)
        s += area[k];
    const double f = dst_area[d] > 0.0 ? s / dst_area[d] : 0.0;
    frac_b[d] = f < 1.0 ? f : 1.0;
}

struct Layout {
    size_t xyz, nv, centre, boxes, counts, offs, keys, parea, head, slot,
        keys_c, area_c, keys_s, n_kept, status, temp, total;
    size_t temp_bytes;
};

int make_layout(int64_t n_cells, int32_t max_edges, int64_t n_pairs,
                Layout *lay)
{
    const size_t c = static_cast<size_t>(n_cells > 0 ? n_cells : 1);
    const size_t n = static_cast<size_t>(n_pairs > 0 ? n_pairs : 1);
    size_t scan_c = 0, scan_n = 0, sort_n = 0;
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, scan_c, static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), uint64_t(0), c,
        rocprim::plus<uint64_t>())));
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, scan_n, static_cast<const uint32_t *>(nullptr),
        static_cast<uint32_t *>(nullptr), 0u, n, rocprim::plus<uint32_t>())));
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        nullptr, sort_n, static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), static_cast<const double *>(nullptr),
        static_cast<double *>(nullptr), n, 0u, 64u)));
    size_t t = scan_c > scan_n ? scan_c : scan_n;
    lay->temp_bytes = t > sort_n ? t : sort_n;
    size_t off = 0;
    lay->xyz = off;    off += align_up(c * max_edges * 3 * 8);
    lay->nv = off;     off += align_up(c * 4);
    lay->centre = off; off += align_up(c * 3 * 8);
    lay->boxes = off;  off += align_up(c * sizeof(Box));
    lay->counts = off; off += align_up(c * 8);
    lay->offs = off;   off += align_up(c * 8);
    lay->keys = off;   off += align_up(n * 8);
    lay->parea = off;  off += align_up(n * 8);
    lay->head = off;   off += align_up(n * 4);
    lay->slot = off;   off += align_up(n * 4);
    lay->keys_c = off; off += align_up(n * 8);
    lay->area_c = off; off += align_up(n * 8);
    lay->keys_s = off; off += align_up(n * 8);
    // the entry count and the error bits side by side: one read-back
    lay->n_kept = off; off += align_up(16);
    lay->status = lay->n_kept + 8;
    lay->temp = off;   off += align_up(lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

int check_geom(const remap_overlap_geom *g, Geom *G)
{
    if (!g)
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon: NULL geometry");
    if (g->n_cells < 0 || g->n_vertices < 0 || g->n_lat < 1 || g->n_lon < 1 ||
        g->max_edges < 3 || !(g->lat_slack >= 0.0))
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon: bad sizes");
    if (g->max_edges > kMaxEdges)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_latlon: maxEdges %d exceeds the %d this "
                    "build serves (REMAP_OVERLAP_MAX_EDGES)",
                    g->max_edges, kMaxEdges);
    if (g->n_cells >= (int64_t(1) << 31) ||
        g->n_lat * g->n_lon >= (int64_t(1) << 31) ||
        g->n_lat >= (int64_t(1) << 30) || g->n_lon >= (int64_t(1) << 30))
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_latlon: sizes beyond 32-bit indices");
    if (g->n_cells > 0 && (!g->vertices_on_cell || !g->n_edges_on_cell ||
                           !g->lat_vertex || !g->lon_vertex))
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon: NULL mesh array");
    if (!g->lat_corner || !g->lon_corner)
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon: NULL grid corners");
    *G = {g->n_cells, g->n_vertices, g->n_lat, g->n_lon, g->max_edges,
          g->lat_slack, g->vertices_on_cell, g->n_edges_on_cell,
          g->lat_vertex, g->lon_vertex, g->lat_corner, g->lon_corner};
    return REMAP_OK;
}

// whether SW, SE, NE, NW runs clockwise (exactly one axis descends): read
// from the corner arrays, which the caller passes on the device
int axis_swap(const Geom &G, hipStream_t stream, bool *swap)
{
    double ends[4];
    REMAP_HIP_CHECK(hipMemcpyAsync(&ends[0], G.lat_c, 8, hipMemcpyDeviceToHost,
                                   stream));
    REMAP_HIP_CHECK(hipMemcpyAsync(&ends[1], G.lat_c + G.n_lat, 8,
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipMemcpyAsync(&ends[2], G.lon_c, 8, hipMemcpyDeviceToHost,
                                   stream));
    REMAP_HIP_CHECK(hipMemcpyAsync(&ends[3], G.lon_c + G.n_lon, 8,
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    *swap = (ends[1] < ends[0]) != (ends[3] < ends[2]);
    return REMAP_OK;
}

uint32_t blocks(int64_t n, int per) { return static_cast<uint32_t>((n + per - 1) / per); }

int overlap_sizes(const remap_overlap_geom *geom, int64_t *counter,
                  int64_t *n_pairs_out, size_t *bytes_out, hipStream_t stream)
{
    Geom G;
    int rc = check_geom(geom, &G);
    if (rc != REMAP_OK)
        return rc;
    if (!counter || !n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon_sizes: NULL output");
    REMAP_HIP_CHECK(hipMemsetAsync(counter, 0, 2 * sizeof(int64_t), stream));
    if (G.n_cells > 0) {
        hipLaunchKernelGGL(cell_prep, dim3(blocks(G.n_cells, kPrepBlock)),
                           dim3(kPrepBlock), 0, stream, G, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr,
                           reinterpret_cast<unsigned long long *>(counter),
                           reinterpret_cast<int32_t *>(counter + 1));
        REMAP_HIP_CHECK(hipGetLastError());
    }
    int64_t got[2];
    REMAP_HIP_CHECK(hipMemcpyAsync(got, counter, sizeof(got),
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    if (int err = static_cast<int>(got[1] & 0xffffffff))
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_latlon: %s%s",
                    (err & REMAP_OVERLAP_ERR_EDGES)
                        ? "a cell has more edges than this build serves "
                          "(REMAP_OVERLAP_MAX_EDGES) "
                        : "",
                    (err & REMAP_OVERLAP_ERR_VERTEX)
                        ? "a cell has fewer than 3 distinct vertices or a "
                          "vertex index out of range"
                        : "");
    Layout lay;
    rc = make_layout(G.n_cells, G.max_edges, got[0], &lay);
    if (rc != REMAP_OK)
        return rc;
    *n_pairs_out = got[0];
    *bytes_out = lay.total;
    return REMAP_OK;
}

int overlap(const remap_overlap_geom *geom, int32_t dst_is_mesh,
            int64_t n_pairs, void *workspace, size_t workspace_bytes,
            int32_t *dst_out, int32_t *src_out, double *area_out,
            double *frac_b_out, double *mesh_area_out, double *grid_area_out,
            int64_t *n_entries_out, hipStream_t stream)
{
    Geom G;
    int rc = check_geom(geom, &G);
    if (rc != REMAP_OK)
        return rc;
    if (n_pairs < 0 || n_pairs >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_latlon: %lld candidate pairs",
                    static_cast<long long>(n_pairs));
    if (!frac_b_out || !mesh_area_out || !grid_area_out || !n_entries_out ||
        (n_pairs > 0 && (!dst_out || !src_out || !area_out)))
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon: NULL output");
    Layout lay;
    rc = make_layout(G.n_cells, G.max_edges, n_pairs, &lay);
    if (rc != REMAP_OK)
        return rc;
    if (!workspace || workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "remap_overlap_latlon: workspace of %zu bytes, need %zu",
                    workspace_bytes, lay.total);
    bool swap = false;
    rc = axis_swap(G, stream, &swap);
    if (rc != REMAP_OK)
        return rc;
    char *ws = static_cast<char *>(workspace);
    double *cell_xyz = reinterpret_cast<double *>(ws + lay.xyz);
    int32_t *cell_nv = reinterpret_cast<int32_t *>(ws + lay.nv);
    double *centre = reinterpret_cast<double *>(ws + lay.centre);
    Box *boxes = reinterpret_cast<Box *>(ws + lay.boxes);
    uint64_t *counts = reinterpret_cast<uint64_t *>(ws + lay.counts);
    uint64_t *offs = reinterpret_cast<uint64_t *>(ws + lay.offs);
    uint64_t *keys = reinterpret_cast<uint64_t *>(ws + lay.keys);
    double *parea = reinterpret_cast<double *>(ws + lay.parea);
    uint32_t *head = reinterpret_cast<uint32_t *>(ws + lay.head);
    uint32_t *slot = reinterpret_cast<uint32_t *>(ws + lay.slot);
    uint64_t *keys_c = reinterpret_cast<uint64_t *>(ws + lay.keys_c);
    double *area_c = reinterpret_cast<double *>(ws + lay.area_c);
    uint64_t *keys_s = reinterpret_cast<uint64_t *>(ws + lay.keys_s);
    int64_t *n_kept = reinterpret_cast<int64_t *>(ws + lay.n_kept);
    int32_t *status = reinterpret_cast<int32_t *>(ws + lay.status);
    void *temp = ws + lay.temp;
    const int64_t n_grid = G.n_lat * G.n_lon;
    const int64_t n_dst = dst_is_mesh ? G.n_cells : n_grid;
    double *dst_area = dst_is_mesh ? mesh_area_out : grid_area_out;

    REMAP_HIP_CHECK(hipMemsetAsync(n_kept, 0, 16, stream));
    hipLaunchKernelGGL(grid_area, dim3(blocks(n_grid, kBlock)), dim3(kBlock),
                       0, stream, G, swap, grid_area_out);
    REMAP_HIP_CHECK(hipGetLastError());
    if (G.n_cells > 0) {
        hipLaunchKernelGGL(cell_prep, dim3(blocks(G.n_cells, kPrepBlock)),
                           dim3(kPrepBlock), 0, stream, G, cell_xyz, cell_nv,
                           centre, mesh_area_out, boxes, counts, nullptr,
                           status);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            temp, tb, static_cast<const uint64_t *>(counts), offs,
            uint64_t(0), static_cast<size_t>(G.n_cells),
            rocprim::plus<uint64_t>(), stream)));
        hipLaunchKernelGGL(fill_pairs, dim3(blocks(G.n_cells, kBlock)),
                           dim3(kBlock), 0, stream, G, boxes, offs, n_pairs,
                           keys, status);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (n_pairs > 0) {
        hipLaunchKernelGGL(clip_pairs, dim3(blocks(n_pairs, kClipBlock)),
                           dim3(kClipBlock), 0, stream, G, swap, n_pairs, keys,
                           cell_xyz, cell_nv, centre, parea, status);
        REMAP_HIP_CHECK(hipGetLastError());
        const uint32_t nb = blocks(n_pairs, kBlock);
        hipLaunchKernelGGL(flag_kept, dim3(nb), dim3(kBlock), 0, stream,
                           n_pairs, G.n_cells, n_grid, dst_is_mesh != 0, keys,
                           parea, mesh_area_out, grid_area_out, head);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            temp, tb, static_cast<const uint32_t *>(head), slot, 0u,
            static_cast<size_t>(n_pairs), rocprim::plus<uint32_t>(), stream)));
        hipLaunchKernelGGL(scatter_kept, dim3(nb), dim3(kBlock), 0, stream,
                           n_pairs, dst_is_mesh != 0, keys, parea, head, slot,
                           keys_c, area_c, n_kept);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    // the one read-back: how many entries to sort
    int64_t back[2];
    REMAP_HIP_CHECK(hipMemcpyAsync(back, n_kept, 16, hipMemcpyDeviceToHost,
                                   stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    const int64_t n_entries = back[0];
    const int err = static_cast<int>(back[1] & 0xffffffff);
    if (err)
        return fail(REMAP_ERR_UNSUPPORTED, "remap_overlap_latlon: %s%s%s%s%s",
                    (err & REMAP_OVERLAP_ERR_EDGES)
                        ? "a cell has more edges than this build serves "
                          "(REMAP_OVERLAP_MAX_EDGES); "
                        : "",
                    (err & REMAP_OVERLAP_ERR_VERTEX)
                        ? "a cell has fewer than 3 distinct vertices or a "
                          "vertex index out of range; "
                        : "",
                    (err & REMAP_OVERLAP_ERR_HEMISPHERE)
                        ? "a candidate pair has a vertex outside the "
                          "tangent hemisphere of the mesh cell's centre; "
                        : "",
                    (err & kErrClip)
                        ? "a clipped polygon outgrew its REMAP_OVERLAP_MAX_EDGES "
                          "+ 4 vertices (mesh vertices on a lat-lon edge); "
                        : "",
                    (err & REMAP_OVERLAP_ERR_CAPACITY)
                        ? "more candidate pairs than n_pairs (a stale "
                          "remap_overlap_latlon_sizes)"
                        : "");
    *n_entries_out = n_entries;
    if (n_entries > 0) {
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
            temp, tb, static_cast<const uint64_t *>(keys_c), keys_s,
            static_cast<const double *>(area_c), area_out,
            static_cast<size_t>(n_entries), 0u, 64u, stream)));
        hipLaunchKernelGGL(split_keys, dim3(blocks(n_entries, kBlock)),
                           dim3(kBlock), 0, stream, n_kept, n_pairs, keys_s,
                           dst_out, src_out);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (n_dst > 0) {
        hipLaunchKernelGGL(dst_sums, dim3(blocks(n_dst, kBlock)), dim3(kBlock),
                           0, stream, n_dst, n_kept, dst_out, area_out,
                           dst_area, frac_b_out);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    return REMAP_OK;
}

}  // namespace
}  // namespace remap

extern "C" {

int remap_overlap_latlon_sizes(const remap_overlap_geom *geom,
                               int64_t *counter, int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream)
{
    return remap::overlap_sizes(geom, counter, n_pairs_out,
                                workspace_bytes_out,
                                static_cast<hipStream_t>(stream));
}

int remap_overlap_latlon(const remap_overlap_geom *geom, int32_t dst_is_mesh,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *mesh_area_out,
                         double *grid_area_out, int64_t *n_entries_out,
                         void *stream)
{
    return remap::overlap(geom, dst_is_mesh, n_pairs, workspace,
                          workspace_bytes, dst_out, src_out, area_out,
                          frac_b_out, mesh_area_out, grid_area_out,
                          n_entries_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
