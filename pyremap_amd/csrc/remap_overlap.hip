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
//
// Between two MPAS meshes (remap_overlap_meshes, further down) the same
// cell preparation runs against a raster of lat-lon buckets, candidate pairs
// come from the buckets the cells' boxes share, and clip_pairs_poly clips a
// cell of one mesh by a (convex) cell of the other.
//
// Cells that come in convex pieces (remap_overlap_pieces, behind the mesh
// path: the concave cells of an MPAS vertex mesh as triangles) go through the
// mesh path piece by piece up to clip_pairs_poly; the piece pairs are then
// re-keyed to their cells, sorted, and merge_runs adds every run of equal
// keys up in a fixed order before the sliver rule is applied to the sum.
//
// With a structured 2-D grid given by its corner arrays on one side or both
// (remap_overlap_grids, at the end) the grid's cells are prepared straight
// from the corners, candidates come from a pyramid of bounding caps over
// the grid's own index space, and clip_pairs_poly and everything behind it
// are the mesh path's.  Host read-backs: one in remap_overlap_latlon, two in
// remap_overlap_meshes, one in remap_overlap_grids (the entry count with
// every error bit, before the sort), remap_overlap_meshes' two and up to two
// more in remap_overlap_pieces (the parents' check, the entry count behind
// the merge); each _sizes call reads its count back.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "remap_common.h"
#include "remap_sphere.h"

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

constexpr size_t kAlign = 256;
size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

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

// A ring whose consecutive duplicates are dropped already: the closing
// duplicate dropped too, turned counter-clockwise, its area (the fan from
// vertex 0) and its centre.  Returns the error bits; *nv is 0 on an error.
__device__ int finish_ring(Ring xyz, int *nv_io, V3 *centre, double *area)
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
    if (const int err = finish_ring(xyz, &nv, centre, area))
        return err;
    *nv_out = nv;
    const V3 cc = *centre;

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

// kBucketMajor: the keys grid cell << 32 | cell instead (a mesh's bucket
// lists, remap_overlap_meshes)
template <bool kBucketMajor>
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
    const uint64_t cc = static_cast<uint64_t>(c);
    const uint64_t hi = cc << 32;
    for (int32_t r = b.r0; r <= b.r1; ++r) {
        const uint64_t base = static_cast<uint64_t>(r) * G.n_lon;
        for (int32_t i = b.a0; i <= b.a1; ++i)
            keys[o++] = kBucketMajor ? (base + i) << 32 | cc : hi | (base + i);
        for (int32_t i = b.b0; i <= b.b1; ++i)
            keys[o++] = kBucketMajor ? (base + i) << 32 | cc : hi | (base + i);
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
        hipLaunchKernelGGL(fill_pairs<false>, dim3(blocks(G.n_cells, kBlock)),
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


// ---------------------------------------------------------------------------
// two MPAS meshes (remap_overlap_meshes): the cells of mesh a (subject)
// clipped by those of mesh b (clipper), candidates through a global uniform
// lat-lon raster of buckets sized to b
//   bucket_edges   the raster's corners: n_lat rows of pi / n_lat, 2 n_lat
//                  columns from 0 to 2 pi
//   cell_prep      both meshes against the raster (lat_slack 0: buckets are
//                  true lat-lon rectangles); boxes as bucket ranges
//   cell_shape     one lane per cell: the angular radius of its polygon about
//                  its centre; b's cells checked convex
//   -- read-back: the bucket key counts and the cells' error bits --
//   fill_pairs     b: bucket << 32 | b, radix sorted; bucket_starts: where
//                  each bucket's cells begin; a: a << 32 | bucket
//   pair_counts / scan / expand_pairs  (a, bucket) -> (a, b) for every b of
//                  the bucket; radix sort; unique (a pair is found once per
//                  bucket the two boxes share)
//   clip_pairs_poly  one lane per unique pair: a's polygon by b's edges in
//                  the gnomonic plane of a's centre
//   flag / scan / scatter, radix sort, dst_sums as above, a in the "mesh"
//   and b in the "grid" half of the keys (dst_is_b only re-keys)
// ---------------------------------------------------------------------------

// one clip by an edge of a convex clipper adds at most one vertex
constexpr int kMaxOutPoly = 2 * kMaxEdges;
// a clipper vertex may lie this far (x the cell's longest edge) on the wrong
// side of another edge's great circle: collinear vertices, rounded
constexpr double kConvexTol = 1e-9;
// bucket rows of the raster: sqrt(n_b / 2), within these bounds
constexpr int64_t kMinBucketRows = 2;
constexpr int64_t kMaxBucketRows = 8192;
constexpr uint64_t kLow = 0xffffffffull;

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

__global__ __launch_bounds__(kBlock) void bucket_edges(
    int64_t n_lat, int64_t n_lon, double *__restrict__ lat_c,
    double *__restrict__ lon_c)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k <= n_lat)
        lat_c[k] = k == n_lat ? kHalfPi
                              : -kHalfPi + kPi * static_cast<double>(k) /
                                               static_cast<double>(n_lat);
    if (k <= n_lon)
        lon_c[k] = k == n_lon ? kTwoPi
                              : kTwoPi * static_cast<double>(k) /
                                    static_cast<double>(n_lon);
}

// the count-only pass of remap_overlap_meshes_sizes: mesh b adds its cells
// to the buckets their boxes cover (hist), mesh a sums hist over its boxes
__global__ __launch_bounds__(kPrepBlock) void mesh_count(
    Geom G, bool is_b, uint32_t *__restrict__ hist,
    unsigned long long *__restrict__ n_keys,
    unsigned long long *__restrict__ n_cand, int32_t *__restrict__ status)
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
    if (err) {
        atomicOr(status, err);
        return;
    }
    if (is_b && !convex_cell(xyz, nv))
        atomicOr(status, REMAP_OVERLAP_ERR_CONVEX);
    const int64_t cnt = box_count(b);
    if (cnt)
        atomicAdd(n_keys, static_cast<unsigned long long>(cnt));
    unsigned long long s = 0;
    for (int32_t r = b.r0; r <= b.r1 && cnt; ++r) {
        const int64_t base = static_cast<int64_t>(r) * G.n_lon;
        for (int half = 0; half < 2; ++half) {
            const int32_t i0 = half ? b.b0 : b.a0, i1 = half ? b.b1 : b.a1;
            for (int32_t i = i0; i <= i1; ++i) {
                if (is_b)
                    atomicAdd(&hist[base + i], 1u);
                else
                    s += hist[base + i];
            }
        }
    }
    if (s)
        atomicAdd(n_cand, s);
}

// one lane per prepared cell: the radius of the cap about its centre that
// holds its polygon; with `convex`, the convexity of a clipper cell
__global__ __launch_bounds__(kBlock) void cell_shape(
    int64_t n_cells, int32_t max_edges, bool convex,
    const double *__restrict__ cell_xyz, const int32_t *__restrict__ cell_nv,
    const double *__restrict__ cell_centre, double *__restrict__ radius,
    int32_t *__restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_cells)
        return;
    const int nv = cell_nv[c];
    const CellRing v = {cell_xyz + c * max_edges * 3};
    const V3 cc = {cell_centre[c * 3], cell_centre[c * 3 + 1],
                   cell_centre[c * 3 + 2]};
    double r = 0.0;
    for (int k = 0; k < nv; ++k) {
        const V3 q = v[k];
        const V3 x = cross(cc, q);
        r = fmax(r, atan2(sqrt(dot(x, x)), dot(cc, q)));
    }
    radius[c] = r;
    if (convex && nv >= 3 && !convex_cell(v, nv))
        atomicOr(status, REMAP_OVERLAP_ERR_CONVEX);
}

__global__ void scan_total(int64_t n, const uint64_t *__restrict__ counts,
                           const uint64_t *__restrict__ offs,
                           int64_t *__restrict__ out)
{
    if (threadIdx.x == 0 && n > 0)
        *out = static_cast<int64_t>(offs[n - 1] + counts[n - 1]);
}

// where the cells of bucket k begin in the sorted keys bucket << 32 | b
// (k = n_buckets: the end)
__global__ __launch_bounds__(kBlock) void bucket_starts(
    int64_t n_buckets, int64_t n_keys, const uint64_t *__restrict__ keys,
    uint32_t *__restrict__ start)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k > n_buckets)
        return;
    const uint64_t want = static_cast<uint64_t>(k) << 32;
    int64_t lo = 0, hi = n_keys;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    start[k] = static_cast<uint32_t>(lo);
}

// the cells of b in the bucket of every key a << 32 | bucket
__global__ __launch_bounds__(kBlock) void pair_counts(
    int64_t n_keys, int64_t n_buckets, const uint64_t *__restrict__ keys,
    const uint32_t *__restrict__ start, uint64_t *__restrict__ counts)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_keys)
        return;
    const uint64_t k = keys[p] & kLow;
    counts[p] = k < static_cast<uint64_t>(n_buckets) ? start[k + 1] - start[k]
                                                     : 0;
}

__global__ __launch_bounds__(kBlock) void expand_pairs(
    int64_t n_keys, int64_t n_buckets, const uint64_t *__restrict__ keys,
    const uint64_t *__restrict__ counts, const uint64_t *__restrict__ offs,
    const uint32_t *__restrict__ start, const uint64_t *__restrict__ bkeys,
    int64_t capacity, uint64_t *__restrict__ pairs,
    int32_t *__restrict__ status)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_keys)
        return;
    const uint64_t key = keys[p];
    const uint64_t k = key & kLow;
    const int64_t cnt = static_cast<int64_t>(counts[p]);
    int64_t o = static_cast<int64_t>(offs[p]);
    if (o + cnt > capacity) {
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
        return;
    }
    if (p == n_keys - 1 && o + cnt != capacity)
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
    if (!cnt || k >= static_cast<uint64_t>(n_buckets))
        return;
    const uint64_t hi = key & ~kLow;
    for (uint32_t i = start[k]; i < start[k + 1]; ++i)
        pairs[o++] = hi | (bkeys[i] & kLow);
}

// one lane per unique candidate pair a << 32 | b: the area of a's polygon
// clipped by b's (convex) in the gnomonic plane of a's centre; lanes past
// the unique count (their keys ~0) write 0
__global__ __launch_bounds__(kClipBlock) void clip_pairs_poly(
    int64_t n_a, int32_t max_edges_a, int64_t n_b, int32_t max_edges_b,
    int64_t n_pairs, const uint64_t *__restrict__ n_unique,
    const uint64_t *__restrict__ keys, const double *__restrict__ xyz_a,
    const int32_t *__restrict__ nv_a, const double *__restrict__ centre_a,
    const double *__restrict__ radius_a, const double *__restrict__ xyz_b,
    const int32_t *__restrict__ nv_b, const double *__restrict__ centre_b,
    const double *__restrict__ radius_b, double *__restrict__ area,
    int32_t *__restrict__ status)
{
    // the polygon being clipped, ping-pong: [buffer][vertex][lane]
    __shared__ double px[2][kMaxOutPoly][kClipBlock];
    __shared__ double py[2][kMaxOutPoly][kClipBlock];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kClipBlock + lane;
    if (p >= n_pairs)
        return;
    if (static_cast<uint64_t>(p) >= *n_unique) {
        area[p] = 0.0;
        return;
    }
    const uint64_t key = keys[p];
    const int64_t a = static_cast<int64_t>(key >> 32);
    const int64_t b = static_cast<int64_t>(key & kLow);
    if (a >= n_a || b >= n_b) {
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
        area[p] = 0.0;
        return;
    }
    const V3 ca = {centre_a[a * 3], centre_a[a * 3 + 1], centre_a[a * 3 + 2]};
    const V3 cb = {centre_b[b * 3], centre_b[b * 3 + 1], centre_b[b * 3 + 2]};
    // the caps that hold the two polygons are apart: no overlap (and no
    // projection of cells too far apart for it)
    const V3 xc = cross(ca, cb);
    if (atan2(sqrt(dot(xc, xc)), dot(ca, cb)) >
        radius_a[a] + radius_b[b] + kBoxEps) {
        area[p] = 0.0;
        return;
    }
    // tangent-plane basis at a's centre
    const V3 ref = fabs(ca.z) < 0.9 ? V3{0.0, 0.0, 1.0} : V3{1.0, 0.0, 0.0};
    const V3 e1 = normalized(cross(ref, ca));
    const V3 e2 = cross(ca, e1);
    const int na = nv_a[a], nb = nv_b[b];
    const double *vb = xyz_b + b * max_edges_b * 3;
    bool bad = false;
    for (int k = 0; k < kMaxEdges; ++k) {
        if (k < na) {
            const double *v = xyz_a + (a * max_edges_a + k) * 3;
            const V3 q = {v[0], v[1], v[2]};
            const double t = dot(q, ca);
            bad |= !(t >= kMinCos);
            px[0][k][lane] = dot(q, e1) / t;
            py[0][k][lane] = dot(q, e2) / t;
        }
    }
    for (int k = 0; k < nb; ++k) {
        const V3 q = {vb[3 * k], vb[3 * k + 1], vb[3 * k + 2]};
        bad |= !(dot(q, ca) >= kMinCos);
    }
    if (bad) {
        atomicOr(status, REMAP_OVERLAP_ERR_HEMISPHERE);
        area[p] = 0.0;
        return;
    }
    auto project = [&](int k, double *x, double *y) {
        const V3 q = {vb[3 * k], vb[3 * k + 1], vb[3 * k + 2]};
        const double t = dot(q, ca);
        *x = dot(q, e1) / t;
        *y = dot(q, e2) / t;
    };
    double fx, fy;
    project(0, &fx, &fy);
    double ax = fx, ay = fy;
    int n = na, cur = 0;
    for (int e = 0; e < nb && n > 0; ++e) {
        double bx = fx, by = fy;
        if (e + 1 < nb)
            project(e + 1, &bx, &by);
        const double dx = bx - ax, dy = by - ay;
        if (dx != 0.0 || dy != 0.0) {
            const int nxt = cur ^ 1;
            int m = 0;
            double sx = px[cur][n - 1][lane], sy = py[cur][n - 1][lane];
            double ss = dx * (sy - ay) - dy * (sx - ax);
            for (int k = 0; k < n; ++k) {
                const double ex = px[cur][k][lane], ey = py[cur][k][lane];
                const double se = dx * (ey - ay) - dy * (ex - ax);
                if ((se >= 0.0) != (ss >= 0.0)) {
                    if (m < kMaxOutPoly) {
                        const double t = ss / (ss - se);
                        px[nxt][m][lane] = sx + t * (ex - sx);
                        py[nxt][m][lane] = sy + t * (ey - sy);
                    }
                    ++m;
                }
                if (se >= 0.0) {
                    if (m < kMaxOutPoly) {
                        px[nxt][m][lane] = ex;
                        py[nxt][m][lane] = ey;
                    }
                    ++m;
                }
                sx = ex;
                sy = ey;
                ss = se;
            }
            if (m > kMaxOutPoly) {
                atomicOr(status, kErrClip);
                area[p] = 0.0;
                return;
            }
            n = m;
            cur = nxt;
        }
        ax = bx;
        ay = by;
    }
    // the fan of Van Oosterom-Strackee triangles straight from the plane:
    // the unit vector of (x, y) is (c + x e1 + y e2) / r, r = sqrt(1 + x^2 +
    // y^2), so det(a, b, c) and the dot products come from the small plane
    // coordinates instead of differences of lifted unit vectors
    double s = 0.0;
    if (n >= 3) {
        const double x0 = px[cur][0][lane], y0 = py[cur][0][lane];
        const double r0 = sqrt(1.0 + x0 * x0 + y0 * y0);
        double x1 = px[cur][1][lane], y1 = py[cur][1][lane];
        double r1 = sqrt(1.0 + x1 * x1 + y1 * y1);
        for (int k = 2; k < n; ++k) {
            const double x2 = px[cur][k][lane], y2 = py[cur][k][lane];
            const double r2 = sqrt(1.0 + x2 * x2 + y2 * y2);
            const double num = ((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)) /
                               (r0 * r1 * r2);
            const double den = 1.0 + (1.0 + x0 * x1 + y0 * y1) / (r0 * r1) +
                               (1.0 + x1 * x2 + y1 * y2) / (r1 * r2) +
                               (1.0 + x2 * x0 + y2 * y0) / (r2 * r0);
            s += 2.0 * atan2(num, den);
            x1 = x2;
            y1 = y2;
            r1 = r2;
        }
    }
    area[p] = s > 0.0 ? s : 0.0;
}

int check_mesh(const remap_overlap_mesh *m, const char *name, Geom *G)
{
    if (!m)
        return fail(REMAP_ERR_ARG, "remap_overlap_meshes: NULL mesh %s",
                    name);
    if (m->n_cells < 0 || m->n_vertices < 0 || m->max_edges < 3)
        return fail(REMAP_ERR_ARG, "remap_overlap_meshes: bad sizes of mesh %s",
                    name);
    if (m->max_edges > kMaxEdges)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_meshes: maxEdges %d of mesh %s exceeds the "
                    "%d this build serves (REMAP_OVERLAP_MAX_EDGES)",
                    m->max_edges, name, kMaxEdges);
    if (m->n_cells >= (int64_t(1) << 31))
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_meshes: mesh %s beyond 32-bit indices",
                    name);
    if (m->n_cells > 0 && (!m->vertices_on_cell || !m->n_edges_on_cell ||
                           !m->lat_vertex || !m->lon_vertex))
        return fail(REMAP_ERR_ARG, "remap_overlap_meshes: NULL array of mesh %s",
                    name);
    *G = {m->n_cells, m->n_vertices, 0, 0, m->max_edges, 0.0,
          m->vertices_on_cell, m->n_edges_on_cell, m->lat_vertex,
          m->lon_vertex, nullptr, nullptr};
    return REMAP_OK;
}

// the bucket raster of mesh b: about one of its cells per bucket
void bucket_raster(int64_t n_b, Geom *A, Geom *B)
{
    int64_t n_lat = static_cast<int64_t>(sqrt(0.5 * static_cast<double>(n_b)) + 0.5);
    n_lat = n_lat < kMinBucketRows ? kMinBucketRows
                                   : (n_lat > kMaxBucketRows ? kMaxBucketRows : n_lat);
    A->n_lat = B->n_lat = n_lat;
    A->n_lon = B->n_lon = 2 * n_lat;
}

// the error bits of one mesh, or of the pairs (name NULL), as text
void describe(const char *name, int err, char *out, size_t size)
{
    out[0] = '\0';
    if (!err)
        return;
    snprintf(out, size, "%s%s%s%s%s%s%s%s", name ? "mesh " : "",
             name ? name : "", name ? ": " : "",
             (err & REMAP_OVERLAP_ERR_EDGES)
                 ? "a cell has more edges than this build serves "
                   "(REMAP_OVERLAP_MAX_EDGES); "
                 : "",
             (err & REMAP_OVERLAP_ERR_VERTEX)
                 ? "a cell has fewer than 3 distinct vertices or a vertex "
                   "index out of range; "
                 : "",
             (err & REMAP_OVERLAP_ERR_CONVEX)
                 ? "a cell is not convex (mesh b's cells clip); "
                 : "",
             (err & REMAP_OVERLAP_ERR_HEMISPHERE)
                 ? "a candidate pair has a vertex outside the tangent "
                   "hemisphere of the mesh a cell's centre; "
                 : "",
             (err & kErrClip)
                 ? "a clipped polygon outgrew its 2 x REMAP_OVERLAP_MAX_EDGES "
                   "vertices; "
                 : "");
    if (err & REMAP_OVERLAP_ERR_CAPACITY) {
        const size_t n = strlen(out);
        snprintf(out + n, size - n, "the candidate pairs differ from n_pairs "
                                    "(a stale remap_overlap_meshes_sizes); ");
    }
}

int meshes_fail(const char *who, int err_a, int err_b, int err_p)
{
    char text[3][192];
    describe("a", err_a, text[0], sizeof(text[0]));
    describe("b", err_b, text[1], sizeof(text[1]));
    describe(nullptr, err_p, text[2], sizeof(text[2]));
    // (remap_overlap_pieces names the bit as well)
    const bool pieces = strcmp(who, "remap_overlap_meshes") != 0;
    return fail(REMAP_ERR_UNSUPPORTED, "%s: %s%s%s%s", who, text[0], text[1],
                text[2],
                pieces && ((err_a | err_b) & REMAP_OVERLAP_ERR_CONVEX)
                    ? "(REMAP_OVERLAP_ERR_CONVEX)"
                    : "");
}

// one mesh's prepared cells in the workspace
struct SideLayout {
    size_t xyz, nv, centre, radius, boxes, counts, offs;
};

struct MeshLayout {
    // known from the sizes of the meshes
    size_t lat_c, lon_c, start, back, temp0, fixed;
    SideLayout a, b;
    size_t temp0_bytes;
    // known from the bucket key counts (the first read-back)
    size_t bkeys, bkeys_s, akeys, pcnt, poff, cand, cand_s, parea, area_c,
        head, slot, temp, total;
    size_t temp_bytes;
};

// the read-back words: [0] b's keys, [1] a's keys, [2] the error bits of a
// (low half) and b (high half), [3] unique pairs, [4] entries, [5] the
// pairs' error bits
constexpr int kBackWords = 6;

size_t take(size_t *off, size_t bytes)
{
    const size_t at = *off;
    *off += align_up(bytes);
    return at;
}

SideLayout side_layout(const Geom &G, size_t *off)
{
    const size_t c = static_cast<size_t>(G.n_cells > 0 ? G.n_cells : 1);
    SideLayout s;
    s.xyz = take(off, c * G.max_edges * 3 * 8);
    s.nv = take(off, c * 4);
    s.centre = take(off, c * 3 * 8);
    s.radius = take(off, c * 8);
    s.boxes = take(off, c * sizeof(Box));
    s.counts = take(off, c * 8);
    s.offs = take(off, c * 8);
    return s;
}

int mesh_fixed_layout(const Geom &A, const Geom &B, MeshLayout *L)
{
    const size_t nc = static_cast<size_t>(
        (A.n_cells > B.n_cells ? A.n_cells : B.n_cells) > 0
            ? (A.n_cells > B.n_cells ? A.n_cells : B.n_cells)
            : 1);
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, L->temp0_bytes, static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), uint64_t(0), nc,
        rocprim::plus<uint64_t>())));
    const size_t n_buckets = static_cast<size_t>(A.n_lat * A.n_lon);
    size_t off = 0;
    L->lat_c = take(&off, (A.n_lat + 1) * 8);
    L->lon_c = take(&off, (A.n_lon + 1) * 8);
    L->start = take(&off, (n_buckets + 1) * 4);
    L->back = take(&off, kBackWords * 8);
    L->a = side_layout(A, &off);
    L->b = side_layout(B, &off);
    L->temp0 = take(&off, L->temp0_bytes);
    L->fixed = off;
    return REMAP_OK;
}

int mesh_var_layout(int64_t n_akeys, int64_t n_bkeys, int64_t n_pairs,
                    MeshLayout *L)
{
    const size_t na = static_cast<size_t>(n_akeys > 0 ? n_akeys : 1);
    const size_t nb = static_cast<size_t>(n_bkeys > 0 ? n_bkeys : 1);
    const size_t n = static_cast<size_t>(n_pairs > 0 ? n_pairs : 1);
    size_t t[6];
    REMAP_HIP_CHECK((rocprim::radix_sort_keys(
        nullptr, t[0], static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), nb, 0u, 64u)));
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, t[1], static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), uint64_t(0), na,
        rocprim::plus<uint64_t>())));
    REMAP_HIP_CHECK((rocprim::radix_sort_keys(
        nullptr, t[2], static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), n, 0u, 64u)));
    REMAP_HIP_CHECK((rocprim::unique(
        nullptr, t[3], static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
        n)));
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        nullptr, t[4], static_cast<const uint32_t *>(nullptr),
        static_cast<uint32_t *>(nullptr), 0u, n, rocprim::plus<uint32_t>())));
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        nullptr, t[5], static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr), static_cast<const double *>(nullptr),
        static_cast<double *>(nullptr), n, 0u, 64u)));
    L->temp_bytes = 0;
    for (size_t b : t)
        L->temp_bytes = b > L->temp_bytes ? b : L->temp_bytes;
    size_t off = L->fixed;
    L->bkeys = take(&off, nb * 8);
    L->bkeys_s = take(&off, nb * 8);
    L->akeys = take(&off, na * 8);
    L->pcnt = take(&off, na * 8);
    L->poff = take(&off, na * 8);
    // candidates; then the unique pairs; then the sorted entry keys
    L->cand = take(&off, n * 8);
    // sorted candidates; then the kept entries' keys
    L->cand_s = take(&off, n * 8);
    L->parea = take(&off, n * 8);
    L->area_c = take(&off, n * 8);
    L->head = take(&off, n * 4);
    L->slot = take(&off, n * 4);
    L->temp = take(&off, L->temp_bytes);
    L->total = off;
    return REMAP_OK;
}

int meshes_sizes(const char *who, const remap_overlap_mesh *mesh_a,
                 const remap_overlap_mesh *mesh_b, int64_t *counter,
                 int64_t *n_pairs_out, size_t *bytes_out, hipStream_t stream)
{
    Geom A, B;
    int rc = check_mesh(mesh_a, "a", &A);
    if (rc == REMAP_OK)
        rc = check_mesh(mesh_b, "b", &B);
    if (rc != REMAP_OK)
        return rc;
    if (!counter || !n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "%s_sizes: NULL output", who);
    bucket_raster(B.n_cells, &A, &B);
    const int64_t n_buckets = A.n_lat * A.n_lon;
    // the histogram of b's cells over the buckets, and the raster
    const size_t hist_bytes = align_up(n_buckets * 4);
    const size_t bytes = hist_bytes + align_up((A.n_lat + 1) * 8) +
                         align_up((A.n_lon + 1) * 8);
    char *buf = nullptr;
    REMAP_HIP_CHECK(hipMalloc(&buf, bytes));
    uint32_t *hist = reinterpret_cast<uint32_t *>(buf);
    double *lat_c = reinterpret_cast<double *>(buf + hist_bytes);
    double *lon_c = lat_c + align_up((A.n_lat + 1) * 8) / 8;
    A.lat_c = B.lat_c = lat_c;
    A.lon_c = B.lon_c = lon_c;
    int64_t got[4];
    hipError_t err = hipMemsetAsync(counter, 0, 4 * sizeof(int64_t), stream);
    if (err == hipSuccess)
        err = hipMemsetAsync(hist, 0, n_buckets * 4, stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(bucket_edges, dim3(blocks(A.n_lon + 1, kBlock)),
                           dim3(kBlock), 0, stream, A.n_lat, A.n_lon, lat_c,
                           lon_c);
        unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counter);
        int32_t *status = reinterpret_cast<int32_t *>(counter + 3);
        if (B.n_cells > 0)
            hipLaunchKernelGGL(mesh_count, dim3(blocks(B.n_cells, kPrepBlock)),
                               dim3(kPrepBlock), 0, stream, B, true, hist,
                               cnt + 2, cnt, status + 1);
        if (A.n_cells > 0)
            hipLaunchKernelGGL(mesh_count, dim3(blocks(A.n_cells, kPrepBlock)),
                               dim3(kPrepBlock), 0, stream, A, false, hist,
                               cnt + 1, cnt, status);
        err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(got, counter, sizeof(got), hipMemcpyDeviceToHost,
                             stream);
    if (err == hipSuccess)
        err = hipStreamSynchronize(stream);
    const hipError_t freed = hipFree(buf);
    REMAP_HIP_CHECK(err);
    REMAP_HIP_CHECK(freed);
    const int err_a = static_cast<int>(got[3] & 0xffffffff);
    const int err_b = static_cast<int>((got[3] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return meshes_fail(who, err_a, err_b, 0);
    MeshLayout lay;
    rc = mesh_fixed_layout(A, B, &lay);
    if (rc == REMAP_OK)
        rc = mesh_var_layout(got[1], got[2], got[0], &lay);
    if (rc != REMAP_OK)
        return rc;
    *n_pairs_out = got[0];
    *bytes_out = lay.total;
    return REMAP_OK;
}

struct Side {
    double *xyz, *centre, *radius;
    int32_t *nv;
    Box *boxes;
    uint64_t *counts, *offs;
};

Side side_at(char *ws, const SideLayout &s)
{
    return {reinterpret_cast<double *>(ws + s.xyz),
            reinterpret_cast<double *>(ws + s.centre),
            reinterpret_cast<double *>(ws + s.radius),
            reinterpret_cast<int32_t *>(ws + s.nv),
            reinterpret_cast<Box *>(ws + s.boxes),
            reinterpret_cast<uint64_t *>(ws + s.counts),
            reinterpret_cast<uint64_t *>(ws + s.offs)};
}

// cell_prep, cell_shape, the scan of the bucket counts and its total
int prep_side(const Geom &G, bool clipper, const Side &s, double *area,
              void *temp, size_t temp_bytes, int64_t *total, int32_t *status,
              hipStream_t stream)
{
    if (G.n_cells <= 0)
        return REMAP_OK;
    hipLaunchKernelGGL(cell_prep, dim3(blocks(G.n_cells, kPrepBlock)),
                       dim3(kPrepBlock), 0, stream, G, s.xyz, s.nv, s.centre,
                       area, s.boxes, s.counts, nullptr, status);
    REMAP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cell_shape, dim3(blocks(G.n_cells, kBlock)),
                       dim3(kBlock), 0, stream, G.n_cells, G.max_edges,
                       clipper, s.xyz, s.nv, s.centre, s.radius, status);
    REMAP_HIP_CHECK(hipGetLastError());
    size_t tb = temp_bytes;
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        temp, tb, static_cast<const uint64_t *>(s.counts), s.offs,
        uint64_t(0), static_cast<size_t>(G.n_cells),
        rocprim::plus<uint64_t>(), stream)));
    hipLaunchKernelGGL(scan_total, dim3(1), dim3(kWave), 0, stream, G.n_cells,
                       s.counts, s.offs, total);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

// the buffers of the pairs (n_pairs each) behind clip_pairs_poly
struct PairWork {
    uint64_t *cand, *cand_s;   // the pairs a << 32 | b; the kept entries' keys
    double *parea, *area_c;
    uint32_t *head, *slot;
    uint64_t *n_unique;
    int64_t *n_kept;
    int32_t *status;
    void *temp;
    size_t temp_bytes;
};

// clip_pairs_poly over the pairs in w.cand (the first *w.n_unique of
// n_pairs), then flag / scan / scatter: the kept entries re-keyed
// (dst, src) in w.cand_s / w.area_c, their number in *w.n_kept
int clip_and_keep(const Geom &A, const Side &sa, const Geom &B, const Side &sb,
                  bool dst_is_a, int64_t n_pairs, const PairWork &w,
                  const double *a_area, const double *b_area,
                  hipStream_t stream)
{
    hipLaunchKernelGGL(clip_pairs_poly, dim3(blocks(n_pairs, kClipBlock)),
                       dim3(kClipBlock), 0, stream, A.n_cells, A.max_edges,
                       B.n_cells, B.max_edges, n_pairs, w.n_unique, w.cand,
                       sa.xyz, sa.nv, sa.centre, sa.radius, sb.xyz, sb.nv,
                       sb.centre, sb.radius, w.parea, w.status);
    REMAP_HIP_CHECK(hipGetLastError());
    const uint32_t nb = blocks(n_pairs, kBlock);
    hipLaunchKernelGGL(flag_kept, dim3(nb), dim3(kBlock), 0, stream, n_pairs,
                       A.n_cells, B.n_cells, dst_is_a, w.cand, w.parea, a_area,
                       b_area, w.head);
    REMAP_HIP_CHECK(hipGetLastError());
    size_t tb = w.temp_bytes;
    REMAP_HIP_CHECK((rocprim::exclusive_scan(
        w.temp, tb, static_cast<const uint32_t *>(w.head), w.slot, 0u,
        static_cast<size_t>(n_pairs), rocprim::plus<uint32_t>(), stream)));
    hipLaunchKernelGGL(scatter_kept, dim3(nb), dim3(kBlock), 0, stream,
                       n_pairs, dst_is_a, w.cand, w.parea, w.head, w.slot,
                       w.cand_s, w.area_c, w.n_kept);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

// the kept entries sorted by (dst, src) into the outputs, frac_b of every
// destination cell (w.cand is the sort's key output)
int sort_and_sum(int64_t n_dst, int64_t n_entries, int64_t n_pairs,
                 const PairWork &w, int32_t *dst_out, int32_t *src_out,
                 double *area_out, const double *dst_area, double *frac_b_out,
                 hipStream_t stream)
{
    if (n_entries > 0) {
        size_t tb = w.temp_bytes;
        REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
            w.temp, tb, static_cast<const uint64_t *>(w.cand_s), w.cand,
            static_cast<const double *>(w.area_c), area_out,
            static_cast<size_t>(n_entries), 0u, 64u, stream)));
        hipLaunchKernelGGL(split_keys, dim3(blocks(n_entries, kBlock)),
                           dim3(kBlock), 0, stream, w.n_kept, n_pairs, w.cand,
                           dst_out, src_out);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (n_dst > 0) {
        hipLaunchKernelGGL(dst_sums, dim3(blocks(n_dst, kBlock)), dim3(kBlock),
                           0, stream, n_dst, w.n_kept, dst_out, area_out,
                           dst_area, frac_b_out);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    return REMAP_OK;
}

// what the front of remap_overlap_meshes leaves behind for the clip
struct MeshRun {
    Geom A, B;
    MeshLayout lay;
    Side sa, sb;
    PairWork work;
    int64_t *back;
};

// Everything in front of clip_pairs_poly: both meshes prepared against b's
// bucket raster (their polygons' areas into a_area / b_area), read-back 1,
// the bucket lists and the unique candidate pairs a << 32 | b in R->work.cand.
// `who` names the entry point in messages; ev (6 events or NULL) receives
// the phase marks [0] start, [1] cells prepared, [2] pairs listed.
int mesh_front(const char *who, const remap_overlap_mesh *mesh_a,
               const remap_overlap_mesh *mesh_b, int64_t n_pairs,
               void *workspace, size_t workspace_bytes, double *a_area,
               double *b_area, bool have_outputs, hipStream_t stream,
               hipEvent_t *ev, MeshRun *R)
{
    Geom &A = R->A, &B = R->B;
    int rc = check_mesh(mesh_a, "a", &A);
    if (rc == REMAP_OK)
        rc = check_mesh(mesh_b, "b", &B);
    if (rc != REMAP_OK)
        return rc;
    if (n_pairs < 0 || n_pairs >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED, "%s: %lld candidate pairs", who,
                    static_cast<long long>(n_pairs));
    if (!have_outputs)
        return fail(REMAP_ERR_ARG, "%s: NULL output", who);
    bucket_raster(B.n_cells, &A, &B);
    const int64_t n_buckets = A.n_lat * A.n_lon;
    MeshLayout &lay = R->lay;
    rc = mesh_fixed_layout(A, B, &lay);
    if (rc != REMAP_OK)
        return rc;
    if (!workspace || workspace_bytes < lay.fixed)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need at least %zu", who,
                    workspace_bytes, lay.fixed);
    char *ws = static_cast<char *>(workspace);
    double *lat_c = reinterpret_cast<double *>(ws + lay.lat_c);
    double *lon_c = reinterpret_cast<double *>(ws + lay.lon_c);
    uint32_t *start = reinterpret_cast<uint32_t *>(ws + lay.start);
    int64_t *back = reinterpret_cast<int64_t *>(ws + lay.back);
    int32_t *status_ab = reinterpret_cast<int32_t *>(back + 2);
    int32_t *status = reinterpret_cast<int32_t *>(back + 5);
    R->back = back;
    R->sa = side_at(ws, lay.a);
    R->sb = side_at(ws, lay.b);
    const Side &sa = R->sa, &sb = R->sb;
    A.lat_c = B.lat_c = lat_c;
    A.lon_c = B.lon_c = lon_c;

    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[0], stream));
    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, kBackWords * 8, stream));
    hipLaunchKernelGGL(bucket_edges, dim3(blocks(A.n_lon + 1, kBlock)),
                       dim3(kBlock), 0, stream, A.n_lat, A.n_lon, lat_c,
                       lon_c);
    REMAP_HIP_CHECK(hipGetLastError());
    void *temp0 = ws + lay.temp0;
    rc = prep_side(B, true, sb, b_area, temp0, lay.temp0_bytes, back,
                   status_ab + 1, stream);
    if (rc == REMAP_OK)
        rc = prep_side(A, false, sa, a_area, temp0, lay.temp0_bytes,
                       back + 1, status_ab, stream);
    if (rc != REMAP_OK)
        return rc;
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[1], stream));
    // read-back 1: the bucket keys of both meshes, the cells' error bits
    int64_t got[3];
    REMAP_HIP_CHECK(hipMemcpyAsync(got, back, sizeof(got),
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    const int64_t n_bkeys = got[0], n_akeys = got[1];
    const int err_a = static_cast<int>(got[2] & 0xffffffff);
    const int err_b = static_cast<int>((got[2] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return meshes_fail(who, err_a, err_b, 0);
    if (n_bkeys >= (int64_t(1) << 32) - 1 || n_akeys >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED, "%s: %lld / %lld bucket keys", who,
                    static_cast<long long>(n_akeys),
                    static_cast<long long>(n_bkeys));
    if (n_pairs > 0 && n_akeys == 0)
        return meshes_fail(who, 0, 0, REMAP_OVERLAP_ERR_CAPACITY);
    rc = mesh_var_layout(n_akeys, n_bkeys, n_pairs, &lay);
    if (rc != REMAP_OK)
        return rc;
    if (workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need %zu", who,
                    workspace_bytes, lay.total);
    uint64_t *bkeys = reinterpret_cast<uint64_t *>(ws + lay.bkeys);
    uint64_t *bkeys_s = reinterpret_cast<uint64_t *>(ws + lay.bkeys_s);
    uint64_t *akeys = reinterpret_cast<uint64_t *>(ws + lay.akeys);
    uint64_t *pcnt = reinterpret_cast<uint64_t *>(ws + lay.pcnt);
    uint64_t *poff = reinterpret_cast<uint64_t *>(ws + lay.poff);
    uint64_t *cand = reinterpret_cast<uint64_t *>(ws + lay.cand);
    uint64_t *cand_s = reinterpret_cast<uint64_t *>(ws + lay.cand_s);
    double *parea = reinterpret_cast<double *>(ws + lay.parea);
    double *area_c = reinterpret_cast<double *>(ws + lay.area_c);
    uint32_t *head = reinterpret_cast<uint32_t *>(ws + lay.head);
    uint32_t *slot = reinterpret_cast<uint32_t *>(ws + lay.slot);
    uint64_t *n_unique = reinterpret_cast<uint64_t *>(back + 3);
    int64_t *n_kept = back + 4;
    void *temp = ws + lay.temp;

    // b's bucket lists
    if (n_bkeys > 0) {
        hipLaunchKernelGGL(fill_pairs<true>, dim3(blocks(B.n_cells, kBlock)),
                           dim3(kBlock), 0, stream, B, sb.boxes, sb.offs,
                           n_bkeys, bkeys, status);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::radix_sort_keys(
            temp, tb, static_cast<const uint64_t *>(bkeys), bkeys_s,
            static_cast<size_t>(n_bkeys), 0u, 64u, stream)));
    }
    hipLaunchKernelGGL(bucket_starts, dim3(blocks(n_buckets + 1, kBlock)),
                       dim3(kBlock), 0, stream, n_buckets, n_bkeys, bkeys_s,
                       start);
    REMAP_HIP_CHECK(hipGetLastError());
    // a's (cell, bucket) keys, expanded to (a, b) candidates
    if (n_akeys > 0) {
        const uint32_t nb = blocks(n_akeys, kBlock);
        hipLaunchKernelGGL(fill_pairs<false>, dim3(blocks(A.n_cells, kBlock)),
                           dim3(kBlock), 0, stream, A, sa.boxes, sa.offs,
                           n_akeys, akeys, status);
        REMAP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(pair_counts, dim3(nb), dim3(kBlock), 0, stream,
                           n_akeys, n_buckets, akeys, start, pcnt);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            temp, tb, static_cast<const uint64_t *>(pcnt), poff, uint64_t(0),
            static_cast<size_t>(n_akeys), rocprim::plus<uint64_t>(), stream)));
        hipLaunchKernelGGL(expand_pairs, dim3(nb), dim3(kBlock), 0, stream,
                           n_akeys, n_buckets, akeys, pcnt, poff, start,
                           bkeys_s, n_pairs, cand, status);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    R->work = {cand, cand_s, parea, area_c, head, slot, n_unique,
               n_kept, status, temp, lay.temp_bytes};
    if (n_pairs > 0) {
        size_t tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::radix_sort_keys(
            temp, tb, static_cast<const uint64_t *>(cand), cand_s,
            static_cast<size_t>(n_pairs), 0u, 64u, stream)));
        // the unique pairs into cand, the rest of it ~0 (no pair)
        REMAP_HIP_CHECK(hipMemsetAsync(cand, 0xff, n_pairs * 8, stream));
        tb = lay.temp_bytes;
        REMAP_HIP_CHECK((rocprim::unique(
            temp, tb, static_cast<const uint64_t *>(cand_s), cand, n_unique,
            static_cast<size_t>(n_pairs), rocprim::equal_to<uint64_t>(),
            stream)));
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[2], stream));
    return REMAP_OK;
}

int meshes(const remap_overlap_mesh *mesh_a, const remap_overlap_mesh *mesh_b,
           int32_t dst_is_b, int64_t n_pairs, void *workspace,
           size_t workspace_bytes, int32_t *dst_out, int32_t *src_out,
           double *area_out, double *frac_b_out, double *a_area_out,
           double *b_area_out, int64_t *n_entries_out, hipStream_t stream)
{
    static const char who[] = "remap_overlap_meshes";
    const bool have_outputs =
        frac_b_out && a_area_out && b_area_out && n_entries_out &&
        (n_pairs <= 0 || (dst_out && src_out && area_out));
    MeshRun R;
    int rc = mesh_front(who, mesh_a, mesh_b, n_pairs, workspace,
                        workspace_bytes, a_area_out, b_area_out, have_outputs,
                        stream, nullptr, &R);
    if (rc != REMAP_OK)
        return rc;
    const bool dst_is_a = dst_is_b == 0;
    if (n_pairs > 0) {
        rc = clip_and_keep(R.A, R.sa, R.B, R.sb, dst_is_a, n_pairs, R.work,
                           a_area_out, b_area_out, stream);
        if (rc != REMAP_OK)
            return rc;
    }
    // read-back 2: how many entries to sort, the pairs' error bits
    int64_t kept[2];
    REMAP_HIP_CHECK(hipMemcpyAsync(kept, R.work.n_kept, 16,
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    const int64_t n_entries = kept[0];
    if (const int err = static_cast<int>(kept[1] & 0xffffffff))
        return meshes_fail(who, 0, 0, err);
    *n_entries_out = n_entries;
    return sort_and_sum(dst_is_a ? R.A.n_cells : R.B.n_cells, n_entries,
                        n_pairs, R.work, dst_out, src_out, area_out,
                        dst_is_a ? a_area_out : b_area_out, frac_b_out,
                        stream);
}

// ---------------------------------------------------------------------------
// cells in convex pieces (remap_overlap_pieces): each side's mesh holds the
// PIECES of its cells, parent[k] the cell piece k belongs to (non-decreasing,
// every cell at least one piece; NULL: piece k is cell k).  Everything up to
// clip_pairs_poly is remap_overlap_meshes on the pieces; behind it
//   check_parents  one lane per piece: parent in range, never decreasing,
//                  never skipping a cell
//   parent_areas   one lane per cell: its pieces' areas summed in piece order
//   flag / scan / scatter_parents  the piece pairs with A > 0 re-keyed
//                  (dst cell, src cell), with their own position and their
//                  (dst piece, src piece) key beside them
//   radix sort     (dst cell << 32 | src cell, position)
//   merge_runs     one lane per sorted entry, the first of each run of equal
//                  keys walks it (runs are 1 to 4 long where a few cells are
//                  split in two or three): the areas added in ascending
//                  (dst piece, src piece) order, whatever order the sort left
//                  them in; kept when the SUM > kSliver * area(dst cell)
//   scan / scatter_entries  the kept runs, already sorted and unique
//   -- read-back 3: the entry count --
//   dst_sums as above over the cells
// With identity parents a run is one piece pair, its sum that pair's area
// and the sliver test the one flag_kept makes: the bytes of
// remap_overlap_meshes.
// ---------------------------------------------------------------------------

// (the struct shares its name with the entry point: the tag names it)
using PiecesArg = struct ::remap_overlap_pieces;

// argument error bits of check_parents (beside the REMAP_OVERLAP_ERR_* bits
// of the two sides)
constexpr int kErrParentOrder = 1 << 8;
constexpr int kErrParentEmpty = 1 << 9;

__global__ __launch_bounds__(kBlock) void check_parents(
    int64_t n_pieces, int64_t n_parents, const int32_t *__restrict__ parent,
    int32_t *__restrict__ status)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_pieces)
        return;
    const int64_t p = parent[k];
    const int64_t prev = k > 0 ? parent[k - 1] : -1;
    if (p < 0 || p >= n_parents || p < prev)
        atomicOr(status, kErrParentOrder);
    else if (p > prev + 1 || (k == n_pieces - 1 && p != n_parents - 1))
        atomicOr(status, kErrParentEmpty);
}

// the first piece of cell c (parent is non-decreasing); NULL: c itself
__device__ inline int64_t first_piece(const int32_t *parent, int64_t n_pieces,
                                      int64_t c)
{
    if (!parent)
        return c;
    int64_t lo = 0, hi = n_pieces;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (parent[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void parent_areas(
    int64_t n_pieces, int64_t n_parents, const int32_t *__restrict__ parent,
    const double *__restrict__ piece_area, double *__restrict__ area)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_parents)
        return;
    int64_t k = first_piece(parent, n_pieces, c);
    double s = 0.0;
    if (!parent) {
        s = k < n_pieces ? piece_area[k] : 0.0;
    } else {
        for (; k < n_pieces && parent[k] == c; ++k)
            s += piece_area[k];
    }
    area[c] = s;
}

__global__ __launch_bounds__(kBlock) void flag_positive(
    int64_t n_pairs, int64_t n_a, int64_t n_b,
    const uint64_t *__restrict__ keys, const double *__restrict__ area,
    uint32_t *__restrict__ head)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs)
        return;
    const uint64_t key = keys[p];
    const bool in = (key >> 32) < static_cast<uint64_t>(n_a) &&
                    (key & kLow) < static_cast<uint64_t>(n_b);
    head[p] = in && area[p] > 0.0 ? 1u : 0u;   // (past the unique pairs: ~0)
}

__global__ __launch_bounds__(kBlock) void scatter_parents(
    int64_t n_pairs, bool dst_is_a, const uint64_t *__restrict__ keys,
    const double *__restrict__ area, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ slot, const int32_t *__restrict__ parent_a,
    const int32_t *__restrict__ parent_b, uint64_t *__restrict__ keys_out,
    uint32_t *__restrict__ at_out, double *__restrict__ area_out,
    uint64_t *__restrict__ pieces_out, int64_t *__restrict__ n_kept)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs)
        return;
    if (p == n_pairs - 1)
        *n_kept = static_cast<int64_t>(slot[p]) + head[p];
    if (!head[p])
        return;
    const uint64_t a = keys[p] >> 32, b = keys[p] & kLow;
    const uint64_t ca = parent_a ? static_cast<uint64_t>(parent_a[a]) : a;
    const uint64_t cb = parent_b ? static_cast<uint64_t>(parent_b[b]) : b;
    const uint32_t s = slot[p];
    keys_out[s] = dst_is_a ? ca << 32 | cb : cb << 32 | ca;
    pieces_out[s] = dst_is_a ? a << 32 | b : b << 32 | a;
    at_out[s] = s;
    area_out[s] = area[p];
}

__global__ __launch_bounds__(kBlock) void merge_runs(
    int64_t n, const uint64_t *__restrict__ keys,
    const uint32_t *__restrict__ at, const double *__restrict__ area,
    const uint64_t *__restrict__ pieces, const double *__restrict__ dst_area,
    double *__restrict__ sums, uint32_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t key = keys[i];
    if (i > 0 && keys[i - 1] == key) {
        head[i] = 0u;
        return;
    }
    int64_t end = i + 1;
    while (end < n && keys[end] == key)
        ++end;
    double s = area[at[i]];
    if (end > i + 1) {
        // selection by the piece keys (unique within a run): the order of the
        // additions does not lean on what the sort does with equal keys
        s = 0.0;
        bool any = false;
        uint64_t last = 0;
        for (int64_t step = i; step < end; ++step) {
            uint64_t next = ~uint64_t(0);
            double a = 0.0;
            for (int64_t j = i; j < end; ++j) {
                const uint32_t q = at[j];
                const uint64_t k = pieces[q];
                if ((!any || k > last) && k <= next) {
                    next = k;
                    a = area[q];
                }
            }
            s += a;
            last = next;
            any = true;
        }
    }
    sums[i] = s;
    head[i] = s > kSliver * dst_area[key >> 32] ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void scatter_entries(
    int64_t n, const uint64_t *__restrict__ keys,
    const double *__restrict__ sums, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ slot, int32_t *__restrict__ dst,
    int32_t *__restrict__ src, double *__restrict__ area,
    int64_t *__restrict__ n_entries)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    if (i == n - 1)
        *n_entries = static_cast<int64_t>(slot[i]) + head[i];
    if (!head[i])
        return;
    const uint32_t s = slot[i];
    dst[s] = static_cast<int32_t>(keys[i] >> 32);
    src[s] = static_cast<int32_t>(keys[i] & kLow);
    area[s] = sums[i];
}

// what remap_overlap_pieces keeps in FRONT of the workspace of the mesh
// path: the pieces' own areas and the buffers of the merge
struct PiecesLayout {
    size_t a_area, b_area, at_c, at_s, pieces_c, back, temp, total;
    size_t temp_bytes;
};

int pieces_layout(int64_t n_a, int64_t n_b, int64_t n_pairs, PiecesLayout *L)
{
    const size_t n = static_cast<size_t>(n_pairs > 0 ? n_pairs : 1);
    REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
        nullptr, L->temp_bytes, static_cast<const uint64_t *>(nullptr),
        static_cast<uint64_t *>(nullptr),
        static_cast<const uint32_t *>(nullptr),
        static_cast<uint32_t *>(nullptr), n, 0u, 64u)));
    size_t off = 0;
    L->a_area = take(&off, static_cast<size_t>(n_a > 0 ? n_a : 1) * 8);
    L->b_area = take(&off, static_cast<size_t>(n_b > 0 ? n_b : 1) * 8);
    L->at_c = take(&off, n * 4);
    L->at_s = take(&off, n * 4);
    L->pieces_c = take(&off, n * 8);
    // [0] the entry count, [1] the parents' error bits: a low, b high
    L->back = take(&off, 16);
    L->temp = take(&off, L->temp_bytes);
    L->total = off;
    return REMAP_OK;
}

int check_pieces(const PiecesArg *p, const char *name)
{
    if (!p)
        return fail(REMAP_ERR_ARG, "remap_overlap_pieces: NULL side %s", name);
    if (p->n_parents < 0 || p->n_parents >= (int64_t(1) << 31))
        return fail(REMAP_ERR_ARG,
                    "remap_overlap_pieces: n_parents %lld of side %s (0 to "
                    "2^31 - 1)",
                    static_cast<long long>(p->n_parents), name);
    // every cell has a piece and every piece a cell
    if (p->mesh.n_cells >= 0 &&
        (p->parent ? p->n_parents > p->mesh.n_cells ||
                         (p->n_parents == 0) != (p->mesh.n_cells == 0)
                   : p->n_parents != p->mesh.n_cells))
        return fail(REMAP_ERR_ARG,
                    "remap_overlap_pieces: side %s has %lld cells for %lld "
                    "pieces%s (a cell without a piece, or pieces without a "
                    "cell)",
                    name, static_cast<long long>(p->n_parents),
                    static_cast<long long>(p->mesh.n_cells),
                    p->parent ? "" : " and no parent array");
    return REMAP_OK;
}

int pieces_sizes(const PiecesArg *a, const PiecesArg *b,
                 int64_t *counter, int64_t *n_pairs_out, size_t *bytes_out,
                 hipStream_t stream)
{
    int rc = check_pieces(a, "a");
    if (rc == REMAP_OK)
        rc = check_pieces(b, "b");
    if (rc == REMAP_OK)
        rc = meshes_sizes("remap_overlap_pieces", &a->mesh, &b->mesh, counter,
                          n_pairs_out, bytes_out, stream);
    if (rc != REMAP_OK)
        return rc;
    PiecesLayout X;
    rc = pieces_layout(a->mesh.n_cells, b->mesh.n_cells, *n_pairs_out, &X);
    if (rc != REMAP_OK)
        return rc;
    *bytes_out += X.total;
    return REMAP_OK;
}

// ev (6 events, or NULL) marks the phases: cell preparation, candidate pairs,
// clip (with its compaction), sort, merge (with frac_b)
int pieces(const PiecesArg *pa, const PiecesArg *pb,
           int32_t dst_is_b, int64_t n_pairs, void *workspace,
           size_t workspace_bytes, int32_t *dst_out, int32_t *src_out,
           double *area_out, double *frac_b_out, double *a_area_out,
           double *b_area_out, int64_t *n_entries_out, hipStream_t stream,
           hipEvent_t *ev)
{
    static const char who[] = "remap_overlap_pieces";
    int rc = check_pieces(pa, "a");
    if (rc == REMAP_OK)
        rc = check_pieces(pb, "b");
    if (rc != REMAP_OK)
        return rc;
    const bool have_outputs =
        frac_b_out && a_area_out && b_area_out && n_entries_out &&
        (n_pairs <= 0 || (dst_out && src_out && area_out));
    const int64_t n_a = pa->mesh.n_cells, n_b = pb->mesh.n_cells;
    PiecesLayout X;
    rc = pieces_layout(n_a, n_b, n_pairs, &X);
    if (rc != REMAP_OK)
        return rc;
    if (!workspace || workspace_bytes < X.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need more than %zu", who,
                    workspace_bytes, X.total);
    char *ws = static_cast<char *>(workspace);
    double *piece_area_a = reinterpret_cast<double *>(ws + X.a_area);
    double *piece_area_b = reinterpret_cast<double *>(ws + X.b_area);
    uint32_t *at_c = reinterpret_cast<uint32_t *>(ws + X.at_c);
    uint32_t *at_s = reinterpret_cast<uint32_t *>(ws + X.at_s);
    uint64_t *pieces_c = reinterpret_cast<uint64_t *>(ws + X.pieces_c);
    int64_t *back = reinterpret_cast<int64_t *>(ws + X.back);
    int32_t *status_ab = reinterpret_cast<int32_t *>(back + 1);

    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, 16, stream));
    // the parents first (a read-back of their own, none with identity
    // parents): an argument error comes before any geometry
    if ((pa->parent && n_a > 0) || (pb->parent && n_b > 0)) {
        if (pa->parent && n_a > 0)
            hipLaunchKernelGGL(check_parents, dim3(blocks(n_a, kBlock)),
                               dim3(kBlock), 0, stream, n_a, pa->n_parents,
                               pa->parent, status_ab);
        if (pb->parent && n_b > 0)
            hipLaunchKernelGGL(check_parents, dim3(blocks(n_b, kBlock)),
                               dim3(kBlock), 0, stream, n_b, pb->n_parents,
                               pb->parent, status_ab + 1);
        REMAP_HIP_CHECK(hipGetLastError());
        int32_t bad[2];
        REMAP_HIP_CHECK(hipMemcpyAsync(bad, status_ab, 8,
                                       hipMemcpyDeviceToHost, stream));
        REMAP_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad[0] || bad[1])
            return fail(REMAP_ERR_ARG, "%s: parent of side %s %s", who,
                        bad[0] ? "a" : "b",
                        ((bad[0] ? bad[0] : bad[1]) & kErrParentOrder)
                            ? "decreases or is outside [0, n_parents)"
                            : "skips a cell: a cell without a piece");
    }
    MeshRun R;
    rc = mesh_front(who, &pa->mesh, &pb->mesh, n_pairs, ws + X.total,
                    workspace_bytes - X.total, piece_area_a, piece_area_b,
                    have_outputs, stream, ev, &R);
    if (rc != REMAP_OK)
        return rc;
    if (pa->n_parents > 0)
        hipLaunchKernelGGL(parent_areas, dim3(blocks(pa->n_parents, kBlock)),
                           dim3(kBlock), 0, stream, n_a, pa->n_parents,
                           pa->parent, piece_area_a, a_area_out);
    if (pb->n_parents > 0)
        hipLaunchKernelGGL(parent_areas, dim3(blocks(pb->n_parents, kBlock)),
                           dim3(kBlock), 0, stream, n_b, pb->n_parents,
                           pb->parent, piece_area_b, b_area_out);
    REMAP_HIP_CHECK(hipGetLastError());
    const bool dst_is_a = dst_is_b == 0;
    const PairWork &w = R.work;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(clip_pairs_poly, dim3(blocks(n_pairs, kClipBlock)),
                           dim3(kClipBlock), 0, stream, n_a, R.A.max_edges,
                           n_b, R.B.max_edges, n_pairs, w.n_unique, w.cand,
                           R.sa.xyz, R.sa.nv, R.sa.centre, R.sa.radius,
                           R.sb.xyz, R.sb.nv, R.sb.centre, R.sb.radius,
                           w.parea, w.status);
        REMAP_HIP_CHECK(hipGetLastError());
        const uint32_t nb = blocks(n_pairs, kBlock);
        hipLaunchKernelGGL(flag_positive, dim3(nb), dim3(kBlock), 0, stream,
                           n_pairs, n_a, n_b, w.cand, w.parea, w.head);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = w.temp_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            w.temp, tb, static_cast<const uint32_t *>(w.head), w.slot, 0u,
            static_cast<size_t>(n_pairs), rocprim::plus<uint32_t>(), stream)));
        hipLaunchKernelGGL(scatter_parents, dim3(nb), dim3(kBlock), 0, stream,
                           n_pairs, dst_is_a, w.cand, w.parea, w.head, w.slot,
                           pa->parent, pb->parent, w.cand_s, at_c, w.area_c,
                           pieces_c, w.n_kept);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    // read-back 2: how many piece pairs to sort, the pairs' error bits
    int64_t kept[2];
    REMAP_HIP_CHECK(hipMemcpyAsync(kept, w.n_kept, 16, hipMemcpyDeviceToHost,
                                   stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    const int64_t n_kept = kept[0];
    if (const int err = static_cast<int>(kept[1] & 0xffffffff))
        return meshes_fail(who, 0, 0, err);
    const double *dst_area = dst_is_a ? a_area_out : b_area_out;
    const int64_t n_dst = dst_is_a ? pa->n_parents : pb->n_parents;
    if (n_kept > 0) {
        // (w.cand is the sort's key output, w.parea the runs' sums)
        size_t tb = X.temp_bytes;
        REMAP_HIP_CHECK((rocprim::radix_sort_pairs(
            ws + X.temp, tb, static_cast<const uint64_t *>(w.cand_s), w.cand,
            static_cast<const uint32_t *>(at_c), at_s,
            static_cast<size_t>(n_kept), 0u, 64u, stream)));
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[4], stream));
    int64_t n_entries = 0;
    if (n_kept > 0) {
        const uint32_t nb = blocks(n_kept, kBlock);
        hipLaunchKernelGGL(merge_runs, dim3(nb), dim3(kBlock), 0, stream,
                           n_kept, w.cand, at_s, w.area_c, pieces_c, dst_area,
                           w.parea, w.head);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = w.temp_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            w.temp, tb, static_cast<const uint32_t *>(w.head), w.slot, 0u,
            static_cast<size_t>(n_kept), rocprim::plus<uint32_t>(), stream)));
        hipLaunchKernelGGL(scatter_entries, dim3(nb), dim3(kBlock), 0, stream,
                           n_kept, w.cand, w.parea, w.head, w.slot, dst_out,
                           src_out, area_out, back);
        REMAP_HIP_CHECK(hipGetLastError());
        // read-back 3: the entries the sliver rule left
        REMAP_HIP_CHECK(hipMemcpyAsync(&n_entries, back, 8,
                                       hipMemcpyDeviceToHost, stream));
        REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    }
    *n_entries_out = n_entries;
    if (n_dst > 0) {
        hipLaunchKernelGGL(dst_sums, dim3(blocks(n_dst, kBlock)), dim3(kBlock),
                           0, stream, n_dst, back, dst_out, area_out, dst_area,
                           frac_b_out);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[5], stream));
    return REMAP_OK;
}

int pieces_timed(const PiecesArg *pa,
                 const PiecesArg *pb, int32_t dst_is_b,
                 int64_t n_pairs, void *workspace, size_t workspace_bytes,
                 int32_t *dst_out, int32_t *src_out, double *area_out,
                 double *frac_b_out, double *a_area_out, double *b_area_out,
                 int64_t *n_entries_out, float *phase_ms, hipStream_t stream)
{
    if (!phase_ms)
        return fail(REMAP_ERR_ARG, "remap_overlap_pieces_timed: NULL phase_ms");
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 6 && err == hipSuccess; ++k)
        err = hipEventCreate(&ev[k]);
    int rc = REMAP_OK;
    if (err == hipSuccess) {
        rc = pieces(pa, pb, dst_is_b, n_pairs, workspace, workspace_bytes,
                    dst_out, src_out, area_out, frac_b_out, a_area_out,
                    b_area_out, n_entries_out, stream, ev);
        if (rc == REMAP_OK)
            err = hipEventSynchronize(ev[5]);
        for (int k = 0; k < 5 && rc == REMAP_OK && err == hipSuccess; ++k)
            err = hipEventElapsedTime(&phase_ms[k], ev[k], ev[k + 1]);
    }
    for (int k = 0; k < 6; ++k)
        if (ev[k])
            (void)hipEventDestroy(ev[k]);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(err);
    return REMAP_OK;
}

// ---------------------------------------------------------------------------
// structured 2-D grids (remap_overlap_grids): a side is an MPAS mesh or a
// grid of ny x nx cells given by its (ny + 1) x (nx + 1) corner arrays, cell
// j * nx + i the polygon of the corners (j, i), (j, i + 1), (j + 1, i + 1),
// (j + 1, i).  Side a is the subject, side b the convex clipper, as above;
// what differs is everything in front of clip_pairs_poly:
//   quad_prep      one lane per grid cell: corners -> unit xyz, duplicates
//                  dropped, counter-clockwise, area, centre (finish_ring, as
//                  for mesh cells; no verticesOnCell table); cell_shape as
//                  above (radius; b convex).  A mesh side: prep_side as above
//                  against a raster of one bucket (its boxes are not used)
//   pyramid_level  bounding caps over the grid's cells, level 0 the cells'
//                  own caps, each node above over 2 x 2 nodes below: centre =
//                  normalised sum of the children's centres, radius = max
//                  (angle to child centre + child radius) + kBoxEps; pi =
//                  "always descend" (children that cancel, a global grid)
//   pyramid_walk   one lane per cell of the OTHER side: depth first from the
//                  root with an explicit stack in LDS, a node entered when
//                  the angle between the centres is at most the sum of the
//                  radii (+ kBoxEps, clip_pairs_poly's own test); a level-0
//                  node is a candidate.  Count pass, exclusive scan, fill
//                  pass with the same walk: keys a << 32 | b whichever side
//                  walked, unique, in a fixed order
//   clip_pairs_poly, flag / scan / scatter, radix sort, dst_sums as above
// The pyramid is the grid side's; when both sides are grids it is b's (the
// clipper, the side with fewer cells: the side with more cells has the
// lanes).  Nothing but the corner arrays is needed: a pole inside the grid,
// cells across the longitude seam and cells of the other side outside the
// grid are caps like any other.
// ---------------------------------------------------------------------------

// levels = ceil(log2(max(ny, nx))) + 1; a stack entry packs level (4 bits),
// row and column (14 bits each)
constexpr int kMaxLevels = 15;
constexpr int64_t kMaxGridSide = int64_t(1) << (kMaxLevels - 1);
// a depth-first walk of a 4-ary tree: a pop and up to four pushes per level
constexpr int kMaxStack = 3 * kMaxLevels + 1;
constexpr int kWalkBlock = 64;

struct GridGeom {
    int64_t ny, nx;
    const double *lat, *lon;
};

struct Pyramid {
    int32_t levels;
    int64_t ny, nx;
    const double *centre0, *radius0;   // level 0: the cells' own caps
    double *nodes;                     // levels >= 1: (x, y, z, radius)
    const int64_t *first;              // first[l]: where level l >= 1 begins
};

__host__ __device__ inline int64_t level_dim(int64_t n, int l)
{
    return (n + (int64_t(1) << l) - 1) >> l;
}

int pyramid_levels(int64_t ny, int64_t nx)
{
    const int64_t n = ny > nx ? ny : nx;
    int levels = 1;
    while (level_dim(n, levels - 1) > 1)
        ++levels;
    return levels;
}

// first[l] of every level; returns the number of nodes above level 0
__host__ __device__ inline int64_t pyramid_first(int64_t ny, int64_t nx,
                                                 int levels, int64_t *first)
{
    int64_t n = 0;
    for (int l = 1; l < levels; ++l) {
        if (first)
            first[l] = n;
        n += level_dim(ny, l) * level_dim(nx, l);
    }
    return n;
}

__global__ void pyramid_table(int64_t ny, int64_t nx, int levels,
                              int64_t *__restrict__ first)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        first[0] = 0;
        pyramid_first(ny, nx, levels, first);
    }
}

__device__ inline void node_cap(const Pyramid &P, int l, int64_t j, int64_t i,
                                V3 *c, double *r)
{
    if (l == 0) {
        const int64_t k = j * P.nx + i;
        *c = {P.centre0[3 * k], P.centre0[3 * k + 1], P.centre0[3 * k + 2]};
        *r = P.radius0[k];
    } else {
        const double *n =
            P.nodes + (P.first[l] + j * level_dim(P.nx, l) + i) * 4;
        *c = {n[0], n[1], n[2]};
        *r = n[3];
    }
}

__device__ inline double angle(V3 a, V3 b)
{
    const V3 x = cross(a, b);
    return atan2(sqrt(dot(x, x)), dot(a, b));
}

// one lane per grid cell: its polygon from the corner arrays
__global__ __launch_bounds__(kPrepBlock) void quad_prep(
    GridGeom Q, double *__restrict__ cell_xyz, int32_t *__restrict__ cell_nv,
    double *__restrict__ cell_centre, double *__restrict__ cell_area,
    int32_t *__restrict__ status)
{
    __shared__ double sx[4][kPrepBlock], sy[4][kPrepBlock], sz[4][kPrepBlock];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kPrepBlock + lane;
    if (c >= Q.ny * Q.nx)
        return;
    const Ring xyz = {&sx[0][lane], &sy[0][lane], &sz[0][lane], kPrepBlock};
    const int64_t j = c / Q.nx, i = c - j * Q.nx;
    const int64_t sw = j * (Q.nx + 1) + i;
    int nv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t at = sw + (k == 1 || k == 2 ? 1 : 0) +
                           (k >= 2 ? Q.nx + 1 : 0);
        const V3 p = unit_latlon(Q.lat[at], Q.lon[at]);
        if (nv > 0) {
            const V3 q = xyz[nv - 1];
            if (p.x == q.x && p.y == q.y && p.z == q.z)
                continue;
        }
        xyz.set(nv++, p);
    }
    V3 cc = {0.0, 0.0, 1.0};
    double area;
    const int err = finish_ring(xyz, &nv, &cc, &area);
    if (err)
        atomicOr(status, err);
    for (int k = 0; k < nv; ++k) {
        const V3 v = xyz[k];
        double *o = cell_xyz + (c * 4 + k) * 3;
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
    }
    cell_nv[c] = nv;
    cell_centre[c * 3 + 0] = cc.x;
    cell_centre[c * 3 + 1] = cc.y;
    cell_centre[c * 3 + 2] = cc.z;
    cell_area[c] = area;
}

// one lane per node of level l >= 1, the level below it complete
__global__ __launch_bounds__(kBlock) void pyramid_level(Pyramid P, int l)
{
    const int64_t w = level_dim(P.nx, l), h = level_dim(P.ny, l);
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= w * h)
        return;
    const int64_t J = k / w, I = k - J * w;
    const int64_t ch = level_dim(P.ny, l - 1), cw = level_dim(P.nx, l - 1);
    V3 s = {0.0, 0.0, 0.0};
    bool open = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t j = 2 * J + (q >> 1), i = 2 * I + (q & 1);
        if (j < ch && i < cw) {
            V3 c;
            double r;
            node_cap(P, l - 1, j, i, &c, &r);
            s = {s.x + c.x, s.y + c.y, s.z + c.z};
            open |= !(r < kPi);
        }
    }
    const double len = sqrt(dot(s, s));
    V3 cc = {0.0, 0.0, 1.0};
    double rad = kPi;
    // (children that cancel, or one that is open itself: always descend)
    if (!open && len > 1e-3) {
        cc = {s.x / len, s.y / len, s.z / len};
        rad = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t j = 2 * J + (q >> 1), i = 2 * I + (q & 1);
            if (j < ch && i < cw) {
                V3 c;
                double r;
                node_cap(P, l - 1, j, i, &c, &r);
                rad = fmax(rad, angle(cc, c) + r);
            }
        }
        rad += kBoxEps;
        if (!(rad < kPi))
            rad = kPi;
    }
    double *n = P.nodes + (P.first[l] + k) * 4;
    n[0] = cc.x;
    n[1] = cc.y;
    n[2] = cc.z;
    n[3] = rad;
}

// one lane per cell of the walking side: the grid cells whose caps meet its
// cap.  Count pass: counts[w]; fill pass (kFill): the keys at offs[w]
template <bool kFill>
__global__ __launch_bounds__(kWalkBlock) void pyramid_walk(
    Pyramid P, int64_t n_w, const double *__restrict__ centre_w,
    const double *__restrict__ radius_w, const int32_t *__restrict__ nv_w,
    bool walker_is_a, uint64_t *__restrict__ counts,
    const uint64_t *__restrict__ offs, int64_t capacity,
    uint64_t *__restrict__ keys, int32_t *__restrict__ status)
{
    __shared__ uint32_t stack[kMaxStack][kWalkBlock];
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * kWalkBlock + lane;
    if (w >= n_w)
        return;
    int64_t o = 0, room = 0;
    if (kFill) {
        o = static_cast<int64_t>(offs[w]);
        room = static_cast<int64_t>(counts[w]);
        if (o + room > capacity) {
            atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
            return;
        }
        if (w == n_w - 1 && o + room != capacity)
            atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
    }
    int64_t cnt = 0;
    if (nv_w[w] >= 3) {
        const V3 cw = {centre_w[w * 3], centre_w[w * 3 + 1],
                       centre_w[w * 3 + 2]};
        const double rw = radius_w[w];
        int top = 0;
        stack[top++][lane] = static_cast<uint32_t>(P.levels - 1) << 28;
        while (top > 0) {
            const uint32_t e = stack[--top][lane];
            const int l = static_cast<int>(e >> 28);
            const int64_t j = (e >> 14) & 0x3fffu, i = e & 0x3fffu;
            V3 c;
            double r;
            node_cap(P, l, j, i, &c, &r);
            if (r < kPi && !(angle(cw, c) <= rw + r + kBoxEps))
                continue;
            if (l == 0) {
                if (kFill && cnt < room) {
                    const uint64_t g = static_cast<uint64_t>(j * P.nx + i);
                    const uint64_t me = static_cast<uint64_t>(w);
                    keys[o + cnt] = walker_is_a ? me << 32 | g : g << 32 | me;
                }
                ++cnt;
                continue;
            }
            const int64_t ch = level_dim(P.ny, l - 1);
            const int64_t cwid = level_dim(P.nx, l - 1);
            // pushed in reverse: popped in row-major order
            for (int q = 3; q >= 0; --q) {
                const int64_t jj = 2 * j + (q >> 1), ii = 2 * i + (q & 1);
                if (jj < ch && ii < cwid) {
                    if (top < kMaxStack)
                        stack[top++][lane] =
                            static_cast<uint32_t>(l - 1) << 28 |
                            static_cast<uint32_t>(jj) << 14 |
                            static_cast<uint32_t>(ii);
                    else
                        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
                }
            }
        }
    }
    if (!kFill)
        counts[w] = static_cast<uint64_t>(cnt);
    else if (cnt != room)
        atomicOr(status, REMAP_OVERLAP_ERR_CAPACITY);
}

// one side of remap_overlap_grids, checked: G.n_cells / G.max_edges hold
// for either kind (a grid: ny x nx cells of 4 corners)
struct GridSide {
    bool is_grid;
    Geom G;
    GridGeom Q;
};

int check_side(const remap_overlap_side *s, const char *name, GridSide *out)
{
    if (!s || (s->mesh != nullptr) == (s->grid != nullptr))
        return fail(REMAP_ERR_ARG,
                    "remap_overlap_grids: side %s needs exactly one of mesh "
                    "and grid", name);
    out->is_grid = s->grid != nullptr;
    out->Q = {0, 0, nullptr, nullptr};
    if (!out->is_grid) {
        const int rc = check_mesh(s->mesh, name, &out->G);
        out->G.n_lat = out->G.n_lon = 1;
        return rc;
    }
    const remap_overlap_grid *g = s->grid;
    if (g->ny < 1 || g->nx < 1 || !g->lat_corner || !g->lon_corner)
        return fail(REMAP_ERR_ARG, "remap_overlap_grids: bad grid %s", name);
    if (g->ny > kMaxGridSide || g->nx > kMaxGridSide)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_grids: grid %s of %lld x %lld cells; at "
                    "most %lld a side",
                    name, static_cast<long long>(g->ny),
                    static_cast<long long>(g->nx),
                    static_cast<long long>(kMaxGridSide));
    out->Q = {g->ny, g->nx, g->lat_corner, g->lon_corner};
    out->G = {g->ny * g->nx, 0, 1, 1, 4, 0.0, nullptr, nullptr, nullptr,
              nullptr, nullptr, nullptr};
    return REMAP_OK;
}

// the error bits of one side, or of the pairs (name NULL), as text, the
// bits' names included
void describe_side(const char *name, int err, char *out, size_t size)
{
    out[0] = '\0';
    if (!err)
        return;
    snprintf(out, size, "%s%s%s%s%s%s%s%s%s", name ? "side " : "",
             name ? name : "", name ? ": " : "",
             (err & REMAP_OVERLAP_ERR_EDGES)
                 ? "a cell has more edges than this build serves "
                   "(REMAP_OVERLAP_ERR_EDGES); "
                 : "",
             (err & REMAP_OVERLAP_ERR_VERTEX)
                 ? "a cell has fewer than 3 distinct corners or a vertex "
                   "index out of range (REMAP_OVERLAP_ERR_VERTEX); "
                 : "",
             (err & REMAP_OVERLAP_ERR_CONVEX)
                 ? "a cell is not convex and side b's cells clip "
                   "(REMAP_OVERLAP_ERR_CONVEX); "
                 : "",
             (err & REMAP_OVERLAP_ERR_HEMISPHERE)
                 ? "a candidate pair has a vertex outside the tangent "
                   "hemisphere of the side a cell's centre "
                   "(REMAP_OVERLAP_ERR_HEMISPHERE); "
                 : "",
             (err & kErrClip)
                 ? "a clipped polygon outgrew its 2 x REMAP_OVERLAP_MAX_EDGES "
                   "vertices; "
                 : "",
             (err & REMAP_OVERLAP_ERR_CAPACITY)
                 ? "the candidate pairs differ from n_pairs, a stale "
                   "remap_overlap_grids_sizes (REMAP_OVERLAP_ERR_CAPACITY); "
                 : "");
}

int grids_fail(int err_a, int err_b, int err_p)
{
    char text[3][256];
    describe_side("a", err_a, text[0], sizeof(text[0]));
    describe_side("b", err_b, text[1], sizeof(text[1]));
    describe_side(nullptr, err_p, text[2], sizeof(text[2]));
    return fail(REMAP_ERR_UNSUPPORTED, "remap_overlap_grids: %s%s%s", text[0],
                text[1], text[2]);
}

// the workspace in front of the pairs: the mesh path's (a raster of one
// bucket, both sides, the read-back words) and the pyramid
struct GridLayout {
    MeshLayout m;
    size_t first, nodes;
    int levels;
    const GridSide *index, *walker;   // whose pyramid; whose lanes walk it
};

int grid_fixed_layout(const GridSide &A, const GridSide &B, GridLayout *L)
{
    const int rc = mesh_fixed_layout(A.G, B.G, &L->m);
    if (rc != REMAP_OK)
        return rc;
    L->index = B.is_grid ? &B : &A;
    L->walker = B.is_grid ? &A : &B;
    const GridGeom &Q = L->index->Q;
    L->levels = pyramid_levels(Q.ny, Q.nx);
    const int64_t n_nodes = pyramid_first(Q.ny, Q.nx, L->levels, nullptr);
    L->first = take(&L->m.fixed, kMaxLevels * 8);
    L->nodes = take(&L->m.fixed, static_cast<size_t>(n_nodes + 1) * 4 * 8);
    return REMAP_OK;
}

int prep_grid_side(const GridSide &S, bool clipper, const Side &s,
                   double *area, int32_t *status, hipStream_t stream)
{
    hipLaunchKernelGGL(quad_prep, dim3(blocks(S.G.n_cells, kPrepBlock)),
                       dim3(kPrepBlock), 0, stream, S.Q, s.xyz, s.nv, s.centre,
                       area, status);
    REMAP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(cell_shape, dim3(blocks(S.G.n_cells, kBlock)),
                       dim3(kBlock), 0, stream, S.G.n_cells, S.G.max_edges,
                       clipper, s.xyz, s.nv, s.centre, s.radius, status);
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

// both sides prepared, the pyramid, the count pass and its scan: the number
// of candidates in back[3], the sides' error bits in back[2], the walker's
// counts / offs ready for the fill pass.  The areas go to a_area / b_area.
int grid_candidates(GridSide &A, GridSide &B, const GridLayout &L, char *ws,
                    double *a_area, double *b_area, Pyramid *pyramid,
                    hipStream_t stream)
{
    const MeshLayout &lay = L.m;
    double *lat_c = reinterpret_cast<double *>(ws + lay.lat_c);
    double *lon_c = reinterpret_cast<double *>(ws + lay.lon_c);
    int64_t *back = reinterpret_cast<int64_t *>(ws + lay.back);
    int32_t *status_ab = reinterpret_cast<int32_t *>(back + 2);
    void *temp0 = ws + lay.temp0;
    A.G.lat_c = B.G.lat_c = lat_c;
    A.G.lon_c = B.G.lon_c = lon_c;
    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, kBackWords * 8, stream));
    hipLaunchKernelGGL(bucket_edges, dim3(1), dim3(kBlock), 0, stream,
                       int64_t(1), int64_t(1), lat_c, lon_c);
    REMAP_HIP_CHECK(hipGetLastError());
    for (int k = 0; k < 2; ++k) {
        const GridSide &S = k ? A : B;
        const Side s = side_at(ws, k ? lay.a : lay.b);
        double *area = k ? a_area : b_area;
        int32_t *status = k ? status_ab : status_ab + 1;
        const int rc = S.is_grid
            ? prep_grid_side(S, k == 0, s, area, status, stream)
            : prep_side(S.G, k == 0, s, area, temp0, lay.temp0_bytes,
                        back + k, status, stream);
        if (rc != REMAP_OK)
            return rc;
    }
    const Side si = side_at(ws, L.index == &A ? lay.a : lay.b);
    const Side sw = side_at(ws, L.walker == &A ? lay.a : lay.b);
    const GridGeom &Q = L.index->Q;
    int64_t *first = reinterpret_cast<int64_t *>(ws + L.first);
    const Pyramid P = {L.levels, Q.ny, Q.nx, si.centre, si.radius,
                       reinterpret_cast<double *>(ws + L.nodes), first};
    *pyramid = P;
    hipLaunchKernelGGL(pyramid_table, dim3(1), dim3(kWave), 0, stream, Q.ny,
                       Q.nx, L.levels, first);
    REMAP_HIP_CHECK(hipGetLastError());
    for (int l = 1; l < L.levels; ++l) {
        const int64_t n = level_dim(Q.ny, l) * level_dim(Q.nx, l);
        hipLaunchKernelGGL(pyramid_level, dim3(blocks(n, kBlock)),
                           dim3(kBlock), 0, stream, P, l);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    const int64_t n_w = L.walker->G.n_cells;
    if (n_w > 0) {
        hipLaunchKernelGGL(pyramid_walk<false>, dim3(blocks(n_w, kWalkBlock)),
                           dim3(kWalkBlock), 0, stream, P, n_w, sw.centre,
                           sw.radius, sw.nv, L.walker == &A, sw.counts,
                           nullptr, int64_t(0), nullptr, status_ab);
        REMAP_HIP_CHECK(hipGetLastError());
        size_t tb = lay.temp0_bytes;
        REMAP_HIP_CHECK((rocprim::exclusive_scan(
            temp0, tb, static_cast<const uint64_t *>(sw.counts), sw.offs,
            uint64_t(0), static_cast<size_t>(n_w), rocprim::plus<uint64_t>(),
            stream)));
        hipLaunchKernelGGL(scan_total, dim3(1), dim3(kWave), 0, stream, n_w,
                           sw.counts, sw.offs, back + 3);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    return REMAP_OK;
}

int check_sides(const remap_overlap_side *a, const remap_overlap_side *b,
                GridSide *A, GridSide *B)
{
    int rc = check_side(a, "a", A);
    if (rc == REMAP_OK)
        rc = check_side(b, "b", B);
    if (rc != REMAP_OK)
        return rc;
    if (!A->is_grid && !B->is_grid)
        return fail(REMAP_ERR_ARG, "remap_overlap_grids: neither side is a "
                                   "grid (two meshes: remap_overlap_meshes)");
    return REMAP_OK;
}

int grids_sizes(const remap_overlap_side *side_a,
                const remap_overlap_side *side_b, int64_t *n_pairs_out,
                size_t *bytes_out, hipStream_t stream)
{
    GridSide A, B;
    int rc = check_sides(side_a, side_b, &A, &B);
    if (rc != REMAP_OK)
        return rc;
    if (!n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "remap_overlap_grids_sizes: NULL output");
    GridLayout L;
    rc = grid_fixed_layout(A, B, &L);
    if (rc != REMAP_OK)
        return rc;
    // the count pass needs both sides prepared: in memory of its own, with
    // the two area arrays behind it
    const size_t na = static_cast<size_t>(A.G.n_cells > 0 ? A.G.n_cells : 1);
    const size_t nb = static_cast<size_t>(B.G.n_cells > 0 ? B.G.n_cells : 1);
    size_t bytes = L.m.fixed;
    const size_t at_a = take(&bytes, na * 8), at_b = take(&bytes, nb * 8);
    char *buf = nullptr;
    REMAP_HIP_CHECK(hipMalloc(&buf, bytes));
    Pyramid P;
    int64_t got[2] = {0, 0};
    rc = grid_candidates(A, B, L, buf, reinterpret_cast<double *>(buf + at_a),
                         reinterpret_cast<double *>(buf + at_b), &P, stream);
    hipError_t err = hipSuccess;
    if (rc == REMAP_OK) {
        err = hipMemcpyAsync(got, buf + L.m.back + 16, sizeof(got),
                             hipMemcpyDeviceToHost, stream);
        if (err == hipSuccess)
            err = hipStreamSynchronize(stream);
    } else {
        (void)hipStreamSynchronize(stream);
    }
    const hipError_t freed = hipFree(buf);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(err);
    REMAP_HIP_CHECK(freed);
    const int err_a = static_cast<int>(got[0] & 0xffffffff);
    const int err_b = static_cast<int>((got[0] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return grids_fail(err_a, err_b, 0);
    if (got[1] >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_grids: %lld candidate pairs",
                    static_cast<long long>(got[1]));
    rc = mesh_var_layout(0, 0, got[1], &L.m);
    if (rc != REMAP_OK)
        return rc;
    *n_pairs_out = got[1];
    *bytes_out = L.m.total;
    return REMAP_OK;
}

int grids(const remap_overlap_side *side_a, const remap_overlap_side *side_b,
          int32_t dst_is_b, int64_t n_pairs, void *workspace,
          size_t workspace_bytes, int32_t *dst_out, int32_t *src_out,
          double *area_out, double *frac_b_out, double *a_area_out,
          double *b_area_out, int64_t *n_entries_out, hipStream_t stream)
{
    GridSide A, B;
    int rc = check_sides(side_a, side_b, &A, &B);
    if (rc != REMAP_OK)
        return rc;
    if (n_pairs < 0 || n_pairs >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_grids: %lld candidate pairs",
                    static_cast<long long>(n_pairs));
    if (!frac_b_out || !a_area_out || !b_area_out || !n_entries_out ||
        (n_pairs > 0 && (!dst_out || !src_out || !area_out)))
        return fail(REMAP_ERR_ARG, "remap_overlap_grids: NULL output");
    GridLayout L;
    rc = grid_fixed_layout(A, B, &L);
    if (rc == REMAP_OK)
        rc = mesh_var_layout(0, 0, n_pairs, &L.m);
    if (rc != REMAP_OK)
        return rc;
    const MeshLayout &lay = L.m;
    if (!workspace || workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "remap_overlap_grids: workspace of %zu bytes, need %zu",
                    workspace_bytes, lay.total);
    char *ws = static_cast<char *>(workspace);
    Pyramid P;
    rc = grid_candidates(A, B, L, ws, a_area_out, b_area_out, &P, stream);
    if (rc != REMAP_OK)
        return rc;
    int64_t *back = reinterpret_cast<int64_t *>(ws + lay.back);
    const Side sa = side_at(ws, lay.a), sb = side_at(ws, lay.b);
    const Side sw = L.walker == &A ? sa : sb;
    const PairWork work = {reinterpret_cast<uint64_t *>(ws + lay.cand),
                           reinterpret_cast<uint64_t *>(ws + lay.cand_s),
                           reinterpret_cast<double *>(ws + lay.parea),
                           reinterpret_cast<double *>(ws + lay.area_c),
                           reinterpret_cast<uint32_t *>(ws + lay.head),
                           reinterpret_cast<uint32_t *>(ws + lay.slot),
                           reinterpret_cast<uint64_t *>(back + 3),
                           back + 4,
                           reinterpret_cast<int32_t *>(back + 5),
                           ws + lay.temp,
                           lay.temp_bytes};
    const bool dst_is_a = dst_is_b == 0;
    const int64_t n_w = L.walker->G.n_cells;
    if (n_w > 0) {
        // (with n_pairs 0 it only checks that there are none)
        hipLaunchKernelGGL(pyramid_walk<true>, dim3(blocks(n_w, kWalkBlock)),
                           dim3(kWalkBlock), 0, stream, P, n_w, sw.centre,
                           sw.radius, sw.nv, L.walker == &A, sw.counts,
                           sw.offs, n_pairs, work.cand, work.status);
        REMAP_HIP_CHECK(hipGetLastError());
    }
    if (n_pairs > 0) {
        rc = clip_and_keep(A.G, sa, B.G, sb, dst_is_a, n_pairs, work,
                           a_area_out, b_area_out, stream);
        if (rc != REMAP_OK)
            return rc;
    }
    // the one read-back: the sides' error bits, the candidates, how many
    // entries to sort, the pairs' error bits
    int64_t got[4];
    REMAP_HIP_CHECK(hipMemcpyAsync(got, back + 2, sizeof(got),
                                   hipMemcpyDeviceToHost, stream));
    REMAP_HIP_CHECK(hipStreamSynchronize(stream));
    const int err_a = static_cast<int>(got[0] & 0xffffffff);
    const int err_b = static_cast<int>((got[0] >> 32) & 0xffffffff);
    int err_p = static_cast<int>(got[3] & 0xffffffff);
    if (got[1] != n_pairs)
        err_p |= REMAP_OVERLAP_ERR_CAPACITY;
    if (err_a || err_b || err_p)
        return grids_fail(err_a, err_b, err_p);
    *n_entries_out = got[2];
    return sort_and_sum(dst_is_a ? A.G.n_cells : B.G.n_cells, got[2], n_pairs,
                        work, dst_out, src_out, area_out,
                        dst_is_a ? a_area_out : b_area_out, frac_b_out,
                        stream);
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

int remap_overlap_meshes_sizes(const remap_overlap_mesh *a,
                               const remap_overlap_mesh *b, int64_t *counter,
                               int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream)
{
    return remap::meshes_sizes("remap_overlap_meshes", a, b, counter,
                               n_pairs_out, workspace_bytes_out,
                               static_cast<hipStream_t>(stream));
}

int remap_overlap_meshes(const remap_overlap_mesh *a,
                         const remap_overlap_mesh *b, int32_t dst_is_b,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *a_area_out,
                         double *b_area_out, int64_t *n_entries_out,
                         void *stream)
{
    return remap::meshes(a, b, dst_is_b, n_pairs, workspace, workspace_bytes,
                         dst_out, src_out, area_out, frac_b_out, a_area_out,
                         b_area_out, n_entries_out,
                         static_cast<hipStream_t>(stream));
}

int remap_overlap_pieces_sizes(const struct remap_overlap_pieces *a,
                               const struct remap_overlap_pieces *b, int64_t *counter,
                               int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream)
{
    return remap::pieces_sizes(a, b, counter, n_pairs_out,
                               workspace_bytes_out,
                               static_cast<hipStream_t>(stream));
}

int remap_overlap_pieces(const struct remap_overlap_pieces *a,
                         const struct remap_overlap_pieces *b, int32_t dst_is_b,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *a_area_out,
                         double *b_area_out, int64_t *n_entries_out,
                         void *stream)
{
    return remap::pieces(a, b, dst_is_b, n_pairs, workspace, workspace_bytes,
                         dst_out, src_out, area_out, frac_b_out, a_area_out,
                         b_area_out, n_entries_out,
                         static_cast<hipStream_t>(stream), nullptr);
}

int remap_overlap_pieces_timed(const struct remap_overlap_pieces *a,
                               const struct remap_overlap_pieces *b,
                               int32_t dst_is_b, int64_t n_pairs,
                               void *workspace, size_t workspace_bytes,
                               int32_t *dst_out, int32_t *src_out,
                               double *area_out, double *frac_b_out,
                               double *a_area_out, double *b_area_out,
                               int64_t *n_entries_out, float *phase_ms_out,
                               void *stream)
{
    return remap::pieces_timed(a, b, dst_is_b, n_pairs, workspace,
                               workspace_bytes, dst_out, src_out, area_out,
                               frac_b_out, a_area_out, b_area_out,
                               n_entries_out, phase_ms_out,
                               static_cast<hipStream_t>(stream));
}

int remap_overlap_grids_sizes(const remap_overlap_side *a,
                              const remap_overlap_side *b,
                              int64_t *n_pairs_out,
                              size_t *workspace_bytes_out, void *stream)
{
    return remap::grids_sizes(a, b, n_pairs_out, workspace_bytes_out,
                              static_cast<hipStream_t>(stream));
}

int remap_overlap_grids(const remap_overlap_side *a,
                        const remap_overlap_side *b, int32_t dst_is_b,
                        int64_t n_pairs, void *workspace,
                        size_t workspace_bytes, int32_t *dst_out,
                        int32_t *src_out, double *area_out,
                        double *frac_b_out, double *a_area_out,
                        double *b_area_out, int64_t *n_entries_out,
                        void *stream)
{
    return remap::grids(a, b, dst_is_b, n_pairs, workspace, workspace_bytes,
                        dst_out, src_out, area_out, frac_b_out, a_area_out,
                        b_area_out, n_entries_out,
                        static_cast<hipStream_t>(stream));
}

}  // extern "C"
