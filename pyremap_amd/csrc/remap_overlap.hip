// remap_overlap.hip -- first-order conservative overlaps on the sphere (what
// ESMF_RegridWeightGen --method conserve computes), four routes to one back
// end:
//   remap_overlap_latlon   an MPAS cell mesh and a lat-lon grid
//   remap_overlap_meshes   two MPAS cell meshes
//   remap_overlap_pieces   cells that come in convex pieces
//   remap_overlap_grids    a structured 2-D grid on one side or both
//
// Geometry (ESMF's convention): every cell is a spherical polygon with
// great-circle edges, lat-lon cells included -- their "lat lines" are the
// great-circle arcs between their corners.  Corners at a pole coincide, so
// the polar rows' cells are triangles (a repeated corner is a zero-length
// edge, which clips nothing and adds no area).  A_ij = spherical area of
// (cell i n cell j); polygon areas come from the same formula.
//
// Every route (all on the caller's stream, fp64 throughout, no float
// atomics) prepares the cells of side a (the subject) and side b (the
// clipper), lists candidate pairs a << 32 | b, clips, and hands over to the
// shared back end:
//   cell_prep      one lane per mesh cell: vertices -> unit xyz (consecutive
//                  duplicates dropped, turned counter-clockwise seen from
//                  outside), the cell's own area, its centre and its
//                  (lat, lon) box -- latitude extrema of the great-circle
//                  arcs included, the poles' cells reaching +-90 deg over the
//                  whole circle -- as rows and column ranges of a lat-lon
//                  grid (the grid itself, or a raster of buckets)
//   candidates     per route: the boxes (latlon), buckets the boxes share
//                  (meshes, pieces), a pyramid of bounding caps (grids)
//   the clip       Tangent / load_ring / clip_edge: gnomonic projection about
//                  the subject's centre (great circles -> straight lines),
//                  Sutherland-Hodgman by the clipper's edges in that plane;
//                  clip_pairs (the four edges of a lat-lon cell, the area
//                  from the vertices lifted to the sphere) and
//                  clip_pairs_poly (a convex cell's edges, the area in the
//                  plane) are its two kernels.  The polygons being clipped
//                  live in per-lane LDS slots (runtime-indexed private
//                  arrays would go to scratch on gfx950)
//   keep_pairs     flag / scan / scatter: keep A_ij > kSliver * A_dst, re-key
//                  (dst, src)
//   sort_and_sum   rocPRIM radix_sort_pairs on (dst << 32 | src, A);
//                  dst_sums, one lane per destination cell: its entries
//                  summed in that order -> frac_b = min(sum / A_dst, 1)
// remap_overlap_pieces leaves the back end after the clip: the piece pairs
// are re-keyed to their cells, sorted, and merge_runs adds every run of equal
// keys up in a fixed order before the sliver rule is applied to the sum.
//
// The host side is written with remap_host.h's helpers (launch, at,
// read_back, the typed rocPRIM calls, take() for every workspace layout) and
// one Route table per entry point that turns the error bits into text
// (route_fail).
// Host read-backs: one in remap_overlap_latlon, two in remap_overlap_meshes,
// one in remap_overlap_grids (the entry count with every error bit, before
// the sort), remap_overlap_meshes' two and up to two more in
// remap_overlap_pieces (the parents' check, the entry count behind the
// merge); each _sizes call reads its count back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string.h>

#include "remap_clip.h"
#include "remap_common.h"
#include "remap_host.h"
#include "remap_sphere.h"

namespace remap {
namespace {

// (kMaxEdges, kClipBlock, kMinCos: remap_clip.h)  One clip by a half-plane
// adds at most one vertex: four lat-lon edges.  Rounding can break that bound where mesh vertices lie on a lat-lon edge
// (their signs alternate along it); a polygon that would outgrow kMaxOut is
// an error (kErrClip), never truncated
constexpr int kMaxOut = kMaxEdges + 4;
// the status bit of that error, next to REMAP_OVERLAP_ERR_* (the bits stay
// inside the library: callers see REMAP_ERR_UNSUPPORTED and the message)
constexpr int kErrClip = 16;
constexpr int kPrepBlock = 64;
// entries with A_ij <= kSliver * A_dst are dropped: touching along an edge
// or at a corner leaves rounding-level areas, not overlaps
constexpr double kSliver = 1e-14;
// slack of the boxes, radians (rounding of the corners' lat / lon)
constexpr double kBoxEps = 1e-9;

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

// (Ring, finish_ring, CellRing and convex_cell: remap_clip.h)

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

// ---------------------------------------------------------------------------
// the clip both clip kernels share: a polygon in the gnomonic plane of a
// centre, in one lane's LDS ring [buffer][vertex][lane] (ping-pong), cut by
// one directed edge at a time
// ---------------------------------------------------------------------------

// (Tangent, tangent_at, load_ring and clip_edge: remap_clip.h, shared with
// the overlap moments of remap_conserve2nd.hip)

// one lane per candidate pair mesh cell << 32 | lat-lon cell: the mesh cell's
// polygon cut by the lat-lon cell's four edges, the area of the result from
// its vertices lifted back to the sphere (a fan of tri_area)
__global__ __launch_bounds__(kClipBlock) void clip_pairs(
    Geom G, bool swap, int64_t n_pairs, const uint64_t *__restrict__ keys,
    const double *__restrict__ cell_xyz, const int32_t *__restrict__ cell_nv,
    const double *__restrict__ cell_centre, double *__restrict__ area,
    int32_t *__restrict__ status)
{
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
    const Tangent T = tangent_at({cell_centre[c * 3], cell_centre[c * 3 + 1],
                                  cell_centre[c * 3 + 2]});
    bool bad = !load_ring(T, cell_xyz + c * G.max_edges * 3, nv, px, py, lane);
    const Quad quad = grid_cell(G.lat_c, G.lon_c, G.n_lon, g, swap);
    double qx[4], qy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double t;
        T.project(quad.p[k], &qx[k], &qy[k], &t);
        bad |= !(t >= kMinCos);
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
        n = clip_edge(px, py, lane, cur, n, ax, ay, dx, dy);
        if (n > kMaxOut) {
            atomicOr(status, kErrClip);
            area[p] = 0.0;
            return;
        }
        cur ^= 1;
    }
    double a = 0.0;
    if (n >= 3) {
        const V3 cc = T.cc, e1 = T.e1, e2 = T.e2;
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

// ---------------------------------------------------------------------------
// what the four routes share on the host: the error bits as text, the
// workspace of one side's prepared cells and of the pairs, and the back end
// behind the clip (keep_pairs, the one read-back of the count, sort_and_sum)
// ---------------------------------------------------------------------------

// a route's entry point and its words for the error bits, in the order of
// kErrBits (a side's text is cut at `room`, as snprintf always cut it)
constexpr int kErrBits[6] = {REMAP_OVERLAP_ERR_EDGES, REMAP_OVERLAP_ERR_VERTEX,
                             REMAP_OVERLAP_ERR_CONVEX,
                             REMAP_OVERLAP_ERR_HEMISPHERE, kErrClip,
                             REMAP_OVERLAP_ERR_CAPACITY};
struct Route {
    const char *who;
    const char *side;    // what a side is called, before its name
    size_t room;
    bool name_convex;    // "(REMAP_OVERLAP_ERR_CONVEX)" behind everything
    const char *bit[6];
};

const Route kLatlon = {
    "remap_overlap_latlon", "", kErrorBufferSize, false,
    {"a cell has more edges than this build serves "
     "(REMAP_OVERLAP_MAX_EDGES); ",
     "a cell has fewer than 3 distinct vertices or a vertex index out of "
     "range; ",
     "",
     "a candidate pair has a vertex outside the tangent hemisphere of the "
     "mesh cell's centre; ",
     "a clipped polygon outgrew its REMAP_OVERLAP_MAX_EDGES + 4 vertices "
     "(mesh vertices on a lat-lon edge); ",
     "more candidate pairs than n_pairs (a stale "
     "remap_overlap_latlon_sizes)"}};

const Route kMeshes = {
    "remap_overlap_meshes", "mesh ", 192, false,
    {"a cell has more edges than this build serves "
     "(REMAP_OVERLAP_MAX_EDGES); ",
     "a cell has fewer than 3 distinct vertices or a vertex index out of "
     "range; ",
     "a cell is not convex (mesh b's cells clip); ",
     "a candidate pair has a vertex outside the tangent hemisphere of the "
     "mesh a cell's centre; ",
     "a clipped polygon outgrew its 2 x REMAP_OVERLAP_MAX_EDGES vertices; ",
     "the candidate pairs differ from n_pairs (a stale "
     "remap_overlap_meshes_sizes); "}};

// (the pieces are meshes; remap_overlap_pieces names the convexity bit)
const Route kPieces = {"remap_overlap_pieces", kMeshes.side, kMeshes.room, true,
                       {kMeshes.bit[0], kMeshes.bit[1], kMeshes.bit[2],
                        kMeshes.bit[3], kMeshes.bit[4], kMeshes.bit[5]}};

const Route kGrids = {
    "remap_overlap_grids", "side ", 256, false,
    {"a cell has more edges than this build serves "
     "(REMAP_OVERLAP_ERR_EDGES); ",
     "a cell has fewer than 3 distinct corners or a vertex index out of "
     "range (REMAP_OVERLAP_ERR_VERTEX); ",
     "a cell is not convex and side b's cells clip "
     "(REMAP_OVERLAP_ERR_CONVEX); ",
     "a candidate pair has a vertex outside the tangent hemisphere of the "
     "side a cell's centre (REMAP_OVERLAP_ERR_HEMISPHERE); ",
     "a clipped polygon outgrew its 2 x REMAP_OVERLAP_MAX_EDGES vertices; ",
     "the candidate pairs differ from n_pairs, a stale "
     "remap_overlap_grids_sizes (REMAP_OVERLAP_ERR_CAPACITY); "}};

// the error bits of one side, or of the pairs (name NULL), as text
void describe(const Route &R, const char *name, int err, char *out)
{
    out[0] = '\0';
    if (!err)
        return;
    size_t n = name ? snprintf(out, R.room, "%s%s: ", R.side, name) : 0;
    for (int k = 0; k < 6 && n < R.room; ++k)
        if (err & kErrBits[k])
            n += snprintf(out + n, R.room - n, "%s", R.bit[k]);
}

int route_fail(const Route &R, int err_a, int err_b, int err_p)
{
    char text[3][kErrorBufferSize];
    describe(R, "a", err_a, text[0]);
    describe(R, "b", err_b, text[1]);
    describe(R, nullptr, err_p, text[2]);
    return fail(REMAP_ERR_UNSUPPORTED, "%s: %s%s%s%s", R.who, text[0], text[1],
                text[2],
                R.name_convex && ((err_a | err_b) & REMAP_OVERLAP_ERR_CONVEX)
                    ? "(REMAP_OVERLAP_ERR_CONVEX)"
                    : "");
}

// what every run writes (dst / src / area may be NULL with no pairs)
struct Outputs {
    int32_t *dst, *src;
    double *area, *frac_b, *a_area, *b_area;
    int64_t *n_entries;
};

int check_call(const char *who, int64_t n_pairs, const Outputs &out)
{
    if (n_pairs < 0 || n_pairs >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED, "%s: %lld candidate pairs", who,
                    static_cast<long long>(n_pairs));
    if (!out.frac_b || !out.a_area || !out.b_area || !out.n_entries ||
        (n_pairs > 0 && (!out.dst || !out.src || !out.area)))
        return fail(REMAP_ERR_ARG, "%s: NULL output", who);
    return REMAP_OK;
}

// one side's prepared cells in the workspace (radius: the mesh and grid
// routes' cell_shape; the lat-lon route takes none)
struct SideLayout {
    size_t xyz, nv, centre, radius, boxes, counts, offs;
};

SideLayout side_layout(const Geom &G, bool radius, size_t *off)
{
    const size_t c = at_least_one(G.n_cells);
    SideLayout s;
    s.xyz = take(off, c * G.max_edges * 3 * 8);
    s.nv = take(off, c * 4);
    s.centre = take(off, c * 3 * 8);
    s.radius = radius ? take(off, c * 8) : 0;
    s.boxes = take(off, c * sizeof(Box));
    s.counts = take(off, c * 8);
    s.offs = take(off, c * 8);
    return s;
}

struct Side {
    double *xyz, *centre, *radius;
    int32_t *nv;
    Box *boxes;
    uint64_t *counts, *offs;
};

Side side_at(char *ws, const SideLayout &s)
{
    return {at<double>(ws, s.xyz), at<double>(ws, s.centre),
            at<double>(ws, s.radius), at<int32_t>(ws, s.nv),
            at<Box>(ws, s.boxes), at<uint64_t>(ws, s.counts),
            at<uint64_t>(ws, s.offs)};
}

// the buffers of the pairs (n_pairs each) from the clip on
struct PairLayout {
    size_t cand, cand_s, parea, area_c, head, slot;
};

PairLayout pair_layout(size_t n, size_t *off)
{
    PairLayout p;
    // candidates (the mesh routes: then the unique pairs); then the sorted
    // entry keys
    p.cand = take(off, n * 8);
    // (the mesh route: sorted candidates;) the kept entries' keys
    p.cand_s = take(off, n * 8);
    p.parea = take(off, n * 8);
    p.area_c = take(off, n * 8);
    p.head = take(off, n * 4);
    p.slot = take(off, n * 4);
    return p;
}

struct PairWork {
    uint64_t *cand, *cand_s;   // the pairs a << 32 | b; the kept entries' keys
    double *parea, *area_c;
    uint32_t *head, *slot;
    uint64_t *n_unique;        // (the lat-lon route has none)
    int64_t *n_kept;           // the error bits of the pairs in the word behind
    int32_t *status;
    void *temp;
    size_t temp_bytes;
};

PairWork pair_work(char *ws, const PairLayout &p, int64_t *counts, void *temp,
                   size_t temp_bytes)
{
    // counts: [0] unique pairs, [1] entries, [2] the pairs' error bits
    return {at<uint64_t>(ws, p.cand), at<uint64_t>(ws, p.cand_s),
            at<double>(ws, p.parea), at<double>(ws, p.area_c),
            at<uint32_t>(ws, p.head), at<uint32_t>(ws, p.slot),
            as<uint64_t>(counts), counts + 1,
            as<int32_t>(counts + 2), temp, temp_bytes};
}

// flag / scan / scatter over the clipped pairs in w.cand / w.parea: the
// entries with A > kSliver * A_dst re-keyed (dst, src) in w.cand_s /
// w.area_c, their number in *w.n_kept
int keep_pairs(int64_t n_pairs, int64_t n_a, int64_t n_b, bool dst_is_a,
               const PairWork &w, const double *a_area, const double *b_area,
               hipStream_t stream)
{
    REMAP_TRY(launch(flag_kept, n_pairs, kBlock, stream, n_pairs, n_a, n_b,
                     dst_is_a, w.cand, w.parea, a_area, b_area, w.head));
    if (n_pairs > 0)
        REMAP_TRY(exclusive_scan(w.temp, w.temp_bytes, w.head, w.slot, n_pairs,
                                 stream));
    return launch(scatter_kept, n_pairs, kBlock, stream, n_pairs, dst_is_a,
                  w.cand, w.parea, w.head, w.slot, w.cand_s, w.area_c,
                  w.n_kept);
}

// the kept entries sorted by (dst, src) into the outputs, frac_b of every
// destination cell (w.cand is the sort's key output)
int sort_and_sum(int64_t n_dst, int64_t n_entries, int64_t n_pairs,
                 const PairWork &w, const Outputs &out, const double *dst_area,
                 hipStream_t stream)
{
    if (n_entries > 0)
        REMAP_TRY(radix_sort_pairs(w.temp, w.temp_bytes, w.cand_s, w.cand,
                                   w.area_c, out.area, n_entries, stream));
    REMAP_TRY(launch(split_keys, n_entries, kBlock, stream, w.n_kept, n_pairs,
                     w.cand, out.dst, out.src));
    return launch(dst_sums, n_dst, kBlock, stream, n_dst, w.n_kept, out.dst,
                  out.area, dst_area, out.frac_b);
}

// ---------------------------------------------------------------------------
// an MPAS mesh and a lat-lon grid (remap_overlap_latlon): the mesh is side a
// ---------------------------------------------------------------------------

struct Layout {
    SideLayout cells;
    PairLayout pairs;
    // the entry count and the error bits side by side (behind a word that is
    // not used: pair_work's n_unique): one read-back
    size_t counts, temp, total;
    size_t temp_bytes;
};

int make_layout(const Geom &G, int64_t n_pairs, Layout *lay)
{
    const size_t c = at_least_one(G.n_cells), n = at_least_one(n_pairs);
    size_t scan_c = 0, scan_n = 0, sort_n = 0;
    REMAP_TRY(scan_temp<uint64_t>(c, &scan_c));
    REMAP_TRY(scan_temp<uint32_t>(n, &scan_n));
    REMAP_TRY(sort_pairs_temp<double>(n, &sort_n));
    lay->temp_bytes = std::max({scan_c, scan_n, sort_n});
    size_t off = 0;
    lay->cells = side_layout(G, false, &off);
    lay->pairs = pair_layout(n, &off);
    lay->counts = take(&off, 24);
    lay->temp = take(&off, lay->temp_bytes);
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
    REMAP_TRY(read_back(&ends[3], G.lon_c + G.n_lon, 8, stream));
    *swap = (ends[1] < ends[0]) != (ends[3] < ends[2]);
    return REMAP_OK;
}

int overlap_sizes(const remap_overlap_geom *geom, int64_t *counter,
                  int64_t *n_pairs_out, size_t *bytes_out, hipStream_t stream)
{
    Geom G;
    REMAP_TRY(check_geom(geom, &G));
    if (!counter || !n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "remap_overlap_latlon_sizes: NULL output");
    REMAP_HIP_CHECK(hipMemsetAsync(counter, 0, 2 * sizeof(int64_t), stream));
    // (count only: the total in counter[0], the error bits in counter[1])
    REMAP_TRY(launch(cell_prep, G.n_cells, kPrepBlock, stream, G, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr,
                     as<unsigned long long>(counter),
                     as<int32_t>(counter + 1)));
    int64_t got[2];
    REMAP_TRY(read_back(got, counter, sizeof(got), stream));
    // (its own punctuation, not kLatlon's)
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
    REMAP_TRY(make_layout(G, got[0], &lay));
    *n_pairs_out = got[0];
    *bytes_out = lay.total;
    return REMAP_OK;
}

int overlap(const remap_overlap_geom *geom, int32_t dst_is_mesh,
            int64_t n_pairs, void *workspace, size_t workspace_bytes,
            const Outputs &out, hipStream_t stream)
{
    Geom G;
    REMAP_TRY(check_geom(geom, &G));
    REMAP_TRY(check_call(kLatlon.who, n_pairs, out));
    Layout lay;
    REMAP_TRY(make_layout(G, n_pairs, &lay));
    REMAP_TRY(need_workspace("remap_overlap_latlon", workspace,
                             workspace_bytes, lay.total));
    bool swap = false;
    REMAP_TRY(axis_swap(G, stream, &swap));
    char *ws = static_cast<char *>(workspace);
    const Side s = side_at(ws, lay.cells);
    int64_t *counts = at<int64_t>(ws, lay.counts);
    const PairWork w = pair_work(ws, lay.pairs, counts, ws + lay.temp,
                                 lay.temp_bytes);
    const int64_t n_grid = G.n_lat * G.n_lon;

    REMAP_HIP_CHECK(hipMemsetAsync(counts, 0, 24, stream));
    REMAP_TRY(launch(grid_area, n_grid, kBlock, stream, G, swap, out.b_area));
    REMAP_TRY(launch(cell_prep, G.n_cells, kPrepBlock, stream, G, s.xyz, s.nv,
                     s.centre, out.a_area, s.boxes, s.counts, nullptr,
                     w.status));
    if (G.n_cells > 0)
        REMAP_TRY(exclusive_scan(w.temp, w.temp_bytes, s.counts, s.offs,
                                 G.n_cells, stream));
    REMAP_TRY(launch(fill_pairs<false>, G.n_cells, kBlock, stream, G, s.boxes,
                     s.offs, n_pairs, w.cand, w.status));
    REMAP_TRY(launch(clip_pairs, n_pairs, kClipBlock, stream, G, swap, n_pairs,
                     w.cand, s.xyz, s.nv, s.centre, w.parea, w.status));
    REMAP_TRY(keep_pairs(n_pairs, G.n_cells, n_grid, dst_is_mesh != 0, w,
                         out.a_area, out.b_area, stream));
    // the one read-back: how many entries to sort, the error bits
    int64_t back[2];
    REMAP_TRY(read_back(back, w.n_kept, 16, stream));
    if (const int err = static_cast<int>(back[1] & 0xffffffff))
        return route_fail(kLatlon, 0, 0, err);
    *out.n_entries = back[0];
    return sort_and_sum(dst_is_mesh ? G.n_cells : n_grid, back[0], n_pairs, w,
                        out, dst_is_mesh ? out.a_area : out.b_area, stream);
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
//   keep_pairs, the read-back of the count, sort_and_sum as above
//   (dst_is_b only re-keys)
// ---------------------------------------------------------------------------

// one clip by an edge of a convex clipper adds at most one vertex
constexpr int kMaxOutPoly = 2 * kMaxEdges;
// bucket rows of the raster: sqrt(n_b / 2), within these bounds
constexpr int64_t kMinBucketRows = 2;
constexpr int64_t kMaxBucketRows = 8192;
constexpr uint64_t kLow = 0xffffffffull;

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
// cut by b's edges (b convex) in the tangent plane of a's centre; lanes past
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
    const Tangent T = tangent_at(ca);
    const int na = nv_a[a], nb = nv_b[b];
    const CellRing vb = {xyz_b + b * max_edges_b * 3};
    bool bad = !load_ring(T, xyz_a + a * max_edges_a * 3, na, px, py, lane);
    for (int k = 0; k < nb; ++k)
        bad |= !(dot(vb[k], ca) >= kMinCos);
    if (bad) {
        atomicOr(status, REMAP_OVERLAP_ERR_HEMISPHERE);
        area[p] = 0.0;
        return;
    }
    double fx, fy, t;
    T.project(vb[0], &fx, &fy, &t);
    double ax = fx, ay = fy;
    int n = na, cur = 0;
    for (int e = 0; e < nb && n > 0; ++e) {
        double bx = fx, by = fy;
        if (e + 1 < nb)
            T.project(vb[e + 1], &bx, &by, &t);
        const double dx = bx - ax, dy = by - ay;
        if (dx != 0.0 || dy != 0.0) {
            n = clip_edge(px, py, lane, cur, n, ax, ay, dx, dy);
            if (n > kMaxOutPoly) {
                atomicOr(status, kErrClip);
                area[p] = 0.0;
                return;
            }
            cur ^= 1;
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

struct MeshLayout {
    // known from the sizes of the meshes
    size_t lat_c, lon_c, start, back, temp0, fixed;
    SideLayout a, b;
    size_t temp0_bytes;
    // known from the bucket key counts (the first read-back)
    size_t bkeys, bkeys_s, akeys, pcnt, poff;
    PairLayout pairs;
    size_t temp, total;
    size_t temp_bytes;
};

// the read-back words: [0] b's keys, [1] a's keys, [2] the error bits of a
// (low half) and b (high half), [3] unique pairs, [4] entries, [5] the
// pairs' error bits
constexpr int kBackWords = 6;

int mesh_fixed_layout(const Geom &A, const Geom &B, MeshLayout *L)
{
    REMAP_TRY(scan_temp<uint64_t>(
        at_least_one(std::max(A.n_cells, B.n_cells)), &L->temp0_bytes));
    const size_t n_buckets = static_cast<size_t>(A.n_lat * A.n_lon);
    size_t off = 0;
    L->lat_c = take(&off, (A.n_lat + 1) * 8);
    L->lon_c = take(&off, (A.n_lon + 1) * 8);
    L->start = take(&off, (n_buckets + 1) * 4);
    L->back = take(&off, kBackWords * 8);
    L->a = side_layout(A, true, &off);
    L->b = side_layout(B, true, &off);
    L->temp0 = take(&off, L->temp0_bytes);
    L->fixed = off;
    return REMAP_OK;
}

int mesh_var_layout(int64_t n_akeys, int64_t n_bkeys, int64_t n_pairs,
                    MeshLayout *L)
{
    const size_t na = at_least_one(n_akeys), nb = at_least_one(n_bkeys);
    const size_t n = at_least_one(n_pairs);
    size_t t[6];
    REMAP_TRY(sort_keys_temp(nb, &t[0]));
    REMAP_TRY(scan_temp<uint64_t>(na, &t[1]));
    REMAP_TRY(sort_keys_temp(n, &t[2]));
    REMAP_TRY(unique_temp(n, &t[3]));
    REMAP_TRY(scan_temp<uint32_t>(n, &t[4]));
    REMAP_TRY(sort_pairs_temp<double>(n, &t[5]));
    L->temp_bytes = *std::max_element(t, t + 6);
    size_t off = L->fixed;
    L->bkeys = take(&off, nb * 8);
    L->bkeys_s = take(&off, nb * 8);
    L->akeys = take(&off, na * 8);
    L->pcnt = take(&off, na * 8);
    L->poff = take(&off, na * 8);
    L->pairs = pair_layout(n, &off);
    L->temp = take(&off, L->temp_bytes);
    L->total = off;
    return REMAP_OK;
}

// the count pass: mesh b's cells into the histogram of the buckets, mesh a's
// sums over it; counter[0] candidates, [1] a's keys, [2] b's keys, [3] the
// error bits of a (low half) and b (high half), read back into got
int count_meshes(const Geom &A, const Geom &B, uint32_t *hist, double *lat_c,
                 double *lon_c, int64_t *counter, int64_t *got,
                 hipStream_t stream)
{
    REMAP_HIP_CHECK(hipMemsetAsync(counter, 0, 4 * sizeof(int64_t), stream));
    REMAP_HIP_CHECK(hipMemsetAsync(hist, 0, A.n_lat * A.n_lon * 4, stream));
    REMAP_TRY(launch(bucket_edges, A.n_lon + 1, kBlock, stream, A.n_lat,
                     A.n_lon, lat_c, lon_c));
    unsigned long long *cnt = as<unsigned long long>(counter);
    int32_t *status = as<int32_t>(counter + 3);
    REMAP_TRY(launch(mesh_count, B.n_cells, kPrepBlock, stream, B, true, hist,
                     cnt + 2, cnt, status + 1));
    REMAP_TRY(launch(mesh_count, A.n_cells, kPrepBlock, stream, A, false, hist,
                     cnt + 1, cnt, status));
    return read_back(got, counter, 4 * sizeof(int64_t), stream);
}

int meshes_sizes(const Route &R, const remap_overlap_mesh *mesh_a,
                 const remap_overlap_mesh *mesh_b, int64_t *counter,
                 int64_t *n_pairs_out, size_t *bytes_out, hipStream_t stream)
{
    Geom A, B;
    REMAP_TRY(check_mesh(mesh_a, "a", &A));
    REMAP_TRY(check_mesh(mesh_b, "b", &B));
    if (!counter || !n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "%s_sizes: NULL output", R.who);
    bucket_raster(B.n_cells, &A, &B);
    // the histogram of b's cells over the buckets, and the raster
    size_t bytes = 0;
    const size_t at_hist = take(&bytes, A.n_lat * A.n_lon * 4);
    const size_t at_lat = take(&bytes, (A.n_lat + 1) * 8);
    const size_t at_lon = take(&bytes, (A.n_lon + 1) * 8);
    char *buf = nullptr;
    REMAP_HIP_CHECK(hipMalloc(&buf, bytes));
    A.lat_c = B.lat_c = at<double>(buf, at_lat);
    A.lon_c = B.lon_c = at<double>(buf, at_lon);
    int64_t got[4];
    const int rc = count_meshes(A, B, at<uint32_t>(buf, at_hist),
                                at<double>(buf, at_lat),
                                at<double>(buf, at_lon), counter, got, stream);
    const hipError_t freed = hipFree(buf);
    REMAP_TRY(rc);
    REMAP_HIP_CHECK(freed);
    const int err_a = static_cast<int>(got[3] & 0xffffffff);
    const int err_b = static_cast<int>((got[3] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return route_fail(R, err_a, err_b, 0);
    MeshLayout lay;
    REMAP_TRY(mesh_fixed_layout(A, B, &lay));
    REMAP_TRY(mesh_var_layout(got[1], got[2], got[0], &lay));
    *n_pairs_out = got[0];
    *bytes_out = lay.total;
    return REMAP_OK;
}

// cell_prep, cell_shape, the scan of the bucket counts and its total
int prep_side(const Geom &G, bool clipper, const Side &s, double *area,
              void *temp, size_t temp_bytes, int64_t *total, int32_t *status,
              hipStream_t stream)
{
    if (G.n_cells <= 0)
        return REMAP_OK;
    REMAP_TRY(launch(cell_prep, G.n_cells, kPrepBlock, stream, G, s.xyz, s.nv,
                     s.centre, area, s.boxes, s.counts, nullptr, status));
    REMAP_TRY(launch(cell_shape, G.n_cells, kBlock, stream, G.n_cells,
                     G.max_edges, clipper, s.xyz, s.nv, s.centre, s.radius,
                     status));
    REMAP_TRY(exclusive_scan(temp, temp_bytes, s.counts, s.offs, G.n_cells,
                             stream));
    return launch(scan_total, 1, kWave, stream, G.n_cells, s.counts, s.offs,
                  total);
}

// clip_pairs_poly over the pairs in w.cand (the first *w.n_unique of
// n_pairs): their areas in w.parea
int clip_poly(const Geom &A, const Side &sa, const Geom &B, const Side &sb,
              int64_t n_pairs, const PairWork &w, hipStream_t stream)
{
    return launch(clip_pairs_poly, n_pairs, kClipBlock, stream, A.n_cells,
                  A.max_edges, B.n_cells, B.max_edges, n_pairs, w.n_unique,
                  w.cand, sa.xyz, sa.nv, sa.centre, sa.radius, sb.xyz, sb.nv,
                  sb.centre, sb.radius, w.parea, w.status);
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
// ev (6 events or NULL) receives the phase marks [0] start, [1] cells
// prepared, [2] pairs listed.
int mesh_front(const Route &route, const remap_overlap_mesh *mesh_a,
               const remap_overlap_mesh *mesh_b, int64_t n_pairs,
               void *workspace, size_t workspace_bytes, const Outputs &out,
               double *a_area, double *b_area, hipStream_t stream,
               hipEvent_t *ev, MeshRun *R)
{
    const char *who = route.who;
    Geom &A = R->A, &B = R->B;
    REMAP_TRY(check_mesh(mesh_a, "a", &A));
    REMAP_TRY(check_mesh(mesh_b, "b", &B));
    REMAP_TRY(check_call(who, n_pairs, out));
    bucket_raster(B.n_cells, &A, &B);
    const int64_t n_buckets = A.n_lat * A.n_lon;
    MeshLayout &lay = R->lay;
    REMAP_TRY(mesh_fixed_layout(A, B, &lay));
    if (!workspace || workspace_bytes < lay.fixed)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need at least %zu", who,
                    workspace_bytes, lay.fixed);
    char *ws = static_cast<char *>(workspace);
    double *lat_c = at<double>(ws, lay.lat_c);
    double *lon_c = at<double>(ws, lay.lon_c);
    uint32_t *start = at<uint32_t>(ws, lay.start);
    int64_t *back = at<int64_t>(ws, lay.back);
    int32_t *status_ab = as<int32_t>(back + 2);
    R->back = back;
    R->sa = side_at(ws, lay.a);
    R->sb = side_at(ws, lay.b);
    const Side &sa = R->sa, &sb = R->sb;
    A.lat_c = B.lat_c = lat_c;
    A.lon_c = B.lon_c = lon_c;

    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[0], stream));
    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, kBackWords * 8, stream));
    REMAP_TRY(launch(bucket_edges, A.n_lon + 1, kBlock, stream, A.n_lat,
                     A.n_lon, lat_c, lon_c));
    void *temp0 = ws + lay.temp0;
    REMAP_TRY(prep_side(B, true, sb, b_area, temp0, lay.temp0_bytes, back,
                        status_ab + 1, stream));
    REMAP_TRY(prep_side(A, false, sa, a_area, temp0, lay.temp0_bytes,
                        back + 1, status_ab, stream));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[1], stream));
    // read-back 1: the bucket keys of both meshes, the cells' error bits
    int64_t got[3];
    REMAP_TRY(read_back(got, back, sizeof(got), stream));
    const int64_t n_bkeys = got[0], n_akeys = got[1];
    const int err_a = static_cast<int>(got[2] & 0xffffffff);
    const int err_b = static_cast<int>((got[2] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return route_fail(route, err_a, err_b, 0);
    if (n_bkeys >= (int64_t(1) << 32) - 1 || n_akeys >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED, "%s: %lld / %lld bucket keys", who,
                    static_cast<long long>(n_akeys),
                    static_cast<long long>(n_bkeys));
    if (n_pairs > 0 && n_akeys == 0)
        return route_fail(route, 0, 0, REMAP_OVERLAP_ERR_CAPACITY);
    REMAP_TRY(mesh_var_layout(n_akeys, n_bkeys, n_pairs, &lay));
    if (workspace_bytes < lay.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need %zu", who,
                    workspace_bytes, lay.total);
    uint64_t *bkeys = at<uint64_t>(ws, lay.bkeys);
    uint64_t *bkeys_s = at<uint64_t>(ws, lay.bkeys_s);
    uint64_t *akeys = at<uint64_t>(ws, lay.akeys);
    uint64_t *pcnt = at<uint64_t>(ws, lay.pcnt);
    uint64_t *poff = at<uint64_t>(ws, lay.poff);
    void *temp = ws + lay.temp;
    R->work = pair_work(ws, lay.pairs, back + 3, temp, lay.temp_bytes);
    const PairWork &w = R->work;

    // b's bucket lists
    if (n_bkeys > 0) {
        REMAP_TRY(launch(fill_pairs<true>, B.n_cells, kBlock, stream, B,
                         sb.boxes, sb.offs, n_bkeys, bkeys, w.status));
        REMAP_TRY(radix_sort_keys(temp, lay.temp_bytes, bkeys, bkeys_s,
                                  n_bkeys, stream));
    }
    REMAP_TRY(launch(bucket_starts, n_buckets + 1, kBlock, stream, n_buckets,
                     n_bkeys, bkeys_s, start));
    // a's (cell, bucket) keys, expanded to (a, b) candidates
    if (n_akeys > 0) {
        REMAP_TRY(launch(fill_pairs<false>, A.n_cells, kBlock, stream, A,
                         sa.boxes, sa.offs, n_akeys, akeys, w.status));
        REMAP_TRY(launch(pair_counts, n_akeys, kBlock, stream, n_akeys,
                         n_buckets, akeys, start, pcnt));
        REMAP_TRY(exclusive_scan(temp, lay.temp_bytes, pcnt, poff, n_akeys,
                                 stream));
        REMAP_TRY(launch(expand_pairs, n_akeys, kBlock, stream, n_akeys,
                         n_buckets, akeys, pcnt, poff, start, bkeys_s, n_pairs,
                         w.cand, w.status));
    }
    if (n_pairs > 0) {
        REMAP_TRY(radix_sort_keys(temp, lay.temp_bytes, w.cand, w.cand_s,
                                  n_pairs, stream));
        // the unique pairs into cand, the rest of it ~0 (no pair)
        REMAP_HIP_CHECK(hipMemsetAsync(w.cand, 0xff, n_pairs * 8, stream));
        REMAP_TRY(unique(temp, lay.temp_bytes, w.cand_s, w.cand, w.n_unique,
                         n_pairs, stream));
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[2], stream));
    return REMAP_OK;
}

int meshes(const remap_overlap_mesh *mesh_a, const remap_overlap_mesh *mesh_b,
           int32_t dst_is_b, int64_t n_pairs, void *workspace,
           size_t workspace_bytes, const Outputs &out, hipStream_t stream)
{
    MeshRun R;
    REMAP_TRY(mesh_front(kMeshes, mesh_a, mesh_b, n_pairs, workspace,
                         workspace_bytes, out, out.a_area, out.b_area, stream,
                         nullptr, &R));
    const bool dst_is_a = dst_is_b == 0;
    REMAP_TRY(clip_poly(R.A, R.sa, R.B, R.sb, n_pairs, R.work, stream));
    REMAP_TRY(keep_pairs(n_pairs, R.A.n_cells, R.B.n_cells, dst_is_a, R.work,
                         out.a_area, out.b_area, stream));
    // read-back 2: how many entries to sort, the pairs' error bits
    int64_t kept[2];
    REMAP_TRY(read_back(kept, R.work.n_kept, 16, stream));
    if (const int err = static_cast<int>(kept[1] & 0xffffffff))
        return route_fail(kMeshes, 0, 0, err);
    *out.n_entries = kept[0];
    return sort_and_sum(dst_is_a ? R.A.n_cells : R.B.n_cells, kept[0], n_pairs,
                        R.work, out, dst_is_a ? out.a_area : out.b_area,
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
    const size_t n = at_least_one(n_pairs);
    REMAP_TRY(sort_pairs_temp<uint32_t>(n, &L->temp_bytes));
    size_t off = 0;
    L->a_area = take(&off, at_least_one(n_a) * 8);
    L->b_area = take(&off, at_least_one(n_b) * 8);
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
    REMAP_TRY(check_pieces(a, "a"));
    REMAP_TRY(check_pieces(b, "b"));
    REMAP_TRY(meshes_sizes(kPieces, &a->mesh, &b->mesh, counter, n_pairs_out,
                           bytes_out, stream));
    PiecesLayout X;
    REMAP_TRY(pieces_layout(a->mesh.n_cells, b->mesh.n_cells, *n_pairs_out,
                            &X));
    *bytes_out += X.total;
    return REMAP_OK;
}

// ev (6 events, or NULL) marks the phases: cell preparation, candidate pairs,
// clip (with its compaction), sort, merge (with frac_b)
int pieces(const PiecesArg *pa, const PiecesArg *pb, int32_t dst_is_b,
           int64_t n_pairs, void *workspace, size_t workspace_bytes,
           const Outputs &out, hipStream_t stream, hipEvent_t *ev)
{
    const char *who = kPieces.who;
    REMAP_TRY(check_pieces(pa, "a"));
    REMAP_TRY(check_pieces(pb, "b"));
    const int64_t n_a = pa->mesh.n_cells, n_b = pb->mesh.n_cells;
    PiecesLayout X;
    REMAP_TRY(pieces_layout(n_a, n_b, n_pairs, &X));
    if (!workspace || workspace_bytes < X.total)
        return fail(REMAP_ERR_WORKSPACE,
                    "%s: workspace of %zu bytes, need more than %zu", who,
                    workspace_bytes, X.total);
    char *ws = static_cast<char *>(workspace);
    double *piece_area_a = at<double>(ws, X.a_area);
    double *piece_area_b = at<double>(ws, X.b_area);
    uint32_t *at_c = at<uint32_t>(ws, X.at_c);
    uint32_t *at_s = at<uint32_t>(ws, X.at_s);
    uint64_t *pieces_c = at<uint64_t>(ws, X.pieces_c);
    int64_t *back = at<int64_t>(ws, X.back);
    int32_t *status_ab = as<int32_t>(back + 1);

    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, 16, stream));
    // the parents first (a read-back of their own, none with identity
    // parents): an argument error comes before any geometry
    if ((pa->parent && n_a > 0) || (pb->parent && n_b > 0)) {
        REMAP_TRY(launch(check_parents, pa->parent ? n_a : 0, kBlock, stream,
                         n_a, pa->n_parents, pa->parent, status_ab));
        REMAP_TRY(launch(check_parents, pb->parent ? n_b : 0, kBlock, stream,
                         n_b, pb->n_parents, pb->parent, status_ab + 1));
        int32_t bad[2];
        REMAP_TRY(read_back(bad, status_ab, 8, stream));
        if (bad[0] || bad[1])
            return fail(REMAP_ERR_ARG, "%s: parent of side %s %s", who,
                        bad[0] ? "a" : "b",
                        ((bad[0] ? bad[0] : bad[1]) & kErrParentOrder)
                            ? "decreases or is outside [0, n_parents)"
                            : "skips a cell: a cell without a piece");
    }
    MeshRun R;
    REMAP_TRY(mesh_front(kPieces, &pa->mesh, &pb->mesh, n_pairs, ws + X.total,
                         workspace_bytes - X.total, out, piece_area_a,
                         piece_area_b, stream, ev, &R));
    REMAP_TRY(launch(parent_areas, pa->n_parents, kBlock, stream, n_a,
                     pa->n_parents, pa->parent, piece_area_a, out.a_area));
    REMAP_TRY(launch(parent_areas, pb->n_parents, kBlock, stream, n_b,
                     pb->n_parents, pb->parent, piece_area_b, out.b_area));
    const bool dst_is_a = dst_is_b == 0;
    const PairWork &w = R.work;
    REMAP_TRY(clip_poly(R.A, R.sa, R.B, R.sb, n_pairs, w, stream));
    if (n_pairs > 0) {
        REMAP_TRY(launch(flag_positive, n_pairs, kBlock, stream, n_pairs, n_a,
                         n_b, w.cand, w.parea, w.head));
        REMAP_TRY(exclusive_scan(w.temp, w.temp_bytes, w.head, w.slot, n_pairs,
                                 stream));
        REMAP_TRY(launch(scatter_parents, n_pairs, kBlock, stream, n_pairs,
                         dst_is_a, w.cand, w.parea, w.head, w.slot, pa->parent,
                         pb->parent, w.cand_s, at_c, w.area_c, pieces_c,
                         w.n_kept));
    }
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[3], stream));
    // read-back 2: how many piece pairs to sort, the pairs' error bits
    int64_t kept[2];
    REMAP_TRY(read_back(kept, w.n_kept, 16, stream));
    const int64_t n_kept = kept[0];
    if (const int err = static_cast<int>(kept[1] & 0xffffffff))
        return route_fail(kPieces, 0, 0, err);
    const double *dst_area = dst_is_a ? out.a_area : out.b_area;
    const int64_t n_dst = dst_is_a ? pa->n_parents : pb->n_parents;
    // (w.cand is the sort's key output, w.parea the runs' sums)
    if (n_kept > 0)
        REMAP_TRY(radix_sort_pairs(ws + X.temp, X.temp_bytes, w.cand_s, w.cand,
                                   at_c, at_s, n_kept, stream));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[4], stream));
    int64_t n_entries = 0;
    if (n_kept > 0) {
        REMAP_TRY(launch(merge_runs, n_kept, kBlock, stream, n_kept, w.cand,
                         at_s, w.area_c, pieces_c, dst_area, w.parea, w.head));
        REMAP_TRY(exclusive_scan(w.temp, w.temp_bytes, w.head, w.slot, n_kept,
                                 stream));
        REMAP_TRY(launch(scatter_entries, n_kept, kBlock, stream, n_kept,
                         w.cand, w.parea, w.head, w.slot, out.dst, out.src,
                         out.area, back));
        // read-back 3: the entries the sliver rule left
        REMAP_TRY(read_back(&n_entries, back, 8, stream));
    }
    *out.n_entries = n_entries;
    REMAP_TRY(launch(dst_sums, n_dst, kBlock, stream, n_dst, back, out.dst,
                     out.area, dst_area, out.frac_b));
    if (ev)
        REMAP_HIP_CHECK(hipEventRecord(ev[5], stream));
    return REMAP_OK;
}

int pieces_timed(const PiecesArg *pa, const PiecesArg *pb, int32_t dst_is_b,
                 int64_t n_pairs, void *workspace, size_t workspace_bytes,
                 const Outputs &out, float *phase_ms, hipStream_t stream)
{
    if (!phase_ms)
        return fail(REMAP_ERR_ARG, "remap_overlap_pieces_timed: NULL phase_ms");
    return timed_phases<6>(phase_ms, [&](hipEvent_t *ev) {
        return pieces(pa, pb, dst_is_b, n_pairs, workspace, workspace_bytes,
                      out, stream, ev);
    });
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
//   clip_pairs_poly, keep_pairs, sort_and_sum as above
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
    REMAP_TRY(mesh_fixed_layout(A.G, B.G, &L->m));
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
    REMAP_TRY(launch(quad_prep, S.G.n_cells, kPrepBlock, stream, S.Q, s.xyz,
                     s.nv, s.centre, area, status));
    return launch(cell_shape, S.G.n_cells, kBlock, stream, S.G.n_cells,
                  S.G.max_edges, clipper, s.xyz, s.nv, s.centre, s.radius,
                  status);
}

// both sides prepared, the pyramid, the count pass and its scan: the number
// of candidates in back[3], the sides' error bits in back[2], the walker's
// counts / offs ready for the fill pass.  The areas go to a_area / b_area.
int grid_candidates(GridSide &A, GridSide &B, const GridLayout &L, char *ws,
                    double *a_area, double *b_area, Pyramid *pyramid,
                    hipStream_t stream)
{
    const MeshLayout &lay = L.m;
    double *lat_c = at<double>(ws, lay.lat_c);
    double *lon_c = at<double>(ws, lay.lon_c);
    int64_t *back = at<int64_t>(ws, lay.back);
    int32_t *status_ab = as<int32_t>(back + 2);
    void *temp0 = ws + lay.temp0;
    A.G.lat_c = B.G.lat_c = lat_c;
    A.G.lon_c = B.G.lon_c = lon_c;
    REMAP_HIP_CHECK(hipMemsetAsync(back, 0, kBackWords * 8, stream));
    REMAP_TRY(launch(bucket_edges, 1, kBlock, stream, 1, 1, lat_c, lon_c));
    for (int k = 0; k < 2; ++k) {
        const GridSide &S = k ? A : B;
        const Side s = side_at(ws, k ? lay.a : lay.b);
        double *area = k ? a_area : b_area;
        int32_t *status = k ? status_ab : status_ab + 1;
        REMAP_TRY(S.is_grid
                      ? prep_grid_side(S, k == 0, s, area, status, stream)
                      : prep_side(S.G, k == 0, s, area, temp0,
                                  lay.temp0_bytes, back + k, status, stream));
    }
    const Side si = side_at(ws, L.index == &A ? lay.a : lay.b);
    const Side sw = side_at(ws, L.walker == &A ? lay.a : lay.b);
    const GridGeom &Q = L.index->Q;
    int64_t *first = at<int64_t>(ws, L.first);
    const Pyramid P = {L.levels, Q.ny, Q.nx, si.centre, si.radius,
                       at<double>(ws, L.nodes), first};
    *pyramid = P;
    REMAP_TRY(launch(pyramid_table, 1, kWave, stream, Q.ny, Q.nx, L.levels,
                     first));
    for (int l = 1; l < L.levels; ++l)
        REMAP_TRY(launch(pyramid_level,
                         level_dim(Q.ny, l) * level_dim(Q.nx, l), kBlock,
                         stream, P, l));
    const int64_t n_w = L.walker->G.n_cells;
    if (n_w > 0) {
        REMAP_TRY(launch(pyramid_walk<false>, n_w, kWalkBlock, stream, P, n_w,
                         sw.centre, sw.radius, sw.nv, L.walker == &A,
                         sw.counts, nullptr, 0, nullptr, status_ab));
        REMAP_TRY(exclusive_scan(temp0, lay.temp0_bytes, sw.counts, sw.offs,
                                 n_w, stream));
        REMAP_TRY(launch(scan_total, 1, kWave, stream, n_w, sw.counts, sw.offs,
                         back + 3));
    }
    return REMAP_OK;
}

int check_sides(const remap_overlap_side *a, const remap_overlap_side *b,
                GridSide *A, GridSide *B)
{
    REMAP_TRY(check_side(a, "a", A));
    REMAP_TRY(check_side(b, "b", B));
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
    REMAP_TRY(check_sides(side_a, side_b, &A, &B));
    if (!n_pairs_out || !bytes_out)
        return fail(REMAP_ERR_ARG, "remap_overlap_grids_sizes: NULL output");
    GridLayout L;
    REMAP_TRY(grid_fixed_layout(A, B, &L));
    // the count pass needs both sides prepared: in memory of its own, with
    // the two area arrays behind it
    size_t bytes = L.m.fixed;
    const size_t at_a = take(&bytes, at_least_one(A.G.n_cells) * 8);
    const size_t at_b = take(&bytes, at_least_one(B.G.n_cells) * 8);
    char *buf = nullptr;
    REMAP_HIP_CHECK(hipMalloc(&buf, bytes));
    Pyramid P;
    int64_t got[2] = {0, 0};
    int rc = grid_candidates(A, B, L, buf, at<double>(buf, at_a),
                             at<double>(buf, at_b), &P, stream);
    if (rc == REMAP_OK)
        rc = read_back(got, buf + L.m.back + 16, sizeof(got), stream);
    else
        (void)hipStreamSynchronize(stream);
    const hipError_t freed = hipFree(buf);
    REMAP_TRY(rc);
    REMAP_HIP_CHECK(freed);
    const int err_a = static_cast<int>(got[0] & 0xffffffff);
    const int err_b = static_cast<int>((got[0] >> 32) & 0xffffffff);
    if (err_a || err_b)
        return route_fail(kGrids, err_a, err_b, 0);
    if (got[1] >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_overlap_grids: %lld candidate pairs",
                    static_cast<long long>(got[1]));
    REMAP_TRY(mesh_var_layout(0, 0, got[1], &L.m));
    *n_pairs_out = got[1];
    *bytes_out = L.m.total;
    return REMAP_OK;
}

int grids(const remap_overlap_side *side_a, const remap_overlap_side *side_b,
          int32_t dst_is_b, int64_t n_pairs, void *workspace,
          size_t workspace_bytes, const Outputs &out, hipStream_t stream)
{
    GridSide A, B;
    REMAP_TRY(check_sides(side_a, side_b, &A, &B));
    REMAP_TRY(check_call(kGrids.who, n_pairs, out));
    GridLayout L;
    REMAP_TRY(grid_fixed_layout(A, B, &L));
    REMAP_TRY(mesh_var_layout(0, 0, n_pairs, &L.m));
    const MeshLayout &lay = L.m;
    REMAP_TRY(need_workspace("remap_overlap_grids", workspace,
                             workspace_bytes, lay.total));
    char *ws = static_cast<char *>(workspace);
    Pyramid P;
    REMAP_TRY(grid_candidates(A, B, L, ws, out.a_area, out.b_area, &P,
                              stream));
    int64_t *back = at<int64_t>(ws, lay.back);
    const Side sa = side_at(ws, lay.a), sb = side_at(ws, lay.b);
    const Side sw = L.walker == &A ? sa : sb;
    const PairWork work = pair_work(ws, lay.pairs, back + 3, ws + lay.temp,
                                    lay.temp_bytes);
    const bool dst_is_a = dst_is_b == 0;
    const int64_t n_w = L.walker->G.n_cells;
    // (with n_pairs 0 it only checks that there are none)
    REMAP_TRY(launch(pyramid_walk<true>, n_w, kWalkBlock, stream, P, n_w,
                     sw.centre, sw.radius, sw.nv, L.walker == &A, sw.counts,
                     sw.offs, n_pairs, work.cand, work.status));
    REMAP_TRY(clip_poly(A.G, sa, B.G, sb, n_pairs, work, stream));
    REMAP_TRY(keep_pairs(n_pairs, A.G.n_cells, B.G.n_cells, dst_is_a, work,
                         out.a_area, out.b_area, stream));
    // the one read-back: the sides' error bits, the candidates, how many
    // entries to sort, the pairs' error bits
    int64_t got[4];
    REMAP_TRY(read_back(got, back + 2, sizeof(got), stream));
    const int err_a = static_cast<int>(got[0] & 0xffffffff);
    const int err_b = static_cast<int>((got[0] >> 32) & 0xffffffff);
    int err_p = static_cast<int>(got[3] & 0xffffffff);
    if (got[1] != n_pairs)
        err_p |= REMAP_OVERLAP_ERR_CAPACITY;
    if (err_a || err_b || err_p)
        return route_fail(kGrids, err_a, err_b, err_p);
    *out.n_entries = got[2];
    return sort_and_sum(dst_is_a ? A.G.n_cells : B.G.n_cells, got[2], n_pairs,
                        work, out, dst_is_a ? out.a_area : out.b_area, stream);
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

// (the mesh is side a, the grid side b)
int remap_overlap_latlon(const remap_overlap_geom *geom, int32_t dst_is_mesh,
                         int64_t n_pairs, void *workspace,
                         size_t workspace_bytes, int32_t *dst_out,
                         int32_t *src_out, double *area_out,
                         double *frac_b_out, double *mesh_area_out,
                         double *grid_area_out, int64_t *n_entries_out,
                         void *stream)
{
    return remap::overlap(geom, dst_is_mesh, n_pairs, workspace,
                          workspace_bytes,
                          {dst_out, src_out, area_out, frac_b_out,
                           mesh_area_out, grid_area_out, n_entries_out},
                          static_cast<hipStream_t>(stream));
}

int remap_overlap_meshes_sizes(const remap_overlap_mesh *a,
                               const remap_overlap_mesh *b, int64_t *counter,
                               int64_t *n_pairs_out,
                               size_t *workspace_bytes_out, void *stream)
{
    return remap::meshes_sizes(remap::kMeshes, a, b, counter, n_pairs_out,
                               workspace_bytes_out,
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
                         {dst_out, src_out, area_out, frac_b_out, a_area_out,
                          b_area_out, n_entries_out},
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
                         {dst_out, src_out, area_out, frac_b_out, a_area_out,
                          b_area_out, n_entries_out},
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
                               workspace_bytes,
                               {dst_out, src_out, area_out, frac_b_out,
                                a_area_out, b_area_out, n_entries_out},
                               phase_ms_out, static_cast<hipStream_t>(stream));
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
                        {dst_out, src_out, area_out, frac_b_out, a_area_out,
                         b_area_out, n_entries_out},
                        static_cast<hipStream_t>(stream));
}

}  // extern "C"
