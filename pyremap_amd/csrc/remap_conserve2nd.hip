// remap_conserve2nd.hip -- second-order conservative maps from the
// first-order overlaps: what a conserve2nd map needs beyond the areas A_ij.
//
//   remap_cell_moments       M = integral of r dA over every cell (SCRIP
//                            layout in, as remap_cell_areas takes it)
//   remap_overlap_moments    M_ij of (source cell j n destination cell i) for
//                            every first-order entry
//   remap_gradient_stencils  the coefficients G of a cell's gradient over its
//                            edge neighbours (Green's theorem over the
//                            neighbours' centroids)
//   remap_conserve2nd_sizes / remap_conserve2nd_assemble
//                            the triples (i, j, A_ij / A_i) and
//                            (i, k, G_jk . d_ij), sorted, equal (i, k) added
//
// The first moment of a great-circle polygon p_0 .. p_n-1 (counter-clockwise)
// is exact:  M = 1/2 sum_k theta_k n_k,  n_k = (p_k x p_k+1) / |p_k x p_k+1|,
// theta_k = atan2(|p_k x p_k+1|, p_k . p_k+1), added in ascending k (add_arc).
// p x q is evaluated as p x (q - p): the products are of the size of the edge,
// not of the unit vectors, so a short edge keeps its relative accuracy.
//
// The overlap polygon is clipped as clip_pairs_poly of remap_overlap.hip clips
// it (remap_clip.h: the same ring loading and edge clipping, the two ping-pong
// rings per lane in LDS), always the SOURCE cell by the destination cell's
// edges in the gnomonic plane of the source cell's centre; the clipped plane
// corners are lifted back to unit vectors for the moment.
//
// fp64 throughout, no floating-point atomics: equal (i, k) are regrouped with
// rocPRIM's stable radix_sort_pairs (the value is the emission position) and
// one lane adds a run up in that order, as remap_column_fractions does.  Two
// calls give the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_clip.h"
#include "remap_common.h"
#include "remap_host.h"
#include "remap_sphere.h"

namespace remap {
namespace {

constexpr int kCells = kWave;     // cells per block: one per lane of wave 0
constexpr int kMaxWidth = REMAP_CELL_AREAS_MAX_WIDTH;
// one clip by an edge of a convex clipper adds at most one vertex
constexpr int kMaxOutPoly = 2 * kMaxEdges;
// remap_overlap.hip's clip-overflow bit
constexpr int kErrClip = 16;
// status bits of this file beside REMAP_OVERLAP_ERR_*: a count outside
// [0, width]; an index (dst, src, nbr) outside its side; a triple count that
// differs from the capacity
constexpr int kErrCount = 1;
constexpr int kErrIndex = 64;
constexpr int kErrCapacity = 128;
constexpr uint64_t kLow = 0xffffffffull;

// m += 1/2 theta n of the arc p -> q; nothing for p == q (or antipodes)
__device__ inline void add_arc(V3 p, V3 q, V3 *m)
{
    const V3 c = cross(p, sub(q, p));
    const double s = sqrt(dot(c, c));
    if (!(s > 0.0))
        return;
    const double h = 0.5 * atan2(s, dot(p, q)) / s;
    m->x += h * c.x;
    m->y += h * c.y;
    m->z += h * c.z;
}

__device__ inline bool same(V3 a, V3 b)
{
    return a.x == b.x && a.y == b.y && a.z == b.z;
}

// consecutive equal corners and the closing copies of corner 0 dropped, in
// place: what is left of the first nc corners
__device__ inline int distinct_corners(Ring r, int nc)
{
    int nv = 0;
    for (int k = 0; k < nc; ++k) {
        const V3 p = r[k];
        if (nv > 0 && same(p, r[nv - 1]))
            continue;
        r.set(nv++, p);
    }
    while (nv > 1 && same(r[nv - 1], r[0]))
        --nv;
    return nv;
}

// staging as cell_areas_kernel: the block's 64 * width corner slots read by
// all lanes in slot order, unit vectors to LDS transposed; lane c of the first
// wave walks cell c's ring
__global__ __launch_bounds__(kBlock) void cell_moments_kernel(
    int64_t n_cells, int32_t width, const double *__restrict__ corner_lat,
    const double *__restrict__ corner_lon, const int32_t *__restrict__ count,
    double *__restrict__ moment_out, int32_t *__restrict__ status)
{
    extern __shared__ double lds[];
    double *sx = lds, *sy = sx + kCells * width, *sz = sy + kCells * width;
    const int64_t cell0 = (int64_t)blockIdx.x * kCells;
    const int64_t left = n_cells - cell0;
    const int cells = static_cast<int>(left < kCells ? left : kCells);
    const int slots = cells * width;
    const int64_t base = cell0 * width;
    for (int s = threadIdx.x; s < slots; s += kBlock) {
        const int c = s / width, k = s - c * width;
        const V3 p = unit_latlon(corner_lat[base + s], corner_lon[base + s]);
        sx[k * kCells + c] = p.x;
        sy[k * kCells + c] = p.y;
        sz[k * kCells + c] = p.z;
    }
    __syncthreads();
    const int lane = threadIdx.x;
    if (lane >= cells)
        return;
    const int64_t cell = cell0 + lane;
    const int32_t nc = count[cell];
    V3 m = {0.0, 0.0, 0.0};
    if (nc < 0 || nc > width) {
        atomicOr(&status[0], kErrCount);
        // (the LOWEST offending cell: the largest n_cells - cell)
        atomicMax(&status[1], static_cast<int32_t>(n_cells - cell));
    } else {
        const Ring r = {sx + lane, sy + lane, sz + lane, kCells};
        const int nv = distinct_corners(r, nc);
        if (nv >= 3) {
            V3 s = {0.0, 0.0, 0.0};
            V3 p = r[0];
            for (int k = 0; k < nv; ++k) {
                const V3 q = r[k + 1 < nv ? k + 1 : 0];
                add_arc(p, q, &m);
                s = {s.x + p.x, s.y + p.y, s.z + p.z};
                p = q;
            }
            // a clockwise ring: its moment points away from its corners
            if (dot(m, s) < 0.0)
                m = {-m.x, -m.y, -m.z};
        }
    }
    moment_out[cell * 3 + 0] = m.x;
    moment_out[cell * 3 + 1] = m.y;
    moment_out[cell * 3 + 2] = m.z;
}

// one lane per cell, SCRIP layout in: the ring the overlap calls prepare
// (finish_ring: distinct corners, turned counter-clockwise, the centre the
// normalised sum of the corners).  A cell with fewer than 3 distinct corners
// has nv 0.
__global__ __launch_bounds__(kClipBlock) void ring_prep(
    int64_t n_cells, int32_t width, const double *__restrict__ corner_lat,
    const double *__restrict__ corner_lon, const int32_t *__restrict__ count,
    bool need_convex, double *__restrict__ xyz, int32_t *__restrict__ nv_out,
    double *__restrict__ centre, int32_t *__restrict__ status)
{
    __shared__ double sx[kMaxEdges][kClipBlock], sy[kMaxEdges][kClipBlock],
        sz[kMaxEdges][kClipBlock];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kClipBlock + lane;
    if (c >= n_cells)
        return;
    const Ring r = {&sx[0][lane], &sy[0][lane], &sz[0][lane], kClipBlock};
    int32_t nc = count[c];
    if (nc < 0 || nc > width) {
        atomicOr(&status[0], kErrCount);
        atomicMax(&status[1], static_cast<int32_t>(n_cells - c));
        nc = 0;
    }
    for (int k = 0; k < nc; ++k)
        r.set(k, unit_latlon(corner_lat[c * width + k],
                             corner_lon[c * width + k]));
    int nv = distinct_corners(r, nc);
    V3 cc = {0.0, 0.0, 0.0};
    double area;
    if (finish_ring(r, &nv, &cc, &area) == 0 && need_convex &&
        !convex_cell(r, nv))
        atomicOr(&status[0], REMAP_OVERLAP_ERR_CONVEX);
    for (int k = 0; k < nv; ++k) {
        const V3 v = r[k];
        double *o = xyz + (c * width + k) * 3;
        o[0] = v.x;
        o[1] = v.y;
        o[2] = v.z;
    }
    nv_out[c] = nv;
    centre[c * 3 + 0] = cc.x;
    centre[c * 3 + 1] = cc.y;
    centre[c * 3 + 2] = cc.z;
}

// A_ij times the mean position M_j / A_j of the source cell: the moment of an
// overlap that has no polygon of its own (and what d_ij is measured from)
__device__ inline V3 mean_moment(double a, const double *src_area,
                                 const double *src_moment, int64_t j)
{
    const double aj = src_area[j];
    if (!(aj > 0.0))
        return {0.0, 0.0, 0.0};
    return {a * (src_moment[j * 3] / aj), a * (src_moment[j * 3 + 1] / aj),
            a * (src_moment[j * 3 + 2] / aj)};
}

// one lane per entry: source cell j by destination cell i's edges in the
// tangent plane of j's centre, as clip_pairs_poly; the moment of what is left
__global__ __launch_bounds__(kClipBlock) void overlap_moments_kernel(
    int64_t n_entries, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ src, const double *__restrict__ area,
    int64_t n_src, int32_t width_src, const double *__restrict__ xyz_src,
    const int32_t *__restrict__ nv_src, const double *__restrict__ centre_src,
    const double *__restrict__ src_area,
    const double *__restrict__ src_moment, int64_t n_dst, int32_t width_dst,
    const double *__restrict__ xyz_dst, const int32_t *__restrict__ nv_dst,
    double *__restrict__ moment_out, int32_t *__restrict__ status)
{
    __shared__ double px[2][kMaxOutPoly][kClipBlock];
    __shared__ double py[2][kMaxOutPoly][kClipBlock];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kClipBlock + lane;
    if (p >= n_entries)
        return;
    double *out = moment_out + p * 3;
    const int64_t i = dst[p], j = src[p];
    if (i < 0 || i >= n_dst || j < 0 || j >= n_src) {
        atomicOr(&status[0], kErrIndex);
        out[0] = out[1] = out[2] = 0.0;
        return;
    }
    V3 m = mean_moment(area[p], src_area, src_moment, j);
    const int na = nv_src[j], nb = nv_dst[i];
    int n = 0, cur = 0;
    const Tangent T = tangent_at({centre_src[j * 3], centre_src[j * 3 + 1],
                                  centre_src[j * 3 + 2]});
    if (na >= 3 && nb >= 3) {
        const CellRing vb = {xyz_dst + i * width_dst * 3};
        bool bad = !load_ring(T, xyz_src + j * width_src * 3, na, px, py,
                              lane);
        for (int k = 0; k < nb; ++k)
            bad |= !(dot(vb[k], T.cc) >= kMinCos);
        if (bad) {
            atomicOr(&status[0], REMAP_OVERLAP_ERR_HEMISPHERE);
            out[0] = out[1] = out[2] = 0.0;
            return;
        }
        double fx, fy, t;
        T.project(vb[0], &fx, &fy, &t);
        double ax = fx, ay = fy;
        n = na;
        for (int e = 0; e < nb && n > 0; ++e) {
            double bx = fx, by = fy;
            if (e + 1 < nb)
                T.project(vb[e + 1], &bx, &by, &t);
            const double dx = bx - ax, dy = by - ay;
            if (dx != 0.0 || dy != 0.0) {
                n = clip_edge(px, py, lane, cur, n, ax, ay, dx, dy);
                if (n > kMaxOutPoly) {
                    atomicOr(&status[0], kErrClip);
                    out[0] = out[1] = out[2] = 0.0;
                    return;
                }
                cur ^= 1;
            }
            ax = bx;
            ay = by;
        }
    }
    if (n >= 3) {
        const V3 cc = T.cc, e1 = T.e1, e2 = T.e2;
        auto lift = [&](int k) {
            const double x = px[cur][k][lane], y = py[cur][k][lane];
            return normalized(V3{cc.x + x * e1.x + y * e2.x,
                                 cc.y + x * e1.y + y * e2.y,
                                 cc.z + x * e1.z + y * e2.z});
        };
        const V3 first = lift(0);
        V3 a = first;
        m = {0.0, 0.0, 0.0};
        for (int k = 1; k <= n; ++k) {
            const V3 b = k < n ? lift(k) : first;
            add_arc(a, b, &m);
            a = b;
        }
    }
    out[0] = m.x;
    out[1] = m.y;
    out[2] = m.z;
}

// G - (G . c) c
__device__ inline V3 tangential(V3 g, V3 c)
{
    const double s = (g.x * c.x + g.y * c.y) + g.z * c.z;
    return {g.x - s * c.x, g.y - s * c.y, g.z - s * c.z};
}

// one lane per cell: Green's theorem with the trapezoid rule over the polygon
// of the neighbours' centroids.  e_t = -1/2 theta_t nu_t / A_N with A_N the
// SIGNED area of that polygon: turning a clockwise polygon round changes the
// sign of every nu_t and of A_N, so e_t is what the reversed order gives.
__global__ __launch_bounds__(kBlock) void gradient_stencils_kernel(
    int64_t n_cells, int32_t width, const int32_t *__restrict__ nbr,
    const int32_t *__restrict__ count, const double *__restrict__ centroid,
    double *__restrict__ coef_out, int32_t *__restrict__ has_out,
    int32_t *__restrict__ status)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_cells)
        return;
    double *out = coef_out + j * (width + 1) * 3;
    for (int k = 0; k < (width + 1) * 3; ++k)
        out[k] = 0.0;
    has_out[j] = 0;
    const int32_t nc = count[j];
    if (nc < 0 || nc > width) {
        atomicOr(&status[0], kErrCount);
        atomicMax(&status[1], static_cast<int32_t>(n_cells - j));
        return;
    }
    if (nc < 3)
        return;
    const int32_t *row = nbr + j * width;
    for (int t = 0; t < nc; ++t) {
        if (row[t] >= n_cells) {
            atomicOr(&status[0], kErrIndex);
            return;
        }
        if (row[t] < 0)
            return;
    }
    auto C = [&](int t) {
        const int64_t b = row[t];
        return V3{centroid[b * 3], centroid[b * 3 + 1], centroid[b * 3 + 2]};
    };
    double an = 0.0;
    {
        const V3 c0 = C(0);
        V3 prev = C(1);
        for (int t = 2; t < nc; ++t) {
            const V3 c = C(t);
            an += tri_area(c0, prev, c);
            prev = c;
        }
    }
    if (!(an != 0.0) || !isfinite(an))
        return;
    auto arc = [&](V3 a, V3 b) {
        const V3 c = cross(a, sub(b, a));
        const double s = sqrt(dot(c, c));
        if (!(s > 0.0))
            return V3{0.0, 0.0, 0.0};
        const double h = -0.5 * atan2(s, dot(a, b)) / (s * an);
        return V3{h * c.x, h * c.y, h * c.z};
    };
    const V3 cj = {centroid[j * 3], centroid[j * 3 + 1], centroid[j * 3 + 2]};
    V3 a = C(0);
    V3 e_prev = arc(C(nc - 1), a);
    V3 sum = {0.0, 0.0, 0.0};
    for (int t = 0; t < nc; ++t) {
        const V3 b = C(t + 1 < nc ? t + 1 : 0);
        const V3 e = arc(a, b);
        const V3 g = tangential({e_prev.x + e.x, e_prev.y + e.y,
                                 e_prev.z + e.z}, cj);
        out[(1 + t) * 3 + 0] = g.x;
        out[(1 + t) * 3 + 1] = g.y;
        out[(1 + t) * 3 + 2] = g.z;
        sum = {sum.x + e.x, sum.y + e.y, sum.z + e.z};
        e_prev = e;
        a = b;
    }
    const V3 g = tangential({-2.0 * sum.x, -2.0 * sum.y, -2.0 * sum.z}, cj);
    out[0] = g.x;
    out[1] = g.y;
    out[2] = g.z;
    has_out[j] = 1;
}

// ---------------------------------------------------------------------------
// the assembly
// ---------------------------------------------------------------------------

// triples of entry e: the first-order term, and with a gradient the cell
// itself and its neighbours; the block's sum to *total when one is given
__global__ __launch_bounds__(kBlock) void triple_counts(
    int64_t n_entries, int64_t n_src, int32_t width,
    const int32_t *__restrict__ src, const int32_t *__restrict__ count,
    const int32_t *__restrict__ has, uint32_t *__restrict__ cnt,
    unsigned long long *__restrict__ total, int64_t *__restrict__ status)
{
    __shared__ unsigned long long block_sum;
    if (threadIdx.x == 0)
        block_sum = 0ull;
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t c = 0;
    if (e < n_entries) {
        const int64_t j = src[e];
        if (j < 0 || j >= n_src) {
            atomicOr(reinterpret_cast<unsigned long long *>(status),
                     static_cast<unsigned long long>(kErrIndex));
        } else {
            c = 1;
            if (has[j]) {
                const int32_t nc = count[j];
                if (nc < 0 || nc > width)
                    atomicOr(reinterpret_cast<unsigned long long *>(status),
                             static_cast<unsigned long long>(kErrCount));
                else
                    c += 1 + static_cast<uint32_t>(nc);
            }
        }
        if (cnt)
            cnt[e] = c;
    }
    if (total) {
        if (c)
            atomicAdd(&block_sum, static_cast<unsigned long long>(c));
        __syncthreads();
        if (threadIdx.x == 0 && block_sum)
            atomicAdd(total, block_sum);
    }
}

__global__ __launch_bounds__(kBlock) void fill_triples(
    int64_t n_entries, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ src, const double *__restrict__ area,
    const double *__restrict__ moment, int64_t n_src, int32_t width,
    const int32_t *__restrict__ nbr, const double *__restrict__ coef,
    const double *__restrict__ src_area,
    const double *__restrict__ src_moment, int64_t n_dst,
    const double *__restrict__ dst_area, int64_t capacity,
    const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
    uint64_t *__restrict__ keys, uint32_t *__restrict__ pos,
    double *__restrict__ w, int64_t *__restrict__ status)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_entries)
        return;
    auto flag = [&](int bit) {
        atomicOr(reinterpret_cast<unsigned long long *>(status),
                 static_cast<unsigned long long>(bit));
    };
    const uint32_t c = cnt[e];
    const int64_t o = off[e];
    if (e == n_entries - 1 && o + c != capacity)
        flag(kErrCapacity);
    if (c == 0 || o + c > capacity)
        return;
    const int64_t i = dst[e], j = src[e];   // (j checked by triple_counts)
    if (i < 0 || i >= n_dst) {
        flag(kErrIndex);
        for (uint32_t k = 0; k < c; ++k) {
            keys[o + k] = ~uint64_t(0);
            pos[o + k] = static_cast<uint32_t>(o + k);
            w[o + k] = 0.0;
        }
        return;
    }
    const uint64_t hi = static_cast<uint64_t>(i) << 32;
    const double a = area[e], ai = dst_area[i];
    keys[o] = hi | static_cast<uint64_t>(j);
    pos[o] = static_cast<uint32_t>(o);
    w[o] = a / ai;
    if (c == 1)
        return;
    const V3 mean = mean_moment(a, src_area, src_moment, j);
    const double dx = (moment[e * 3] - mean.x) / ai;
    const double dy = (moment[e * 3 + 1] - mean.y) / ai;
    const double dz = (moment[e * 3 + 2] - mean.z) / ai;
    const double *g = coef + j * (width + 1) * 3;
    for (uint32_t k = 1; k < c; ++k) {
        int64_t col = j;
        if (k > 1) {
            col = nbr[j * width + (k - 2)];
            if (col < 0 || col >= n_src) {
                flag(kErrIndex);
                col = j;
            }
        }
        const double *gk = g + (k - 1) * 3;
        keys[o + k] = hi | static_cast<uint64_t>(col);
        pos[o + k] = static_cast<uint32_t>(o + k);
        w[o + k] = (gk[0] * dx + gk[1] * dy) + gk[2] * dz;
    }
}

// one lane per sorted triple; the first of a run of equal keys adds the run
// up in sorted order, which is emission order (the sort is stable)
__global__ __launch_bounds__(kBlock) void sum_runs(
    int64_t n, const uint64_t *__restrict__ keys,
    const uint32_t *__restrict__ pos, const double *__restrict__ w,
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
    // (a position is below n unless the capacity was wrong: kErrCapacity)
    auto at = [&](int64_t m) { return pos[m] < n ? w[pos[m]] : 0.0; };
    double s = at(i);
    for (int64_t m = i + 1; m < n && keys[m] == key; ++m)
        s = s + at(m);
    sums[i] = s;
    head[i] = 1u;
}

__global__ __launch_bounds__(kBlock) void scatter_triples(
    int64_t n, const uint64_t *__restrict__ keys,
    const double *__restrict__ sums, const uint32_t *__restrict__ head,
    const uint32_t *__restrict__ slot, int32_t *__restrict__ row,
    int32_t *__restrict__ col, double *__restrict__ s_out,
    int64_t *__restrict__ n_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    if (i == n - 1)
        *n_out = static_cast<int64_t>(slot[i]) + head[i];
    if (!head[i])
        return;
    const uint32_t s = slot[i];
    row[s] = static_cast<int32_t>(keys[i] >> 32);
    col[s] = static_cast<int32_t>(keys[i] & kLow);
    s_out[s] = sums[i];
}

struct MomentsLayout {
    size_t xyz_src, nv_src, centre_src, xyz_dst, nv_dst, centre_dst, total;
};

MomentsLayout moments_layout(int64_t n_src, int32_t width_src, int64_t n_dst,
                             int32_t width_dst)
{
    MomentsLayout lay;
    size_t off = 0;
    lay.xyz_src = take(&off, at_least_one(n_src) * width_src * 24);
    lay.nv_src = take(&off, at_least_one(n_src) * 4);
    lay.centre_src = take(&off, at_least_one(n_src) * 24);
    lay.xyz_dst = take(&off, at_least_one(n_dst) * width_dst * 24);
    lay.nv_dst = take(&off, at_least_one(n_dst) * 4);
    // (the destination's centres: written by ring_prep, read by nobody)
    lay.centre_dst = take(&off, at_least_one(n_dst) * 24);
    lay.total = off;
    return lay;
}

struct AssembleLayout {
    size_t cnt, off, keys_in, pos_in, w, keys_out, pos_out, head, slot, temp,
        total;
    size_t temp_bytes;
};

int assemble_layout(int64_t n_entries, int64_t capacity, AssembleLayout *lay)
{
    const size_t n = at_least_one(n_entries), cap = at_least_one(capacity);
    size_t scan_n = 0, scan_cap = 0, sort = 0;
    REMAP_TRY(scan_temp<uint32_t>(n, &scan_n));
    REMAP_TRY(scan_temp<uint32_t>(cap, &scan_cap));
    REMAP_TRY(sort_pairs_temp<uint32_t>(cap, &sort));
    lay->temp_bytes = scan_n > scan_cap ? scan_n : scan_cap;
    if (sort > lay->temp_bytes)
        lay->temp_bytes = sort;
    size_t off = 0;
    lay->cnt = take(&off, n * 4);
    lay->off = take(&off, n * 4);
    lay->keys_in = take(&off, cap * 8);   // later: the runs' sums
    lay->pos_in = take(&off, cap * 4);
    lay->w = take(&off, cap * 8);
    lay->keys_out = take(&off, cap * 8);
    lay->pos_out = take(&off, cap * 4);
    lay->head = take(&off, cap * 4);
    lay->slot = take(&off, cap * 4);
    lay->temp = take(&off, lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

int count_fail(const char *name, int32_t width, int64_t n_cells,
               const int32_t *err)
{
    return fail(REMAP_ERR_ARG,
                "%s: a count outside [0, %d], first at cell %lld", name, width,
                static_cast<long long>(n_cells) - err[1]);
}

int check_cells(const char *name, int64_t n_cells, int32_t width,
                int32_t max_width)
{
    if (n_cells < 0 || n_cells > INT32_MAX || width < 1)
        return fail(REMAP_ERR_ARG,
                    "%s: n_cells %lld, width %d: expected 0 <= n_cells < 2^31 "
                    "and width >= 1", name, static_cast<long long>(n_cells),
                    width);
    if (width > max_width)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "%s: width %d, this build serves up to %d corners a cell",
                    name, width, max_width);
    return REMAP_OK;
}

int check_assemble(const char *name, int64_t n_entries, int64_t n_src,
                   int32_t width)
{
    if (n_entries < 0 || n_entries > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_entries %lld: expected 0 <= "
                    "n_entries < 2^31", name,
                    static_cast<long long>(n_entries));
    return check_cells(name, n_src, width, kMaxEdges);
}

int status_fail(const char *name, int64_t bits)
{
    if (bits & kErrCount)
        return fail(REMAP_ERR_ARG, "%s: a count outside [0, width]", name);
    if (bits & kErrIndex)
        return fail(REMAP_ERR_ARG,
                    "%s: an entry or a neighbour names a cell outside its "
                    "side", name);
    return fail(REMAP_ERR_ARG,
                "%s: capacity differs from remap_conserve2nd_sizes' count",
                name);
}

}  // namespace

int cell_moments(int64_t n_cells, int32_t width, const double *corner_lat,
                 const double *corner_lon, const int32_t *count,
                 double *moment_out, int32_t *status, hipStream_t stream)
{
    const char *name = "remap_cell_moments";
    REMAP_TRY(check_cells(name, n_cells, width, kMaxWidth));
    if (!status)
        return fail(REMAP_ERR_ARG, "%s: NULL status", name);
    if (n_cells == 0)
        return REMAP_OK;
    if (!corner_lat || !corner_lon || !count || !moment_out)
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    const size_t lds_bytes = sizeof(double) * 3 * kCells * width;
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    REMAP_TRY(launch_blocks(cell_moments_kernel, blocks(n_cells, kCells),
                            kBlock, lds_bytes, stream, n_cells, width,
                            corner_lat, corner_lon, count, moment_out,
                            status));
    int32_t err[2] = {0, 0};
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0])
        return count_fail(name, width, n_cells, err);
    return REMAP_OK;
}

int overlap_moments_workspace(int64_t n_src, int32_t width_src, int64_t n_dst,
                              int32_t width_dst, size_t *bytes_out)
{
    const char *name = "remap_overlap_moments_workspace";
    if (!bytes_out)
        return fail(REMAP_ERR_ARG, "%s: NULL bytes_out", name);
    REMAP_TRY(check_cells(name, n_src, width_src, kMaxEdges));
    REMAP_TRY(check_cells(name, n_dst, width_dst, kMaxEdges));
    *bytes_out = moments_layout(n_src, width_src, n_dst, width_dst).total;
    return REMAP_OK;
}

int overlap_moments(int64_t n_entries, const int32_t *dst, const int32_t *src,
                    const double *area, int64_t n_src, int32_t width_src,
                    const double *src_lat, const double *src_lon,
                    const int32_t *src_count, const double *src_area,
                    const double *src_moment, int64_t n_dst,
                    int32_t width_dst, const double *dst_lat,
                    const double *dst_lon, const int32_t *dst_count,
                    double *moment_out, int32_t *status, void *workspace,
                    size_t workspace_bytes, hipStream_t stream)
{
    const char *name = "remap_overlap_moments";
    if (n_entries < 0 || n_entries > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_entries %lld: expected 0 <= "
                    "n_entries < 2^31", name,
                    static_cast<long long>(n_entries));
    REMAP_TRY(check_cells(name, n_src, width_src, kMaxEdges));
    REMAP_TRY(check_cells(name, n_dst, width_dst, kMaxEdges));
    if (!status)
        return fail(REMAP_ERR_ARG, "%s: NULL status", name);
    if (n_entries == 0)
        return REMAP_OK;
    if (!dst || !src || !area || !src_lat || !src_lon || !src_count ||
        !src_area || !src_moment || !dst_lat || !dst_lon || !dst_count ||
        !moment_out)
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    const MomentsLayout lay =
        moments_layout(n_src, width_src, n_dst, width_dst);
    REMAP_TRY(need_workspace(name, workspace, workspace_bytes, lay.total));
    char *ws = static_cast<char *>(workspace);
    double *xyz_src = at<double>(ws, lay.xyz_src);
    int32_t *nv_src = at<int32_t>(ws, lay.nv_src);
    double *centre_src = at<double>(ws, lay.centre_src);
    double *xyz_dst = at<double>(ws, lay.xyz_dst);
    int32_t *nv_dst = at<int32_t>(ws, lay.nv_dst);
    double *centre_dst = at<double>(ws, lay.centre_dst);
    int32_t err[2] = {0, 0};

    // the two sides' counts are checked one after the other, so that the
    // message can name the side
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    REMAP_TRY(launch(ring_prep, n_src, kClipBlock, stream, n_src, width_src,
                     src_lat, src_lon, src_count, false, xyz_src, nv_src,
                     centre_src, status));
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0] & kErrCount)
        return count_fail("remap_overlap_moments (source)", width_src, n_src,
                          err);
    REMAP_TRY(launch(ring_prep, n_dst, kClipBlock, stream, n_dst, width_dst,
                     dst_lat, dst_lon, dst_count, true, xyz_dst, nv_dst,
                     centre_dst, status));
    REMAP_TRY(launch(overlap_moments_kernel, n_entries, kClipBlock, stream,
                     n_entries, dst, src, area, n_src, width_src, xyz_src,
                     nv_src, centre_src, src_area, src_moment, n_dst,
                     width_dst, xyz_dst, nv_dst, moment_out, status));
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0] & kErrCount)
        return count_fail("remap_overlap_moments (destination)", width_dst,
                          n_dst, err);
    if (err[0] & kErrIndex)
        return fail(REMAP_ERR_ARG, "%s: an entry names a cell outside its "
                    "side (%lld destination, %lld source cells)", name,
                    static_cast<long long>(n_dst),
                    static_cast<long long>(n_src));
    if (err[0] & REMAP_OVERLAP_ERR_CONVEX)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "%s: a destination cell is not convex (status %d)", name,
                    err[0]);
    if (err[0] & REMAP_OVERLAP_ERR_HEMISPHERE)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "%s: an entry pairs cells too far apart for the "
                    "projection about the source cell's centre (status %d)",
                    name, err[0]);
    if (err[0] & kErrClip)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "%s: a clipped polygon outgrew %d corners (status %d)",
                    name, kMaxOutPoly, err[0]);
    return REMAP_OK;
}

int gradient_stencils(int64_t n_cells, int32_t width, const int32_t *nbr,
                      const int32_t *count, const double *centroid,
                      double *coef_out, int32_t *has_out, int32_t *status,
                      hipStream_t stream)
{
    const char *name = "remap_gradient_stencils";
    REMAP_TRY(check_cells(name, n_cells, width, kMaxEdges));
    if (!status)
        return fail(REMAP_ERR_ARG, "%s: NULL status", name);
    if (n_cells == 0)
        return REMAP_OK;
    if (!nbr || !count || !centroid || !coef_out || !has_out)
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    REMAP_TRY(launch(gradient_stencils_kernel, n_cells, kBlock, stream,
                     n_cells, width, nbr, count, centroid, coef_out, has_out,
                     status));
    int32_t err[2] = {0, 0};
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0] & kErrCount)
        return count_fail(name, width, n_cells, err);
    if (err[0] & kErrIndex)
        return fail(REMAP_ERR_ARG, "%s: a neighbour beyond the %lld cells",
                    name, static_cast<long long>(n_cells));
    return REMAP_OK;
}

int conserve2nd_sizes(int64_t n_entries, const int32_t *src, int64_t n_src,
                      int32_t width, const int32_t *count, const int32_t *has,
                      int64_t *counters, int64_t *capacity_out,
                      size_t *workspace_bytes_out, hipStream_t stream)
{
    const char *name = "remap_conserve2nd_sizes";
    REMAP_TRY(check_assemble(name, n_entries, n_src, width));
    if (!counters || !capacity_out || !workspace_bytes_out)
        return fail(REMAP_ERR_ARG, "%s: NULL counters or output", name);
    int64_t host[2] = {0, 0};
    if (n_entries > 0) {
        if (!src || !count || !has)
            return fail(REMAP_ERR_ARG, "%s: NULL array", name);
        REMAP_HIP_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(int64_t),
                                       stream));
        REMAP_TRY(launch(triple_counts, n_entries, kBlock, stream, n_entries,
                         n_src, width, src, count, has, nullptr,
                         as<unsigned long long>(counters), counters + 1));
        REMAP_TRY(read_back(host, counters, sizeof(host), stream));
        if (host[1])
            return status_fail(name, host[1]);
    }
    if (host[0] >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "%s: %lld triples, beyond 32-bit positions", name,
                    static_cast<long long>(host[0]));
    AssembleLayout lay;
    REMAP_TRY(assemble_layout(n_entries, host[0], &lay));
    *capacity_out = host[0];
    *workspace_bytes_out = lay.total;
    return REMAP_OK;
}

int conserve2nd_assemble(int64_t n_entries, const int32_t *dst,
                         const int32_t *src, const double *area,
                         const double *moment, int64_t n_src, int32_t width,
                         const int32_t *nbr, const int32_t *count,
                         const double *coef, const int32_t *has,
                         const double *src_area, const double *src_moment,
                         int64_t n_dst, const double *dst_area,
                         int64_t capacity, void *workspace,
                         size_t workspace_bytes, int32_t *row_out,
                         int32_t *col_out, double *s_out, int64_t *counters,
                         int64_t *n_out, hipStream_t stream)
{
    const char *name = "remap_conserve2nd_assemble";
    REMAP_TRY(check_assemble(name, n_entries, n_src, width));
    if (n_dst < 0 || n_dst > INT32_MAX || capacity < n_entries ||
        capacity >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_ARG, "%s: n_dst %lld, capacity %lld", name,
                    static_cast<long long>(n_dst),
                    static_cast<long long>(capacity));
    if (!counters || !n_out)
        return fail(REMAP_ERR_ARG, "%s: NULL counters or n_out", name);
    *n_out = 0;
    if (n_entries == 0)
        return REMAP_OK;
    if (!dst || !src || !area || !moment || !nbr || !count || !coef || !has ||
        !src_area || !src_moment || !dst_area || !row_out || !col_out ||
        !s_out)
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    AssembleLayout lay;
    REMAP_TRY(assemble_layout(n_entries, capacity, &lay));
    REMAP_TRY(need_workspace(name, workspace, workspace_bytes, lay.total));
    char *ws = static_cast<char *>(workspace);
    uint32_t *cnt = at<uint32_t>(ws, lay.cnt);
    uint32_t *off = at<uint32_t>(ws, lay.off);
    uint64_t *keys_in = at<uint64_t>(ws, lay.keys_in);
    // (keys_in is free once the sort has read it: the runs' sums go there)
    double *sums = at<double>(ws, lay.keys_in);
    uint32_t *pos_in = at<uint32_t>(ws, lay.pos_in);
    double *w = at<double>(ws, lay.w);
    uint64_t *keys_out = at<uint64_t>(ws, lay.keys_out);
    uint32_t *pos_out = at<uint32_t>(ws, lay.pos_out);
    uint32_t *head = at<uint32_t>(ws, lay.head);
    uint32_t *slot = at<uint32_t>(ws, lay.slot);
    void *temp = ws + lay.temp;

    REMAP_HIP_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(int64_t), stream));
    REMAP_TRY(launch(triple_counts, n_entries, kBlock, stream, n_entries,
                     n_src, width, src, count, has, cnt, nullptr,
                     counters + 1));
    REMAP_TRY(exclusive_scan(temp, lay.temp_bytes, cnt, off, n_entries,
                             stream));
    REMAP_TRY(launch(fill_triples, n_entries, kBlock, stream, n_entries, dst,
                     src, area, moment, n_src, width, nbr, coef, src_area,
                     src_moment, n_dst, dst_area, capacity, cnt, off, keys_in,
                     pos_in, w, counters + 1));
    // (a capacity that differs leaves slots unwritten: the status is read
    // with the count, and nothing below reads beyond the workspace)
    REMAP_TRY(radix_sort_pairs(temp, lay.temp_bytes, keys_in, keys_out,
                               pos_in, pos_out, capacity, stream));
    REMAP_TRY(launch(sum_runs, capacity, kBlock, stream, capacity, keys_out,
                     pos_out, w, sums, head));
    REMAP_TRY(exclusive_scan(temp, lay.temp_bytes, head, slot, capacity,
                             stream));
    REMAP_TRY(launch(scatter_triples, capacity, kBlock, stream, capacity,
                     keys_out, sums, head, slot, row_out, col_out, s_out,
                     counters));
    int64_t host[2] = {0, 0};
    REMAP_TRY(read_back(host, counters, sizeof(host), stream));
    if (host[1])
        return status_fail(name, host[1]);
    *n_out = host[0];
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_cell_moments(int64_t n_cells, int32_t width,
                       const double *corner_lat, const double *corner_lon,
                       const int32_t *count, double *moment_out,
                       int32_t *status, void *stream)
{
    return remap::cell_moments(n_cells, width, corner_lat, corner_lon, count,
                               moment_out, status,
                               static_cast<hipStream_t>(stream));
}

int remap_overlap_moments_workspace(int64_t n_src, int32_t width_src,
                                    int64_t n_dst, int32_t width_dst,
                                    size_t *bytes_out)
{
    return remap::overlap_moments_workspace(n_src, width_src, n_dst,
                                            width_dst, bytes_out);
}

int remap_overlap_moments(int64_t n_entries, const int32_t *dst,
                          const int32_t *src, const double *area,
                          int64_t n_src, int32_t width_src,
                          const double *src_lat, const double *src_lon,
                          const int32_t *src_count, const double *src_area,
                          const double *src_moment, int64_t n_dst,
                          int32_t width_dst, const double *dst_lat,
                          const double *dst_lon, const int32_t *dst_count,
                          double *moment_out, int32_t *status,
                          void *workspace, size_t workspace_bytes,
                          void *stream)
{
    return remap::overlap_moments(
        n_entries, dst, src, area, n_src, width_src, src_lat, src_lon,
        src_count, src_area, src_moment, n_dst, width_dst, dst_lat, dst_lon,
        dst_count, moment_out, status, workspace, workspace_bytes,
        static_cast<hipStream_t>(stream));
}

int remap_gradient_stencils(int64_t n_cells, int32_t width,
                            const int32_t *nbr, const int32_t *count,
                            const double *centroid, double *coef_out,
                            int32_t *has_out, int32_t *status, void *stream)
{
    return remap::gradient_stencils(n_cells, width, nbr, count, centroid,
                                    coef_out, has_out, status,
                                    static_cast<hipStream_t>(stream));
}

int remap_conserve2nd_sizes(int64_t n_entries, const int32_t *src,
                            int64_t n_src, int32_t width,
                            const int32_t *count, const int32_t *has,
                            int64_t *counters, int64_t *capacity_out,
                            size_t *workspace_bytes_out, void *stream)
{
    return remap::conserve2nd_sizes(n_entries, src, n_src, width, count, has,
                                    counters, capacity_out,
                                    workspace_bytes_out,
                                    static_cast<hipStream_t>(stream));
}

int remap_conserve2nd_assemble(int64_t n_entries, const int32_t *dst,
                               const int32_t *src, const double *area,
                               const double *moment, int64_t n_src,
                               int32_t width, const int32_t *nbr,
                               const int32_t *count, const double *coef,
                               const int32_t *has, const double *src_area,
                               const double *src_moment, int64_t n_dst,
                               const double *dst_area, int64_t capacity,
                               void *workspace, size_t workspace_bytes,
                               int32_t *row_out, int32_t *col_out,
                               double *s_out, int64_t *counters,
                               int64_t *n_out, void *stream)
{
    return remap::conserve2nd_assemble(
        n_entries, dst, src, area, moment, n_src, width, nbr, count, coef,
        has, src_area, src_moment, n_dst, dst_area, capacity, workspace,
        workspace_bytes, row_out, col_out, s_out, counters, n_out,
        static_cast<hipStream_t>(stream));
}

}  // extern "C"
