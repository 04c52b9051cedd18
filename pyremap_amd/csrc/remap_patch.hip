// remap_patch.hip -- patch-recovery maps (method 'patch') from the triangles
// of an MPAS mesh's dual: what a patch map needs beyond the point location
// of remap_locate.hip.
//
//   remap_node_rings       the one-ring of every node: the distinct nodes
//                          that share a triangle with it, ascending
//   remap_patch_fits       a least-squares quadratic per node over itself and
//                          its ring: h and the upper triangle of N^-1
//   remap_patch_sizes / remap_patch_rows
//                          per located point the blend of its triangle's three
//                          quadratics by the located weights, as a map row
//
// The frame of a node c is tangent_at of remap_clip.h; a member r has the
// gnomonic coordinates x = (r . e1) / (r . c), y = (r . e2) / (r . c), scaled
// by h, the largest radius of the node's members; phi = (1, x, y, x^2, xy,
// y^2), N = sum phi phi^T over the members (the node, then its ring).
//
// A row is written in one walk: the three member lists of a point's triangle
// (each a node and its ascending ring) are merged by column, so the columns
// come out ascending, every column's contributions are added in emission
// order (t ascending; a column is in a member list at most once) and no
// per-lane list is kept.  Pass 1 (sizes) is the same walk without the values;
// an exclusive scan of the counts gives every row its place, so the output is
// sorted by (row, col) without a global sort.  The members' phi are
// re-projected from xyz: a node stores 22 doubles, not its design matrix.
//
// fp64 throughout, no floating-point atomics, every call on the caller's
// stream; two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_clip.h"
#include "remap_common.h"
#include "remap_host.h"
#include "remap_sphere.h"

namespace remap {
namespace {

constexpr int kRing = REMAP_PATCH_MAX_RING;
constexpr int kFit = REMAP_PATCH_FIT_WIDTH;    // h, 21 of N^-1
constexpr int kMinMembers = 6;
constexpr double kPatchMinCos = 0.5;
// (1e-8 admitted fits singular to eight digits on edge and vertex meshes:
// DESIGN section 18 has the sweep)
constexpr double kPivot = 1e-2;
// status bits: a node id outside [0, n_nodes) (tri, ring); a triangle id
// outside [-1, n_tri) (found); offsets that are not remap_patch_sizes' for
// these arrays
constexpr int kErrIndex = 1;
constexpr int kErrFound = 2;
constexpr int kErrCapacity = 4;
constexpr int32_t kNone = INT32_MAX;

__device__ inline V3 node_at(const double *xyz, int64_t v)
{
    return {xyz[v * 3], xyz[v * 3 + 1], xyz[v * 3 + 2]};
}

// phi . g at (x, y), the terms added in the order of phi
__device__ inline double basis_dot(const double *g, double x, double y)
{
    double s = g[0];
    s = s + g[1] * x;
    s = s + g[2] * y;
    s = s + g[3] * (x * x);
    s = s + g[4] * (x * y);
    s = s + g[5] * (y * y);
    return s;
}

// ---------------------------------------------------------------------------
// rings
// ---------------------------------------------------------------------------

// the six directed pairs (a, b) of every triangle, keyed a << 32 | b; a
// triangle with a node outside the mesh emits the highest key six times
__global__ __launch_bounds__(kBlock) void ring_pairs(
    int64_t n_tri, const int32_t *__restrict__ tri, int64_t n_nodes,
    uint64_t *__restrict__ keys, int32_t *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tri)
        return;
    const int64_t v[3] = {tri[t * 3], tri[t * 3 + 1], tri[t * 3 + 2]};
    uint64_t *out = keys + t * 6;
    bool ok = true;
    for (int k = 0; k < 3; ++k)
        ok &= v[k] >= 0 && v[k] < n_nodes;
    if (!ok) {
        atomicOr(&status[0], kErrIndex);
        for (int k = 0; k < 6; ++k)
            out[k] = ~uint64_t(0);
        return;
    }
    int k = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            if (a != b)
                out[k++] = static_cast<uint64_t>(v[a]) << 32 |
                    static_cast<uint64_t>(v[b]);
}

// head[i] = 1 for the first of a run of equal keys (a, b) with a != b
__global__ __launch_bounds__(kBlock) void ring_heads(
    int64_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t key = keys[i];
    const bool fresh = i == 0 || keys[i - 1] != key;
    head[i] = fresh && key != ~uint64_t(0) &&
        (key >> 32) != (key & 0xffffffffull);
}

// rank[i]: the heads before i.  The first key of node a leaves its rank in
// first[a]
__global__ __launch_bounds__(kBlock) void ring_firsts(
    int64_t n, const uint64_t *__restrict__ keys,
    const uint32_t *__restrict__ rank, int64_t n_nodes,
    uint32_t *__restrict__ first)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t a = keys[i] >> 32;
    if (a >= static_cast<uint64_t>(n_nodes))
        return;
    if (i == 0 || (keys[i - 1] >> 32) != a)
        first[a] = rank[i];
}

// every head to its slot of ring[a] (the lowest kRing are kept); the last
// key of node a writes count[a]
__global__ __launch_bounds__(kBlock) void ring_fill(
    int64_t n, const uint64_t *__restrict__ keys,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank,
    const uint32_t *__restrict__ first, int64_t n_nodes,
    int32_t *__restrict__ ring, int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t key = keys[i];
    const uint64_t a = key >> 32;
    if (a >= static_cast<uint64_t>(n_nodes))
        return;
    const uint32_t slot = rank[i] - first[a];
    if (head[i] && slot < static_cast<uint32_t>(kRing))
        ring[a * kRing + slot] = static_cast<int32_t>(key & 0xffffffffull);
    if (i == n - 1 || (keys[i + 1] >> 32) != a)
        count[a] = static_cast<int32_t>(slot + head[i]);
}

// ---------------------------------------------------------------------------
// fits
// ---------------------------------------------------------------------------

// member m of node v: m = 0 the node itself, 1 + k slot k of its ring; -1
// where the slot is empty, *err set where it names no node
__device__ inline int64_t member_of(const int32_t *ring, int64_t n_nodes,
                                    int64_t v, int m, int *err)
{
    if (m == 0)
        return v;
    const int64_t id = ring[v * kRing + (m - 1)];
    if (id < -1 || id >= n_nodes) {
        *err |= kErrIndex;
        return -1;
    }
    return id;
}

// the fit of node v into fit[0 .. kFit): 1 and h, N^-1's upper triangle, or 0
// and zeros
__device__ inline int fit_node(int64_t n_nodes, const double *xyz,
                               const int32_t *ring, const int32_t *count,
                               int64_t v, double *fit, int *err)
{
    for (int k = 0; k < kFit; ++k)
        fit[k] = 0.0;
    const Tangent T = tangent_at(node_at(xyz, v));
    int members = 0;
    bool ok = true;
    double h = 0.0;
    for (int m = 0; m <= kRing; ++m) {
        const int64_t id = member_of(ring, n_nodes, v, m, err);
        if (id < 0)
            continue;
        ++members;
        double x, y, t;
        T.project(node_at(xyz, id), &x, &y, &t);
        const double r = sqrt(x * x + y * y);
        ok &= t > kPatchMinCos && isfinite(r);
        h = r > h ? r : h;
    }
    const int32_t nc = count[v];
    ok &= members >= kMinMembers && nc <= kRing && nc == members - 1 &&
        h > 0.0;
    if (!ok)
        return 0;
    // N, the upper triangle row-major, the members added in order
    double N[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j)
            N[i][j] = 0.0;
    for (int m = 0; m <= kRing; ++m) {
        const int64_t id = member_of(ring, n_nodes, v, m, err);
        if (id < 0)
            continue;
        double x, y, t;
        T.project(node_at(xyz, id), &x, &y, &t);
        x = x / h;
        y = y / h;
        const double phi[6] = {1.0, x, y, x * x, x * y, y * y};
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j)
                N[i][j] += phi[i] * phi[j];
    }
    // unpivoted Cholesky N = L L^T, row by row
    double L[6][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double d = N[k][k];
#pragma unroll
        for (int j = 0; j < k; ++j)
            d -= L[k][j] * L[k][j];
        ok &= isfinite(d) && d > kPivot * N[k][k];
        L[k][k] = sqrt(ok ? d : 1.0);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double s = N[k][i];
#pragma unroll
            for (int j = 0; j < k; ++j)
                s -= L[i][j] * L[k][j];
            L[i][k] = s / L[k][k];
        }
    }
    // M = L^-1 by forward substitution, N^-1 = M^T M
    double M[6][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        M[k][k] = 1.0 / L[k][k];
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = k; j < i; ++j)
                s -= L[i][j] * M[j][k];
            M[i][k] = s / L[i][i];
        }
    }
    double inv[21];
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            // (M is lower triangular: rows below j only)
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < 6; ++m)
                if (m >= j)
                    s += M[m][i] * M[m][j];
            ok &= isfinite(s);
            inv[at++] = s;
        }
    if (!ok)
        return 0;
    fit[0] = h;
#pragma unroll
    for (int k = 0; k < 21; ++k)
        fit[1 + k] = inv[k];
    return 1;
}

__global__ __launch_bounds__(kBlock) void patch_fits_kernel(
    int64_t n_nodes, const double *__restrict__ xyz,
    const int32_t *__restrict__ ring, const int32_t *__restrict__ count,
    double *__restrict__ fit_out, int32_t *__restrict__ has_out,
    int32_t *__restrict__ status)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_nodes)
        return;
    double fit[kFit];
    int err = 0;
    has_out[v] = fit_node(n_nodes, xyz, ring, count, v, fit, &err);
#pragma unroll
    for (int k = 0; k < kFit; ++k)
        fit_out[v * kFit + k] = fit[k];
    if (err)
        atomicOr(&status[0], err);
}

// ---------------------------------------------------------------------------
// rows
// ---------------------------------------------------------------------------

// The merge of the member lists of a point's three nodes by column.  Each
// list is the node itself and the first len[t] slots of its (ascending) ring;
// a bilinear row has len 0 everywhere.
struct RowWalk {
    const int32_t *ring;
    int64_t n_nodes;
    int32_t v[3];
    int32_t len[3], at[3];
    int32_t next_ring[3];     // the ring's next column, kNone at its end
    bool self_done[3];
    bool patch;
    int err;

    __device__ void load(int t)
    {
        next_ring[t] = kNone;
        if (at[t] >= len[t])
            return;
        const int32_t id = ring[(int64_t)v[t] * kRing + at[t]];
        if (id < 0 || id >= n_nodes) {
            err |= kErrIndex;
            at[t] = len[t];
            return;
        }
        next_ring[t] = id;
    }

    __device__ int32_t candidate(int t) const
    {
        const int32_t s = self_done[t] ? kNone : v[t];
        return s < next_ring[t] ? s : next_ring[t];
    }

    // the lowest column not yet taken, kNone at the end of the row
    __device__ int32_t column() const
    {
        int32_t c = candidate(0);
        const int32_t c1 = candidate(1), c2 = candidate(2);
        c = c1 < c ? c1 : c;
        return c2 < c ? c2 : c;
    }

    // list t past column c
    __device__ void advance(int t, int32_t c)
    {
        if (!self_done[t] && v[t] == c) {
            self_done[t] = true;
        } else {
            ++at[t];
            load(t);
        }
    }
};

// the walk of point p: false where the point has no row (found = -1, or an
// index outside its side: *err)
__device__ inline bool start_walk(int64_t n_nodes, const double *xyz,
                                  int64_t n_tri, const int32_t *tri,
                                  const int32_t *ring, const int32_t *count,
                                  const int32_t *has, const int32_t *found,
                                  const double *points, int64_t p, RowWalk *w,
                                  int *err)
{
    const int64_t f = found[p];
    if (f < 0 || f >= n_tri) {
        if (f != -1)
            *err |= kErrFound;
        return false;
    }
    w->ring = ring;
    w->n_nodes = n_nodes;
    w->err = 0;
    const V3 q = node_at(points, p);
    bool patch = true;
    for (int t = 0; t < 3; ++t) {
        const int32_t v = tri[f * 3 + t];
        if (v < 0 || v >= n_nodes) {
            *err |= kErrIndex;
            return false;
        }
        w->v[t] = v;
        patch &= has[v] != 0 && dot(q, node_at(xyz, v)) > kPatchMinCos;
    }
    w->patch = patch;
    for (int t = 0; t < 3; ++t) {
        int32_t n = patch ? count[w->v[t]] : 0;
        n = n < 0 ? 0 : (n > kRing ? kRing : n);
        w->len[t] = n;
        w->at[t] = 0;
        w->self_done[t] = false;
        w->load(t);
    }
    return true;
}

// pass 1: cnt[p] = the distinct columns of row p; cnt[n_pts] = 0
__global__ __launch_bounds__(kBlock) void patch_sizes_kernel(
    int64_t n_nodes, const double *__restrict__ xyz, int64_t n_tri,
    const int32_t *__restrict__ tri, const int32_t *__restrict__ ring,
    const int32_t *__restrict__ count, const int32_t *__restrict__ has,
    int64_t n_pts, const int32_t *__restrict__ found,
    const double *__restrict__ points, int64_t *__restrict__ cnt,
    int32_t *__restrict__ status)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > n_pts)
        return;
    int64_t n = 0;
    int err = 0;
    RowWalk w;
    if (p < n_pts && start_walk(n_nodes, xyz, n_tri, tri, ring, count, has,
                                found, points, p, &w, &err)) {
        // (a column leaves at least one list: at most 3 * (kRing + 1) turns)
        for (int32_t c = w.column(); c != kNone; c = w.column()) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (w.candidate(t) == c)
                    w.advance(t, c);
            ++n;
        }
        err |= w.err;
    }
    cnt[p] = n;
    if (err)
        atomicOr(&status[0], err);
}

// pass 2 for point p: the same walk with the values, written at [o, end).
// Returns the status bits.
__device__ inline int emit_row(int64_t n_nodes, const double *xyz,
                               int64_t n_tri, const int32_t *tri,
                               const int32_t *ring, const int32_t *count,
                               const double *fit, const int32_t *has,
                               const int32_t *found, const double *wgt,
                               const double *points, int64_t p, int64_t o,
                               int64_t end, int32_t *row_out,
                               int32_t *col_out, double *s_out)
{
    int err = 0;
    RowWalk w;
    if (!start_walk(n_nodes, xyz, n_tri, tri, ring, count, has, found, points,
                    p, &w, &err))
        return err | (end != o ? kErrCapacity : 0);
    const double b[3] = {wgt[p * 3], wgt[p * 3 + 1], wgt[p * 3 + 2]};
    Tangent T[3];
    double h[3], g[3][6];
    if (w.patch) {
        const V3 q = node_at(points, p);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double *f = fit + (int64_t)w.v[t] * kFit;
            T[t] = tangent_at(node_at(xyz, w.v[t]));
            h[t] = f[0];
            double x, y, c;
            T[t].project(q, &x, &y, &c);
            x = x / h[t];
            y = y / h[t];
            const double phi[6] = {1.0, x, y, x * x, x * y, y * y};
            // g = N^-1 phi from the upper triangle (row i starts at
            // i * 6 - i * (i - 1) / 2), added in ascending j
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    s += f[1 + lo * 6 - lo * (lo - 1) / 2 + (hi - lo)] *
                        phi[j];
                }
                g[t][i] = s;
            }
        }
    }
    for (int32_t c = w.column(); c != kNone; c = w.column()) {
        double s = 0.0;
        bool first = true;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (w.candidate(t) != c)
                continue;
            double val = b[t];
            if (w.patch) {
                double x, y, cc;
                T[t].project(node_at(xyz, c), &x, &y, &cc);
                val = b[t] * basis_dot(g[t], x / h[t], y / h[t]);
            }
            s = first ? val : s + val;
            first = false;
            w.advance(t, c);
        }
        // (nothing is written outside the row's own slots)
        if (o >= end)
            return err | w.err | kErrCapacity;
        row_out[o] = static_cast<int32_t>(p);
        col_out[o] = c;
        s_out[o] = s;
        ++o;
    }
    return err | w.err | (o != end ? kErrCapacity : 0);
}

__global__ __launch_bounds__(kBlock) void patch_rows_kernel(
    int64_t n_nodes, const double *__restrict__ xyz, int64_t n_tri,
    const int32_t *__restrict__ tri, const int32_t *__restrict__ ring,
    const int32_t *__restrict__ count, const double *__restrict__ fit,
    const int32_t *__restrict__ has, int64_t n_pts,
    const int32_t *__restrict__ found, const double *__restrict__ wgt,
    const double *__restrict__ points, const int64_t *__restrict__ offsets,
    int64_t capacity, int32_t *__restrict__ row_out,
    int32_t *__restrict__ col_out, double *__restrict__ s_out,
    int32_t *__restrict__ status)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pts)
        return;
    const int64_t o = offsets[p], end = offsets[p + 1];
    if (o < 0 || end < o || end > capacity ||
        (p == n_pts - 1 && end != capacity)) {
        atomicOr(&status[0], kErrCapacity);
        return;
    }
    const int err = emit_row(n_nodes, xyz, n_tri, tri, ring, count, fit, has,
                             found, wgt, points, p, o, end, row_out, col_out,
                             s_out);
    if (err)
        atomicOr(&status[0], err);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct RingsLayout {
    size_t keys_in, keys_out, head, rank, first, temp, total, temp_bytes;
};

int rings_layout(int64_t n_tri, int64_t n_nodes, RingsLayout *lay)
{
    const size_t n = at_least_one(n_tri) * 6;
    size_t sort = 0, scan = 0;
    REMAP_TRY(sort_keys_temp(n, &sort));
    REMAP_TRY(scan_temp<uint32_t>(n, &scan));
    lay->temp_bytes = sort > scan ? sort : scan;
    size_t off = 0;
    lay->keys_in = take(&off, n * 8);
    lay->keys_out = take(&off, n * 8);
    lay->head = take(&off, n * 4);
    lay->rank = take(&off, n * 4);
    lay->first = take(&off, at_least_one(n_nodes) * 4);
    lay->temp = take(&off, lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

int check_sizes(const char *name, int64_t n_nodes, int64_t n_tri)
{
    // (6 n_tri pairs are ranked in 32 bits)
    if (n_nodes < 1 || n_nodes > INT32_MAX || n_tri < 0 ||
        n_tri > (int64_t(1) << 32) / 6 - 1)
        return fail(REMAP_ERR_ARG,
                    "%s: n_nodes %lld, n_tri %lld: expected 1 <= n_nodes < "
                    "2^31 and 0 <= n_tri < 2^32 / 6", name,
                    static_cast<long long>(n_nodes),
                    static_cast<long long>(n_tri));
    return REMAP_OK;
}

int status_fail(const char *name, int32_t bits)
{
    if (bits & kErrIndex)
        return fail(REMAP_ERR_ARG,
                    "%s: tri or ring names a node outside the mesh", name);
    if (bits & kErrFound)
        return fail(REMAP_ERR_ARG,
                    "%s: found names a triangle outside [-1, n_tri)", name);
    return fail(REMAP_ERR_ARG,
                "%s: offsets differ from remap_patch_sizes' for these arrays",
                name);
}

// the status word read back (the one read-back of a call, waited for): what
// its bits say, or REMAP_OK
int status_check(const char *name, const int32_t *status, hipStream_t stream)
{
    int32_t err = 0;
    REMAP_TRY(read_back(&err, status, sizeof(int32_t), stream));
    if (err)
        return status_fail(name, err);
    return REMAP_OK;
}

// remap_patch_sizes' workspace: the n_pts + 1 counts, then the scan's scratch
struct SizesLayout {
    size_t cnt, temp, total, temp_bytes;
};

int sizes_layout(int64_t n_pts, SizesLayout *lay)
{
    REMAP_TRY(scan_temp<int64_t>(static_cast<size_t>(n_pts) + 1,
                                 &lay->temp_bytes));
    size_t off = 0;
    lay->cnt = take(&off, static_cast<size_t>(n_pts + 1) * 8);
    lay->temp = take(&off, lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

}  // namespace

int node_rings_workspace(int64_t n_tri, int64_t n_nodes, size_t *bytes_out)
{
    const char *name = "remap_node_rings_workspace";
    if (!bytes_out)
        return fail(REMAP_ERR_ARG, "%s: NULL bytes_out", name);
    REMAP_TRY(check_sizes(name, n_nodes, n_tri));
    RingsLayout lay;
    REMAP_TRY(rings_layout(n_tri, n_nodes, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int node_rings(int64_t n_tri, const int32_t *tri, int64_t n_nodes,
               int32_t *ring_out, int32_t *count_out, int32_t *status,
               void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *name = "remap_node_rings";
    REMAP_TRY(check_sizes(name, n_nodes, n_tri));
    if (!ring_out || !count_out || !status || (n_tri > 0 && !tri))
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    RingsLayout lay;
    REMAP_TRY(rings_layout(n_tri, n_nodes, &lay));
    REMAP_TRY(need_workspace(name, workspace, workspace_bytes, lay.total));
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    REMAP_HIP_CHECK(hipMemsetAsync(ring_out, 0xff,
                                   sizeof(int32_t) * n_nodes * kRing, stream));
    REMAP_HIP_CHECK(hipMemsetAsync(count_out, 0, sizeof(int32_t) * n_nodes,
                                   stream));
    if (n_tri == 0)
        return REMAP_OK;
    char *ws = static_cast<char *>(workspace);
    uint64_t *keys_in = at<uint64_t>(ws, lay.keys_in);
    uint64_t *keys = at<uint64_t>(ws, lay.keys_out);
    uint32_t *head = at<uint32_t>(ws, lay.head);
    uint32_t *rank = at<uint32_t>(ws, lay.rank);
    uint32_t *first = at<uint32_t>(ws, lay.first);
    void *temp = ws + lay.temp;
    const int64_t n = n_tri * 6;
    REMAP_TRY(launch(ring_pairs, n_tri, kBlock, stream, n_tri, tri, n_nodes,
                     keys_in, status));
    REMAP_TRY(radix_sort_keys(temp, lay.temp_bytes, keys_in, keys, n, stream));
    REMAP_TRY(launch(ring_heads, n, kBlock, stream, n, keys, head));
    REMAP_TRY(exclusive_scan(temp, lay.temp_bytes, head, rank, n, stream));
    REMAP_TRY(launch(ring_firsts, n, kBlock, stream, n, keys, rank, n_nodes,
                     first));
    REMAP_TRY(launch(ring_fill, n, kBlock, stream, n, keys, head, rank, first,
                     n_nodes, ring_out, count_out));
    return status_check(name, status, stream);
}

int patch_fits(int64_t n_nodes, const double *xyz, const int32_t *ring,
               const int32_t *count, double *fit_out, int32_t *has_out,
               int32_t *status, hipStream_t stream)
{
    const char *name = "remap_patch_fits";
    REMAP_TRY(check_sizes(name, n_nodes, 0));
    if (!xyz || !ring || !count || !fit_out || !has_out || !status)
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    REMAP_TRY(launch(patch_fits_kernel, n_nodes, kBlock, stream, n_nodes, xyz,
                     ring, count, fit_out, has_out, status));
    return status_check(name, status, stream);
}

int check_points(const char *name, int64_t n_nodes, int64_t n_tri,
                 int64_t n_pts)
{
    REMAP_TRY(check_sizes(name, n_nodes, n_tri));
    if (n_tri > INT32_MAX || n_pts < 0 || n_pts > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "%s: n_tri %lld, n_pts %lld: expected n_tri < 2^31 and "
                    "0 <= n_pts < 2^31", name, static_cast<long long>(n_tri),
                    static_cast<long long>(n_pts));
    return REMAP_OK;
}

int patch_sizes_workspace(int64_t n_pts, size_t *bytes_out)
{
    const char *name = "remap_patch_sizes_workspace";
    if (!bytes_out)
        return fail(REMAP_ERR_ARG, "%s: NULL bytes_out", name);
    if (n_pts < 0 || n_pts > INT32_MAX)
        return fail(REMAP_ERR_ARG, "%s: n_pts %lld: expected 0 <= n_pts < "
                    "2^31", name, static_cast<long long>(n_pts));
    SizesLayout lay;
    REMAP_TRY(sizes_layout(n_pts, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int patch_sizes(int64_t n_nodes, const double *xyz, int64_t n_tri,
                const int32_t *tri, const int32_t *ring, const int32_t *count,
                const int32_t *has, int64_t n_pts, const int32_t *found,
                const double *points, int64_t *offsets_out,
                int64_t *total_out, int32_t *status, void *workspace,
                size_t workspace_bytes, hipStream_t stream)
{
    const char *name = "remap_patch_sizes";
    REMAP_TRY(check_points(name, n_nodes, n_tri, n_pts));
    if (!xyz || !ring || !count || !has || !offsets_out || !total_out ||
        !status || (n_tri > 0 && !tri) || (n_pts > 0 && (!found || !points)))
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    SizesLayout lay;
    REMAP_TRY(sizes_layout(n_pts, &lay));
    REMAP_TRY(need_workspace(name, workspace, workspace_bytes, lay.total));
    char *ws = static_cast<char *>(workspace);
    int64_t *cnt = at<int64_t>(ws, lay.cnt);
    *total_out = 0;
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    // (n_pts + 1 >= 1 lanes: the last writes the count behind the rows)
    REMAP_TRY(launch(patch_sizes_kernel, n_pts + 1, kBlock, stream, n_nodes,
                     xyz, n_tri, tri, ring, count, has, n_pts, found, points,
                     cnt, status));
    REMAP_TRY(exclusive_scan(ws + lay.temp, lay.temp_bytes, cnt, offsets_out,
                             n_pts + 1, stream));
    int64_t total = 0;
    REMAP_HIP_CHECK(hipMemcpyAsync(&total, offsets_out + n_pts,
                                   sizeof(int64_t), hipMemcpyDeviceToHost,
                                   stream));
    REMAP_TRY(status_check(name, status, stream));
    *total_out = total;
    return REMAP_OK;
}

int patch_rows(int64_t n_nodes, const double *xyz, int64_t n_tri,
               const int32_t *tri, const int32_t *ring, const int32_t *count,
               const double *fit, const int32_t *has, int64_t n_pts,
               const int32_t *found, const double *w, const double *points,
               const int64_t *offsets, int64_t capacity, int32_t *row_out,
               int32_t *col_out, double *s_out, int32_t *status,
               hipStream_t stream)
{
    const char *name = "remap_patch_rows";
    REMAP_TRY(check_points(name, n_nodes, n_tri, n_pts));
    if (capacity < 0)
        return fail(REMAP_ERR_ARG, "%s: capacity %lld", name,
                    static_cast<long long>(capacity));
    if (!status)
        return fail(REMAP_ERR_ARG, "%s: NULL status", name);
    if (n_pts == 0)
        return REMAP_OK;
    if (!xyz || !ring || !count || !fit || !has || !found || !w || !points ||
        !offsets || (n_tri > 0 && !tri) ||
        (capacity > 0 && (!row_out || !col_out || !s_out)))
        return fail(REMAP_ERR_ARG, "%s: NULL array", name);
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    REMAP_TRY(launch(patch_rows_kernel, n_pts, kBlock, stream, n_nodes, xyz,
                     n_tri, tri, ring, count, fit, has, n_pts, found, w,
                     points, offsets, capacity, row_out, col_out, s_out,
                     status));
    return status_check(name, status, stream);
}

}  // namespace remap

extern "C" {

int remap_node_rings_workspace(int64_t n_tri, int64_t n_nodes,
                               size_t *bytes_out)
{
    return remap::node_rings_workspace(n_tri, n_nodes, bytes_out);
}

int remap_node_rings(int64_t n_tri, const int32_t *tri, int64_t n_nodes,
                     int32_t *ring_out, int32_t *count_out, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    return remap::node_rings(n_tri, tri, n_nodes, ring_out, count_out, status,
                             workspace, workspace_bytes,
                             static_cast<hipStream_t>(stream));
}

int remap_patch_fits(int64_t n_nodes, const double *xyz, const int32_t *ring,
                     const int32_t *count, double *fit_out, int32_t *has_out,
                     int32_t *status, void *stream)
{
    return remap::patch_fits(n_nodes, xyz, ring, count, fit_out, has_out,
                             status, static_cast<hipStream_t>(stream));
}

int remap_patch_sizes_workspace(int64_t n_pts, size_t *bytes_out)
{
    return remap::patch_sizes_workspace(n_pts, bytes_out);
}

int remap_patch_sizes(int64_t n_nodes, const double *xyz, int64_t n_tri,
                      const int32_t *tri, const int32_t *ring,
                      const int32_t *count, const int32_t *has, int64_t n_pts,
                      const int32_t *found, const double *points,
                      int64_t *offsets_out, int64_t *total_out,
                      int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    return remap::patch_sizes(n_nodes, xyz, n_tri, tri, ring, count, has,
                              n_pts, found, points, offsets_out, total_out,
                              status, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

int remap_patch_rows(int64_t n_nodes, const double *xyz, int64_t n_tri,
                     const int32_t *tri, const int32_t *ring,
                     const int32_t *count, const double *fit,
                     const int32_t *has, int64_t n_pts, const int32_t *found,
                     const double *w, const double *points,
                     const int64_t *offsets, int64_t capacity,
                     int32_t *row_out, int32_t *col_out, double *s_out,
                     int32_t *status, void *stream)
{
    return remap::patch_rows(n_nodes, xyz, n_tri, tri, ring, count, fit, has,
                             n_pts, found, w, points, offsets, capacity,
                             row_out, col_out, s_out, status,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
