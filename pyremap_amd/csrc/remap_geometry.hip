// remap_geometry.hip -- what a complete mapping file says about its two grids
// beyond the weights: every cell's area (area_a, area_b) and the fraction of
// every source cell that takes part in the map (frac_a).
//
// remap_cell_areas: cells in SCRIP layout, (n_cells, width) row-major corner
// latitudes / longitudes in radians, the first count[i] slots of row i valid.
// A cell is the great-circle polygon of those corners; its area is
//   | sum_k tri_area(p_0, p_k, p_k+1) |
// over the ring with consecutive equal corners dropped and the closing copies
// of p_0 dropped -- the ring, the fan and the triangle formula (tri_area of
// remap_sphere.h, Van Oosterom-Strackee) of remap_overlap.hip's cell
// preparation, so a cell has the bits here that the overlap calls give it.
// The sum is signed and its absolute value taken at the end: a clockwise
// ring and a concave cell (a vertex cell beside a land mask) come out right.
// Fewer than 3 corners left: area 0.
//   A block serves kCells = 64 cells.  Its 64 * width corner slots are read
// by all 256 lanes in slot order (coalesced), turned into unit vectors there
// (the trigonometry is the expensive part and runs on every lane), and
// written to LDS transposed, corner k of cell c at [k * 64 + c]; then lane c
// of the first wave walks cell c's ring in LDS, conflict-free.
//
// remap_column_fractions: out[j] = sum of value[k] over col[k] == j, added
// in ascending k starting from +0.0 -- np.bincount(col, weights=value) on
// the same entry order, bit for bit -- then divided by denom[j] when denom
// is given and cut to at most 1 when clamp is set.  A column without entries
// is 0 (it is not divided).  No floating-point atomics: the entries are
// regrouped by column with rocPRIM's radix_sort_pairs, the LSD radix sort
// remap_csr.hip uses, which is STABLE (entries of one key keep their input
// order: rocPRIM documents it, and csr_from_coo's left-to-right sum of
// duplicates rests on it), and one lane walks one column in that order.  Two
// calls give the same bytes.  A column of many entries (the source cell
// under a polar cap) is walked by its one lane, serially: the order is the
// contract.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string.h>

#include "remap_common.h"
#include "remap_host.h"
#include "remap_sphere.h"

namespace remap {
namespace {

constexpr int kCells = kWave;     // cells per block: one per lane of wave 0
constexpr int kMaxWidth = REMAP_CELL_AREAS_MAX_WIDTH;
// a column's key: its 32 bits are what the sort looks at
constexpr unsigned kKeyBits = 32;

__global__ __launch_bounds__(kBlock) void cell_areas_kernel(
    int64_t n_cells, int32_t width, const double *__restrict__ corner_lat,
    const double *__restrict__ corner_lon, const int32_t *__restrict__ count,
    double *__restrict__ area_out, int32_t *__restrict__ status)
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
    if (nc < 0 || nc > width) {
        atomicOr(&status[0], 1);
        // (the LOWEST offending cell: the largest n_cells - cell)
        atomicMax(&status[1], static_cast<int32_t>(n_cells - cell));
        area_out[cell] = 0.0;
        return;
    }
    double *x = sx + lane, *y = sy + lane, *z = sz + lane;
    // consecutive equal corners dropped, in place (nv <= k throughout)
    int nv = 0;
    for (int k = 0; k < nc; ++k) {
        const V3 p = {x[k * kCells], y[k * kCells], z[k * kCells]};
        if (nv > 0 && p.x == x[(nv - 1) * kCells] &&
            p.y == y[(nv - 1) * kCells] && p.z == z[(nv - 1) * kCells])
            continue;
        x[nv * kCells] = p.x;
        y[nv * kCells] = p.y;
        z[nv * kCells] = p.z;
        ++nv;
    }
    const V3 p0 = {x[0], y[0], z[0]};
    while (nv > 1 && x[(nv - 1) * kCells] == p0.x &&
           y[(nv - 1) * kCells] == p0.y && z[(nv - 1) * kCells] == p0.z)
        --nv;
    double a = 0.0;
    if (nv >= 3) {
        V3 prev = {x[kCells], y[kCells], z[kCells]};
        for (int k = 2; k < nv; ++k) {
            const V3 p = {x[k * kCells], y[k * kCells], z[k * kCells]};
            a += tri_area(p0, prev, p);
            prev = p;
        }
    }
    area_out[cell] = fabs(a);
}

struct Layout {
    size_t keys_in, keys_out, vals_out, temp, total;
    size_t temp_bytes;
};

int make_layout(int64_t n_entries, Layout *lay)
{
    const size_t n = at_least_one(n_entries);
    REMAP_TRY((sort_pairs_temp<double, uint32_t>(n, &lay->temp_bytes,
                                                 kKeyBits)));
    size_t off = 0;
    lay->keys_in = take(&off, n * 4);
    lay->keys_out = take(&off, n * 4);
    lay->vals_out = take(&off, n * 8);
    lay->temp = take(&off, lay->temp_bytes);
    lay->total = off;
    return REMAP_OK;
}

__global__ __launch_bounds__(kBlock) void column_keys(
    int64_t n_entries, int64_t n_cols, int32_t base,
    const int32_t *__restrict__ col, uint32_t *__restrict__ keys,
    int64_t *__restrict__ bad)
{
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_entries)
        return;
    const int64_t c = (int64_t)col[n] - base;
    if (c < 0 || c >= n_cols) {
        atomicAdd(reinterpret_cast<unsigned long long *>(bad), 1ull);
        keys[n] = ~0u;  // behind every column (n_cols < 2^31)
        return;
    }
    keys[n] = static_cast<uint32_t>(c);
}

__global__ __launch_bounds__(kBlock) void column_sums(
    int64_t n_entries, int64_t n_cols, const uint32_t *__restrict__ keys,
    const double *__restrict__ vals, const double *__restrict__ denom,
    int32_t clamp, double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_cols)
        return;
    const uint32_t key = static_cast<uint32_t>(j);
    // the first sorted entry whose column is >= j
    int64_t lo = 0, hi = n_entries;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    // bincount's order: from +0.0, one entry after the other
    double s = 0.0;
    int64_t m = lo;
    for (; m < n_entries && keys[m] == key; ++m)
        s = s + vals[m];
    if (m > lo) {
        if (denom)
            s = s / denom[j];
        if (clamp && s > 1.0)
            s = 1.0;
    }
    out[j] = s;
}

}  // namespace

int cell_areas(int64_t n_cells, int32_t width, const double *corner_lat,
               const double *corner_lon, const int32_t *count,
               double *area_out, int32_t *status, hipStream_t stream)
{
    if (n_cells < 0 || n_cells > INT32_MAX || width < 1)
        return fail(REMAP_ERR_ARG,
                    "remap_cell_areas: n_cells %lld, width %d: expected 0 <= "
                    "n_cells < 2^31 and width >= 1",
                    static_cast<long long>(n_cells), width);
    if (width > kMaxWidth)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_cell_areas: width %d, this build serves up to %d "
                    "corners a cell", width, kMaxWidth);
    if (!status)
        return fail(REMAP_ERR_ARG, "remap_cell_areas: NULL status");
    if (n_cells == 0)
        return REMAP_OK;
    if (!corner_lat || !corner_lon || !count || !area_out)
        return fail(REMAP_ERR_ARG, "remap_cell_areas: NULL array");
    const size_t lds_bytes = sizeof(double) * 3 * kCells * width;
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    REMAP_TRY(launch_blocks(cell_areas_kernel, blocks(n_cells, kCells),
                            kBlock, lds_bytes, stream, n_cells, width,
                            corner_lat, corner_lon, count, area_out, status));
    int32_t err[2] = {0, 0};
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0])
        return fail(REMAP_ERR_ARG,
                    "remap_cell_areas: a count outside [0, %d], first at "
                    "cell %lld", width,
                    static_cast<long long>(n_cells) - err[1]);
    return REMAP_OK;
}

int column_fractions_workspace(int64_t n_entries, size_t *bytes_out)
{
    if (!bytes_out || n_entries < 0)
        return fail(REMAP_ERR_ARG,
                    "remap_column_fractions_workspace: bad args");
    Layout lay;
    REMAP_TRY(make_layout(n_entries, &lay));
    *bytes_out = lay.total;
    return REMAP_OK;
}

int column_fractions(int64_t n_entries, int64_t n_cols, const int32_t *col,
                     int32_t index_base, const double *value,
                     const double *denom, int32_t clamp, double *out,
                     int64_t *bad_out, void *workspace,
                     size_t workspace_bytes, hipStream_t stream)
{
    if (n_entries < 0 || n_cols < 0)
        return fail(REMAP_ERR_ARG,
                    "remap_column_fractions: negative size");
    if (n_cols >= (int64_t(1) << 31) ||
        n_entries >= (int64_t(1) << 32) - 1)
        return fail(REMAP_ERR_UNSUPPORTED,
                    "remap_column_fractions: sizes beyond 32-bit indices");
    if (!bad_out)
        return fail(REMAP_ERR_ARG, "remap_column_fractions: NULL bad_out");
    if (n_entries > 0 && (!col || !value))
        return fail(REMAP_ERR_ARG,
                    "remap_column_fractions: NULL entry array");
    if (n_cols > 0 && !out)
        return fail(REMAP_ERR_ARG, "remap_column_fractions: NULL out");
    Layout lay;
    REMAP_TRY(make_layout(n_entries, &lay));
    REMAP_TRY(need_workspace("remap_column_fractions", workspace,
                             workspace_bytes, lay.total));
    char *ws = static_cast<char *>(workspace);
    uint32_t *keys_in = at<uint32_t>(ws, lay.keys_in);
    uint32_t *keys_out = at<uint32_t>(ws, lay.keys_out);
    double *vals_out = at<double>(ws, lay.vals_out);

    REMAP_HIP_CHECK(hipMemsetAsync(bad_out, 0, sizeof(int64_t), stream));
    REMAP_TRY(launch(column_keys, n_entries, kBlock, stream, n_entries,
                     n_cols, index_base, col, keys_in, bad_out));
    if (n_entries > 0)
        REMAP_TRY(radix_sort_pairs(ws + lay.temp, lay.temp_bytes, keys_in,
                                   keys_out, value, vals_out, n_entries,
                                   stream, kKeyBits));
    return launch(column_sums, n_cols, kBlock, stream, n_entries, n_cols,
                  keys_out, vals_out, denom, clamp, out);
}

}  // namespace remap

extern "C" {

int remap_cell_areas(int64_t n_cells, int32_t width, const double *corner_lat,
                     const double *corner_lon, const int32_t *count,
                     double *area_out, int32_t *status, void *stream)
{
    return remap::cell_areas(n_cells, width, corner_lat, corner_lon, count,
                             area_out, status,
                             static_cast<hipStream_t>(stream));
}

int remap_column_fractions_workspace(int64_t n_entries, size_t *bytes_out)
{
    return remap::column_fractions_workspace(n_entries, bytes_out);
}

int remap_column_fractions(int64_t n_entries, int64_t n_cols,
                           const int32_t *col, int32_t index_base,
                           const double *value, const double *denom,
                           int32_t clamp, double *out, int64_t *bad_out,
                           void *workspace, size_t workspace_bytes,
                           void *stream)
{
    return remap::column_fractions(n_entries, n_cols, col, index_base, value,
                                   denom, clamp, out, bad_out, workspace,
                                   workspace_bytes,
                                   static_cast<hipStream_t>(stream));
}

}  // extern "C"
