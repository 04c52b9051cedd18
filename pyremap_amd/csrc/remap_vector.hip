// remap_vector.hip -- vector fields on the apply path: the eastward and
// northward components (u, v) of every source cell are rotated to Cartesian
// (x, y, z), summed with the row's weights and projected on the destination
// cell's east and north, in one launch (ESMF's vectorRegrid).
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.vector.apply
// is the same statement in numpy).  BA (n_a, 5) and BB (n_b, 5) hold the rows
// (ex, ey, nx, ny, nz) of the source and destination cells, made on the host.
// For destination element (i, b, k) the row's entries are walked in CSR
// order, four float64 accumulators from +0.0:
//   u = (double)U[cell(col), b, k];  v = (double)V[cell(col), b, k]
//   the entry counts iff neither is a NaN; then, with the basis row of col:
//   px = u*ex + v*nx;  py = u*ey + v*ny;  pz = v*nz
//   cx += S*px;  cy += S*py;  cz += S*pz;  valid += S
//   with the basis row (Ex, Ey, Nx, Ny, Nz) of row i:
//   tu = cx*Ex + cy*Ey;  tv = (cx*Nx + cy*Ny) + cz*Nz
//   valid > threshold ? (yu, yv) = (tu / valid, tv / valid) : both NaN
// Every product and every sum rounds on its own (the library is built with
// -ffp-contract=off, and nothing here asks for an fma); an entry that does
// not count is skipped, not added as a zero.  Every NaN written is the one
// quiet NaN 0x7ff8000000000000.
//
// Two forms, as remap_sgs.hip has them (rowpass.h).  Runs of at least a
// wave's width (k_inner >= 64) take a wave per (row, chunk of columns),
// vector_rowwave below: the entry's basis row is the same in every lane and
// is a scalar load beside col and val.  Everything else takes one lane per
// (row, column), vector_rowlane: a lane walks its row four or two entries at
// a time, the (col, S) pairs fetched together (index clamped to the last
// entry: no load sits behind a branch), then the basis rows and the values
// together, then the sums in CSR order.  With several batches ((Time,
// nCells[, n])) the lanes run over the rows and columns of ONE batch and a
// lane serves four batches with one fetch of the row's indices, weights and
// basis rows.  No LDS, no atomics.  The pass moves what two REMAP_MODE_MASKED
// applies move plus 40 bytes per entry and per row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "rowpass.h"

namespace remap {
namespace {

using namespace rowpass;

constexpr char kName[] = "remap_apply_vector";
constexpr int kBasis = 5;           // (ex, ey, nx, ny, nz)

struct VectorParams {               // (rowpass.h: P)
    const int64_t *__restrict__ rowptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ val;
    const void *__restrict__ U;
    const void *__restrict__ V;
    const double *__restrict__ BA;
    const double *__restrict__ BB;
    double *__restrict__ YU;
    double *__restrict__ YV;
    int64_t row_begin, n_rows;      // rows [row_begin, row_begin + n_rows)
    int64_t K, k_inner;             // K = n_batch * k_inner
    int64_t ldx, bsx, ldy, bsy;
    int64_t src_outer;
    uint32_t src_fold;
    int64_t total;                  // n_rows * K
    double thr;
};

// element offset of source cell a in U and in V
__device__ inline int64_t cell_offset(const VectorParams &p, int32_t a)
{
    int64_t o[1];
    rowpass::cell_offsets(p, a, {p.ldx}, {p.src_outer}, o);
    return o[0];
}

struct Basis {
    double ex, ey, nx, ny, nz;
};

__device__ inline Basis load_basis(const double *__restrict__ B, int64_t cell)
{
    const double *__restrict__ b = B + cell * kBasis;
    return {b[0], b[1], b[2], b[3], b[4]};
}

struct Sums {
    double cx, cy, cz, valid;
};

// one entry of the definition
__device__ inline void add_entry(Sums &s, double a, const Basis &e, double u,
                                 double v)
{
    if (u == u && v == v) {
        const double uex = u * e.ex;
        const double vnx = v * e.nx;
        const double uey = u * e.ey;
        const double vny = v * e.ny;
        const double px = uex + vnx;
        const double py = uey + vny;
        const double pz = v * e.nz;
        const double ax = a * px;
        const double ay = a * py;
        const double az = a * pz;
        s.cx = s.cx + ax;
        s.cy = s.cy + ay;
        s.cz = s.cz + az;
        s.valid = s.valid + a;
    }
}

// (a quotient that is itself a NaN -- inf / inf, a NaN weight -- leaves as
// the same quiet NaN as a masked element: the bits of YU and YV are defined)
__device__ inline void finish(const Sums &s, const Basis &E, double thr,
                              double &yu, double &yv)
{
    const double xe = s.cx * E.ex;
    const double ye = s.cy * E.ey;
    const double tu = xe + ye;
    const double xn = s.cx * E.nx;
    const double yn = s.cy * E.ny;
    const double zn = s.cz * E.nz;
    const double tv = (xn + yn) + zn;
    const double qu = tu / s.valid;
    const double qv = tv / s.valid;
    const bool ok = s.valid > thr;
    yu = (ok && qu == qu) ? qu : __builtin_nan("");
    yv = (ok && qv == qv) ? qv : __builtin_nan("");
}

// IT: the type the flat index is split in (rowpass::narrow_index).
// BATCH_MAJOR (several batches whose rows lie closer than the batches: (Time,
// nCells[, n])): the lanes run over (row, k) of ONE batch, k fastest, and a
// lane serves kBatches batches of its (row, k): the row's indices, weights
// and basis rows are fetched once for them.  (A batch past the last is served
// as a copy of the last and not stored.)
// UNR: the entries a lane fetches together.  Four without batches; with them
// four where k_inner == 1 ((Time, nCells): 8-byte gathers, a short row in one
// round) and two otherwise (the registers of eight source values a round
// cost more occupancy than the second round costs): both measured, DESIGN
// section 22.
constexpr int kBatches = 4;

template <typename XT, typename IT, bool BATCH_MAJOR, int UNR>
__global__ __launch_bounds__(kBlock) void vector_rowlane(
    const VectorParams p, const int64_t n_batch)
{
    constexpr int NB = BATCH_MAJOR ? kBatches : 1;
    const int64_t gid64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid64 >= p.total)
        return;
    const IT gid = static_cast<IT>(gid64);
    const IT ki = static_cast<IT>(p.k_inner);
    IT r, b, k;
    if constexpr (BATCH_MAJOR) {
        const IT per = static_cast<IT>(p.n_rows) * ki;
        const IT bg = gid / per;
        const IT rem = gid - bg * per;
        r = rem / ki;
        k = rem - r * ki;
        b = bg * NB;
    } else {
        const IT K = static_cast<IT>(p.K);
        r = gid / K;
        const IT kf = gid - r * K;
        b = kf / ki;
        k = kf - b * ki;
    }
    const int64_t i = p.row_begin + static_cast<int64_t>(r);
    const XT *__restrict__ Up[NB];
    const XT *__restrict__ Vp[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        int64_t bn = static_cast<int64_t>(b) + n;
        if (bn > n_batch - 1)
            bn = n_batch - 1;
        const int64_t at = bn * p.bsx + static_cast<int64_t>(k);
        Up[n] = static_cast<const XT *>(p.U) + at;
        Vp[n] = static_cast<const XT *>(p.V) + at;
    }
    const int64_t o = i * p.ldy + static_cast<int64_t>(b) * p.bsy +
                      static_cast<int64_t>(k);
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    Sums sum[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
        sum[n] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t base = s; base < e; base += UNR) {
        int32_t c[UNR];
        double a[UNR];
        Basis bs[UNR];
        XT us[UNR][NB];
        XT vs[UNR][NB];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t jj = base + u < e ? base + u : e - 1;
            c[u] = p.col[jj];
            a[u] = p.val[jj];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t ox = cell_offset(p, c[u]);
            bs[u] = load_basis(p.BA, c[u]);
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                us[u][n] = Up[n][ox];
                vs[u][n] = Vp[n][ox];
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (base + u < e) {
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    add_entry(sum[n], a[u], bs[u],
                              static_cast<double>(us[u][n]),
                              static_cast<double>(vs[u][n]));
            }
    }
    const Basis E = load_basis(p.BB, i);
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (static_cast<int64_t>(b) + n < n_batch) {
            double yu, yv;
            finish(sum[n], E, p.thr, yu, yv);
            __builtin_nontemporal_store(yu, p.YU + o + n * p.bsy);
            __builtin_nontemporal_store(yv, p.YV + o + n * p.bsy);
        }
}

// ---------------------------------------------------------------------------
// rowwave: one wave per (row, chunk of kWave * VEC contiguous columns), lanes
// across the columns, as sgs_rowwave -- for runs of >= kWave columns; the
// work list and VEC are rowpass.h's.  The row is the same in every lane, so
// the row pointers, the column indices, the weights and the entries' basis
// rows are scalar loads, the loop over the row's entries is wave-uniform and
// reads exactly the row's entries, UNR pairs of source runs in flight at a
// time.  YU and YV are written once (store_once).
// ---------------------------------------------------------------------------
template <typename XT, int VEC>
__global__ __launch_bounds__(kBlock) void vector_rowwave(
    const VectorParams p, const int64_t n_waves, const int64_t chunks,
    const int64_t per_xcd)
{
    constexpr int UNR = 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = rowwave_place(per_xcd);
    if (w >= n_waves)
        return;
    const int64_t cb = w / p.n_rows;            // (batch, chunk), chunk-major
    const int64_t r = w - cb * p.n_rows;
    const int64_t b = cb / chunks;
    const int64_t chunk = cb - b * chunks;
    const int64_t k = chunk * (kWave * VEC) + (int64_t)lane * VEC;
    if (k >= p.k_inner)                         // (VEC = 2: k_inner is even)
        return;
    const int64_t i = p.row_begin + r;
    const XT *__restrict__ U = static_cast<const XT *>(p.U) + b * p.bsx + k;
    const XT *__restrict__ V = static_cast<const XT *>(p.V) + b * p.bsx + k;
    const int64_t o = i * p.ldy + b * p.bsy + k;
    const int64_t s = p.rowptr[i];
    const int64_t e = p.rowptr[i + 1];
    using PX = Pack<XT, VEC>;
    Sums sum[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        sum[v] = {0.0, 0.0, 0.0, 0.0};
    int64_t j = s;
    for (; j + UNR <= e; j += UNR) {
        PX us[UNR], vs[UNR];
        double a[UNR];
        Basis bs[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int32_t c = p.col[j + u];
            const int64_t ox = cell_offset(p, c);
            a[u] = p.val[j + u];
            bs[u] = load_basis(p.BA, c);
            us[u] = *reinterpret_cast<const PX *>(U + ox);
            vs[u] = *reinterpret_cast<const PX *>(V + ox);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                add_entry(sum[v], a[u], bs[u],
                          static_cast<double>(us[u].v[v]),
                          static_cast<double>(vs[u].v[v]));
    }
    for (; j < e; ++j) {
        const int32_t c = p.col[j];
        const int64_t ox = cell_offset(p, c);
        const double a = p.val[j];
        const Basis bs = load_basis(p.BA, c);
        const PX us = *reinterpret_cast<const PX *>(U + ox);
        const PX vs = *reinterpret_cast<const PX *>(V + ox);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            add_entry(sum[v], a, bs, static_cast<double>(us.v[v]),
                      static_cast<double>(vs.v[v]));
    }
    const Basis E = load_basis(p.BB, i);
    Pack<double, VEC> yu, yv;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        finish(sum[v], E, p.thr, yu.v[v], yv.v[v]);
    store_once<VEC>(p.YU + o, yu);
    store_once<VEC>(p.YV + o, yv);
}

template <typename XT>
int launch_rowwave(const VectorParams &p, int64_t n_batch, hipStream_t stream)
{
    const bool even = even_strides(p) && aligned_to(p.U, 2 * sizeof(XT)) &&
                      aligned_to(p.V, 2 * sizeof(XT)) &&
                      aligned_to(p.YU, 16) && aligned_to(p.YV, 16);
    WaveGrid g;
    const int rc = rowwave_grid(kName, p, n_batch, even ? 2 : 1, g);
    if (rc != REMAP_OK)
        return rc;
    if (even)
        hipLaunchKernelGGL((vector_rowwave<XT, 2>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    else
        hipLaunchKernelGGL((vector_rowwave<XT, 1>), g.grid, dim3(kBlock), 0,
                           stream, p, g.n_waves, g.chunks, g.per_xcd);
    return REMAP_OK;
}

template <typename XT>
int launch_vector(const VectorParams &p, int64_t n_batch, bool batch_major,
                  hipStream_t stream)
{
    if (p.k_inner >= kWave)
        // runs of a wave's width and more: a wave per (row, chunk)
        return launch_rowwave<XT>(p, n_batch, stream);
    VectorParams q = p;
    if (batch_major)                // (a lane per kBatches batches)
        q.total = (n_batch + kBatches - 1) / kBatches * p.n_rows * p.k_inner;
    const dim3 grid = rowlane_grid(q.total);
    const bool narrow = narrow_index(p);
    const bool single = p.k_inner == 1;
    if (narrow && batch_major && single)
        hipLaunchKernelGGL((vector_rowlane<XT, uint32_t, true, 4>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (narrow && batch_major)
        hipLaunchKernelGGL((vector_rowlane<XT, uint32_t, true, 2>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (narrow)
        hipLaunchKernelGGL((vector_rowlane<XT, uint32_t, false, 4>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (batch_major && single)
        hipLaunchKernelGGL((vector_rowlane<XT, int64_t, true, 4>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else if (batch_major)
        hipLaunchKernelGGL((vector_rowlane<XT, int64_t, true, 2>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    else
        hipLaunchKernelGGL((vector_rowlane<XT, int64_t, false, 4>), grid,
                           dim3(kBlock), 0, stream, q, n_batch);
    return REMAP_OK;
}

}  // namespace

int apply_vector(const remap_vector_args *a, hipStream_t stream)
{
    if (!a)
        return fail(REMAP_ERR_ARG, "%s: NULL args", kName);
    VectorParams p;
    bool empty;
    const int checked = check_args(kName, *a, p, empty);
    if (checked != REMAP_OK || empty)
        return checked;
    if (!p.rowptr || (a->A.nnz > 0 && (!p.col || !a->A.val || !a->BA)) ||
        !a->U || !a->V || !a->BB || !a->YU || !a->YV)
        return fail(REMAP_ERR_ARG,
                    "%s: NULL rowptr, col, val, U, V, BA, BB, YU or YV",
                    kName);
    p.val = a->A.val;
    p.U = a->U;
    p.V = a->V;
    p.BA = a->BA;
    p.BB = a->BB;
    p.YU = a->YU;
    p.YV = a->YV;
    p.thr = a->threshold;
    // several batches whose rows lie closer than the batches: the lanes run
    // over the rows and columns of one batch
    const bool batch_major = a->n_batch > 1 &&
                             a->y_row_stride <= a->y_batch_stride;
    const int rc = a->x_dtype == REMAP_DTYPE_F64
                       ? launch_vector<double>(p, a->n_batch, batch_major,
                                               stream)
                       : launch_vector<float>(p, a->n_batch, batch_major,
                                              stream);
    if (rc != REMAP_OK)
        return rc;
    REMAP_HIP_CHECK(hipGetLastError());
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_apply_vector(const struct remap_vector_args *args, void *stream)
{
    return remap::apply_vector(args, static_cast<hipStream_t>(stream));
}

}  // extern "C"
