// remap_expand.hip -- the reference's expand_dist / expand_factor on the
// device: every cell's corners moved away from the cell's centre before the
// conservative weights are made (smoothed maps).
//
// Definition (include/remap_hip.h has the contract; pyremap_amd.weights
// .expand_cells is the same statement in numpy).  All in fp64, WGS84
// (a = 6378137 m, 1/f = 298.257223563), heights 0:
//   ecef(lat, lon)  (0, 0, +-b) where |lat| >= pi/2 (rule A: a pole is ONE
//                   point, whatever its longitude, as unit_latlon of
//                   remap_overlap.hip has it), otherwise with N = a /
//                   sqrt(1 - e2 sin^2 lat): (N cos lat cos lon,
//                   N cos lat sin lon, N (1 - e2) sin lat)
//   c = ecef(centre), p = ecef(corner), v = p - c, d = |v|
//   d == 0          the corner stays as it was given (rule B: the fixed point
//                   of the expansion; the reference divides 0 by 0 there)
//   r = factor * d + dist; r <= 0 is an error
//   t = c + (r / d) * v
//   lon' = atan2(t.y, t.x); lat' = the geodetic latitude of t, its height
//   dropped: kSteps steps of Bowring's iteration on the reduced latitude,
//     th = atan2(a t.z, b q), q = sqrt(t.x^2 + t.y^2), then kSteps times
//     lat' = atan2(t.z + e'2 b sin^3 th, q - e2 a cos^3 th),
//     th = atan2(b sin lat', a cos lat')
//   -- a fixed count, no data-dependent loop.  One step is Bowring's closed
//   formula, up to 2e-10 rad off the foot point for the expansions served
//   here; the second step is converged to rounding and the third is margin.
//   Slots k >= count[cell] are copied (rule C).
//
// One lane per corner SLOT of the (n_cells, width) arrays: loads and stores
// of the corner arrays are coalesced, the per-cell values (centre, count,
// dist, factor) are re-read and the centre's ecef recomputed by each of the
// cell's `width` lanes (they hit the same cache lines).  No LDS, no
// floating-point atomics: the result is a pure function of the inputs, two
// corners with equal inputs get equal bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "remap_common.h"
#include "remap_host.h"

namespace remap {
namespace {

constexpr double kA = 6378137.0;
constexpr double kF = 1.0 / 298.257223563;
constexpr double kB = kA * (1.0 - kF);
constexpr double kE2 = kF * (2.0 - kF);
constexpr double kEp2 = kE2 / (1.0 - kE2);
constexpr double kHalfPi = 0.5 * 3.14159265358979323846;
constexpr int kSteps = 3;

struct V3 {
    double x, y, z;
};

__device__ inline V3 ecef(double lat, double lon)
{
    if (lat >= kHalfPi)
        return {0.0, 0.0, kB};
    if (lat <= -kHalfPi)
        return {0.0, 0.0, -kB};
    const double s = sin(lat), c = cos(lat);
    const double n = kA / sqrt(1.0 - kE2 * s * s);
    return {n * c * cos(lon), n * c * sin(lon), n * (1.0 - kE2) * s};
}

__device__ inline void flag(int32_t *status, int bit, int64_t n_cells,
                            int64_t cell)
{
    atomicOr(&status[0], bit);
    // (the LOWEST offending cell: the largest n_cells - cell)
    atomicMax(&status[1], static_cast<int32_t>(n_cells - cell));
}

__global__ __launch_bounds__(kBlock) void expand_slots(
    int64_t n_cells, int32_t width, const double *__restrict__ centre_lat,
    const double *__restrict__ centre_lon,
    const double *__restrict__ corner_lat,
    const double *__restrict__ corner_lon, const int32_t *__restrict__ count,
    const double *__restrict__ dist, int32_t dist_stride,
    const double *__restrict__ factor, int32_t factor_stride,
    double *__restrict__ out_lat, double *__restrict__ out_lon,
    int32_t *__restrict__ status)
{
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (at >= n_cells * width)
        return;
    const int64_t cell = at / width;
    const int32_t k = static_cast<int32_t>(at - cell * width);
    const double lat = corner_lat[at], lon = corner_lon[at];
    const int32_t nc = count[cell];
    const double clat = centre_lat[cell], clon = centre_lon[cell];
    const double ds = dist[cell * dist_stride];
    const double fc = factor[cell * factor_stride];
    // (every slot is checked, padding too: the numpy statement's rule)
    double new_lat = lat, new_lon = lon;
    if (nc < 0 || nc > width) {
        flag(status, REMAP_EXPAND_ERR_COUNT, n_cells, cell);
    } else if (!(isfinite(lat) && isfinite(lon) && isfinite(clat) &&
                 isfinite(clon) && isfinite(ds) && isfinite(fc))) {
        flag(status, REMAP_EXPAND_ERR_FINITE, n_cells, cell);
    } else if (k < nc) {
        const V3 c = ecef(clat, clon), p = ecef(lat, lon);
        const V3 v = {p.x - c.x, p.y - c.y, p.z - c.z};
        const double d = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
        if (d > 0.0) {
            const double r = fc * d + ds;
            if (!(r > 0.0)) {
                flag(status, REMAP_EXPAND_ERR_RADIUS, n_cells, cell);
            } else {
                const double g = r / d;
                const V3 t = {c.x + g * v.x, c.y + g * v.y, c.z + g * v.z};
                const double q = sqrt(t.x * t.x + t.y * t.y);
                double th = atan2(kA * t.z, kB * q);
                for (int step = 0; step < kSteps; ++step) {
                    const double s = sin(th), co = cos(th);
                    new_lat = atan2(t.z + kEp2 * kB * (s * s * s),
                                    q - kE2 * kA * (co * co * co));
                    th = atan2(kB * sin(new_lat), kA * cos(new_lat));
                }
                new_lon = atan2(t.y, t.x);
            }
        }
    }
    out_lat[at] = new_lat;
    out_lon[at] = new_lon;
}

}  // namespace

int expand_cells(int64_t n_cells, int32_t width, const double *centre_lat,
                 const double *centre_lon, const double *corner_lat,
                 const double *corner_lon, const int32_t *count,
                 const double *dist, int32_t dist_stride,
                 const double *factor, int32_t factor_stride, double *out_lat,
                 double *out_lon, int32_t *status, hipStream_t stream)
{
    if (n_cells < 0 || n_cells > INT32_MAX || width < 1)
        return fail(REMAP_ERR_ARG,
                    "remap_expand_cells: n_cells %lld, width %d: expected 0 "
                    "<= n_cells < 2^31 and width >= 1",
                    static_cast<long long>(n_cells), width);
    if ((dist_stride != 0 && dist_stride != 1) ||
        (factor_stride != 0 && factor_stride != 1))
        return fail(REMAP_ERR_ARG,
                    "remap_expand_cells: strides %d and %d: expected 0 (a "
                    "scalar) or 1 (a value per cell)",
                    dist_stride, factor_stride);
    if (!dist || !factor || !status)
        return fail(REMAP_ERR_ARG, "remap_expand_cells: NULL dist, factor "
                                   "or status");
    if (n_cells == 0)
        return REMAP_OK;
    if (!centre_lat || !centre_lon || !corner_lat || !corner_lon || !count ||
        !out_lat || !out_lon)
        return fail(REMAP_ERR_ARG, "remap_expand_cells: NULL array");
    const int64_t slots = n_cells * width;
    const int64_t n_blocks = (slots + kBlock - 1) / kBlock;
    if (n_blocks > INT32_MAX)
        return fail(REMAP_ERR_ARG,
                    "remap_expand_cells: %lld corner slots are more than one "
                    "launch serves", static_cast<long long>(slots));
    REMAP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    REMAP_TRY(launch(expand_slots, slots, kBlock, stream, n_cells, width,
                     centre_lat, centre_lon, corner_lat, corner_lon, count,
                     dist, dist_stride, factor, factor_stride, out_lat,
                     out_lon, status));
    int32_t err[2] = {0, 0};
    REMAP_TRY(read_back(err, status, sizeof(err), stream));
    if (err[0]) {
        const long long cell = static_cast<long long>(n_cells) - err[1];
        return fail(REMAP_ERR_ARG,
                    "remap_expand_cells: %s%s%sfirst at cell %lld",
                    (err[0] & REMAP_EXPAND_ERR_COUNT)
                        ? "a count outside [0, width] "
                          "(REMAP_EXPAND_ERR_COUNT); " : "",
                    (err[0] & REMAP_EXPAND_ERR_FINITE)
                        ? "a NaN or Inf among the inputs "
                          "(REMAP_EXPAND_ERR_FINITE); " : "",
                    (err[0] & REMAP_EXPAND_ERR_RADIUS)
                        ? "factor * d + dist <= 0 for a corner at a distance "
                          "d > 0 from its centre (REMAP_EXPAND_ERR_RADIUS); "
                        : "",
                    cell);
    }
    return REMAP_OK;
}

}  // namespace remap

extern "C" {

int remap_expand_cells(int64_t n_cells, int32_t width,
                       const double *centre_lat, const double *centre_lon,
                       const double *corner_lat, const double *corner_lon,
                       const int32_t *count, const double *dist,
                       int32_t dist_stride, const double *factor,
                       int32_t factor_stride, double *out_lat,
                       double *out_lon, int32_t *status, void *stream)
{
    return remap::expand_cells(n_cells, width, centre_lat, centre_lon,
                               corner_lat, corner_lon, count, dist,
                               dist_stride, factor, factor_stride, out_lat,
                               out_lon, status,
                               static_cast<hipStream_t>(stream));
}

}  // extern "C"
