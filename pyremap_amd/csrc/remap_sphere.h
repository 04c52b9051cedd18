// Points and triangles on the unit sphere: the device functions the overlap
// kernels (remap_overlap.hip) and the cell areas (remap_geometry.hip) share,
// so that one cell's area has the same bits wherever it is computed, and the
// vector type of the point locations (remap_locate.hip, remap_quads.hip).
#ifndef REMAP_SPHERE_H
#define REMAP_SPHERE_H

#include <hip/hip_runtime.h>

namespace remap {

constexpr double kPi = 3.14159265358979323846;
constexpr double kHalfPi = 0.5 * kPi;
constexpr double kTwoPi = 2.0 * kPi;

struct V3 {
    double x, y, z;
};

// point i of an array of xyz triples
__device__ inline V3 load3(const double *__restrict__ p, int64_t i)
{
    return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
}

__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z,
            a.x * b.y - a.y * b.x};
}
// the squared length of the chord from u to v
__device__ inline double edge2(V3 u, V3 v)
{
    const double dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z;
    return (dx * dx + dy * dy) + dz * dz;
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

}  // namespace remap

#endif  // REMAP_SPHERE_H
