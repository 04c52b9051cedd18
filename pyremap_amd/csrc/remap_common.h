// Shared helpers of libremap_hip.so (gfx950 only).
#ifndef REMAP_COMMON_H
#define REMAP_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "remap_hip.h"

namespace remap {

// thread-local message behind remap_last_error()
char *error_buffer();
constexpr int kErrorBufferSize = 512;

inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), kErrorBufferSize, fmt, ap);
    va_end(ap);
    return code;
}

inline int hip_fail(hipError_t err, const char *what)
{
    return fail(REMAP_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
}

#define REMAP_HIP_CHECK(expr)                                   \
    do {                                                        \
        hipError_t err__ = (expr);                              \
        if (err__ != hipSuccess)                                \
            return ::remap::hip_fail(err__, #expr);             \
    } while (0)

// The modes of remap_apply_f64 and remap_plan_apply.  (The enumerators are
// not contiguous: 4 to 7, 12, 14 and 15 are not assigned.)
inline bool is_rowstat_mode(int mode)
{
    return mode >= REMAP_MODE_MIN && mode <= REMAP_MODE_MEDIAN;
}

// the cotangent of the division, the first step of the adjoint apply
// (apply_cotangent.h)
inline bool is_cotangent_mode(int mode)
{
    return mode == REMAP_MODE_COTAN_FRACB || mode == REMAP_MODE_COTAN_MASKED;
}

// one pass of a creeping fill over a grid's neighbour matrix (apply_fill.h)
inline bool is_fill_mode(int mode)
{
    return mode == REMAP_MODE_FILL_BEST || mode == REMAP_MODE_FILL_MEAN;
}

inline bool is_known_mode(int mode)
{
    return (mode >= REMAP_MODE_RAW && mode <= REMAP_MODE_LAF) ||
           is_rowstat_mode(mode) || mode == REMAP_MODE_CLASSFRAC ||
           is_cotangent_mode(mode) || is_fill_mode(mode);
}

// the modes that are a row pass over ONE CSR and pick their own launch: no
// schedule, no tune, no flags (apply_laf.h, apply_rowstat.h,
// apply_classfrac.h, apply_cotangent.h, apply_fill.h)
inline bool is_rowpass_mode(int mode)
{
    return mode == REMAP_MODE_LAF || is_rowstat_mode(mode) ||
           mode == REMAP_MODE_CLASSFRAC || is_cotangent_mode(mode) ||
           is_fill_mode(mode);
}

constexpr int kWave = 64;        // gfx950 wavefront
constexpr int kBlock = 256;      // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kXcds = 8;         // MI355X: 8 XCDs, blocks dealt round-robin

}  // namespace remap

#endif  // REMAP_COMMON_H
