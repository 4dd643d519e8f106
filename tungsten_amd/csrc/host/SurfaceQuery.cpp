#include "SurfaceQuery.hpp"
#include "../../../include/tungsten_host.h"

#include <cstdint>
#include <cstdio>

static_assert(sizeof(TgHipSurface) == 96, "a TgHipSurface is six 16-byte vectors");
static_assert(sizeof(TgHipSurfaceQueryDesc) == 16, "TgHipSurfaceQueryDesc is four words");

int checkSurfaceQuery(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error)
{
    if (!desc) { error = "tghip_query_surface: no description"; return TGHIP_E_INVALID; }
    if (desc->flags & ~TGHIP_DEVELOP_DEVICE_POINTERS) { error = "tghip_query_surface: unknown flag bits"; return TGHIP_E_INVALID; }
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u || desc->reserved[2] != 0u) {
        error = "tghip_query_surface: the reserved words must be zero";
        return TGHIP_E_INVALID;
    }
    if (uint64_t(n) > 0x7FFFFFFFull) { error = "tghip_query_surface: more than 2^31 - 1 rays"; return TGHIP_E_INVALID; }
    if (n == 0) return TGHIP_OK;                 // (an empty batch asks nothing of its arrays)
    if (!rays || !out) { error = "tghip_query_surface: rays and out are needed for a batch that is not empty"; return TGHIP_E_INVALID; }
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        // the kernels read a ray as two 16-byte vectors and write an answer as six
        if ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u) {
            error = "tghip_query_surface: device rays and answers must be 16-byte aligned";
            return TGHIP_E_INVALID;
        }
    }
    return TGHIP_OK;
}

extern "C" int tgh_query_surface_check(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen)
{
    std::string error;
    const int rc = checkSurfaceQuery(desc, rays, out, n, error);
    if (rc != TGHIP_OK && err && errlen) std::snprintf(err, errlen, "%s", error.c_str());
    return rc;
}
