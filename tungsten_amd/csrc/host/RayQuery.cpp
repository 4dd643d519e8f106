#include "RayQuery.hpp"
#include "../../../include/tungsten_host.h"

#include <cstdint>
#include <cstdio>

int checkRayQuery(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error)
{
    if (!desc) { error = "tghip_query_rays: no description"; return TGHIP_E_INVALID; }
    if (desc->mode != TGHIP_QUERY_CLOSEST && desc->mode != TGHIP_QUERY_OCCLUDED) { error = "tghip_query_rays: unknown mode"; return TGHIP_E_INVALID; }
    if (desc->flags & ~TGHIP_DEVELOP_DEVICE_POINTERS) { error = "tghip_query_rays: unknown flag bits"; return TGHIP_E_INVALID; }
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u) { error = "tghip_query_rays: the reserved words must be zero"; return TGHIP_E_INVALID; }
    if (uint64_t(n) > 0x7FFFFFFFull) { error = "tghip_query_rays: more than 2^31 - 1 rays"; return TGHIP_E_INVALID; }
    if (n == 0) return TGHIP_OK;                 // (an empty batch asks nothing of its arrays)
    if (!rays || !out) { error = "tghip_query_rays: rays and out are needed for a batch that is not empty"; return TGHIP_E_INVALID; }
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        // the kernel reads a ray as two 16-byte vectors and writes a hit as one; an occlusion answer is a byte
        const uintptr_t wide = reinterpret_cast<uintptr_t>(rays) | (desc->mode == TGHIP_QUERY_CLOSEST ? reinterpret_cast<uintptr_t>(out) : uintptr_t(0));
        if (wide & 15u) { error = "tghip_query_rays: device rays and hits must be 16-byte aligned"; return TGHIP_E_INVALID; }
    }
    return TGHIP_OK;
}

extern "C" int tgh_query_rays_check(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen)
{
    std::string error;
    const int rc = checkRayQuery(desc, rays, out, n, error);
    if (rc != TGHIP_OK && err && errlen) std::snprintf(err, errlen, "%s", error.c_str());
    return rc;
}
