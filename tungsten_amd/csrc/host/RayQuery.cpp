#include "RayQuery.hpp"
#include "QueryCheck.hpp"
#include "../../../include/tungsten_host.h"

int checkRayQuery(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error)
{
    const QueryCheck c = {"tghip_query_rays", error};
    if (!desc) return c.refuse("no description");
    if (desc->mode != TGHIP_QUERY_CLOSEST && desc->mode != TGHIP_QUERY_OCCLUDED) return c.refuse("unknown mode");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS, desc->reserved, 2);
    if (rc == TGHIP_OK) rc = c.rays(n);
    // the kernel reads a ray as two 16-byte vectors and writes a hit as one; an occlusion answer is a byte
    if (rc == TGHIP_OK)
        rc = c.arrays(n, (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, rays, out, "rays and out",
                      queryAddress(rays) | (desc->mode == TGHIP_QUERY_CLOSEST ? queryAddress(out) : uintptr_t(0)), "device rays and hits");
    return rc;
}

extern "C" int tgh_query_rays_check(const TgHipRayQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkRayQuery(desc, rays, out, n, error), error, err, errlen);
}
