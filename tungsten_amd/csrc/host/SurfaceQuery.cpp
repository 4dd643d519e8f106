#include "SurfaceQuery.hpp"
#include "QueryCheck.hpp"
#include "../../../include/tungsten_host.h"

static_assert(sizeof(TgHipSurface) == 96, "a TgHipSurface is six 16-byte vectors");
static_assert(sizeof(TgHipSurfaceQueryDesc) == 16, "TgHipSurfaceQueryDesc is four words");

int checkSurfaceQuery(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, std::string &error)
{
    const QueryCheck c = {"tghip_query_surface", error};
    if (!desc) return c.refuse("no description");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS, desc->reserved, 3);
    if (rc == TGHIP_OK) rc = c.rays(n);
    // the kernels read a ray as two 16-byte vectors and write an answer as six
    if (rc == TGHIP_OK)
        rc = c.arrays(n, (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, rays, out, "rays and out", queryAddress(rays) | queryAddress(out),
                      "device rays and answers");
    return rc;
}

extern "C" int tgh_query_surface_check(const TgHipSurfaceQueryDesc *desc, const void *rays, const void *out, size_t n, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkSurfaceQuery(desc, rays, out, n, error), error, err, errlen);
}
