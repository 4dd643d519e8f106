#include "RadianceQuery.hpp"
#include "QueryCheck.hpp"
#include "../../../include/tungsten_host.h"

int checkRadianceQuery(const TgHipRadianceQueryDesc *desc, const void *rays, const void *rgbSum, const void *count, size_t n, bool sceneHasSobol,
                       std::string &error)
{
    const QueryCheck c = {"tghip_query_radiance", error};
    if (!desc) return c.refuse("no description");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_RADIANCE_SOBOL, desc->reserved, 3);
    if (rc != TGHIP_OK) return rc;
    if (desc->spp_end <= desc->spp_begin) return c.refuse("spp_end must be above spp_begin");
    if ((desc->flags & TGHIP_RADIANCE_SOBOL) && !sceneHasSobol) return c.refuse("TGHIP_RADIANCE_SOBOL needs sobol_matrices in the scene description");
    // k_query_paths reads a ray as two 16-byte vectors; the sums and counts are written word by word
    if ((rc = c.rays(n)) == TGHIP_OK)
        rc = c.arrays(n, (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, rays, rgbSum, "rays and rgb_sum", queryAddress(rays), "device rays",
                      queryAddress(rgbSum) | queryAddress(count), "device rgb_sum and count");
    if (rc != TGHIP_OK) return rc;
    // the size planPass refuses a record pass at -- 2^32 samples on one device: a plain pass of that size it would cut into batches without end
    if (uint64_t(n)*(desc->spp_end - desc->spp_begin) >= (1ull << 32))
        return c.refuse("pass too large (2^32 samples or more per device): fewer rays or a shorter sample range per call", TGHIP_E_UNSUPPORTED);
    return TGHIP_OK;
}

RadianceQueryImage radianceQueryImage(size_t n)
{
    RadianceQueryImage im;
    im.width = RADIANCE_QUERY_WIDTH;
    im.height = uint32_t((uint64_t(n) + RADIANCE_QUERY_WIDTH - 1u)/RADIANCE_QUERY_WIDTH);
    return im;
}

TgHipPassDesc radianceQueryPass(const TgHipRadianceQueryDesc &desc)
{
    TgHipPassDesc pass = TgHipPassDesc();
    pass.spp_begin = desc.spp_begin; pass.spp_end = desc.spp_end;
    pass.seed = desc.seed;
    pass.shard_index = 0; pass.shard_count = 1;
    pass.flags = (desc.flags & TGHIP_RADIANCE_SOBOL) ? TGHIP_PASS_SOBOL : 0u;
    return pass;
}

int planRadianceQuery(const TgHipRadianceQueryDesc &desc, size_t n, const PassPlanOptions &opt, PassPlan &out, std::string &error)
{
    const RadianceQueryImage im = radianceQueryImage(n);
    return planPass(radianceQueryPass(desc), im.width, im.height, opt, out, error);
}

extern "C" int tgh_query_radiance_check(const TgHipRadianceQueryDesc *desc, const void *rays, const void *rgb_sum, const void *count, size_t n,
                                        int scene_has_sobol, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkRadianceQuery(desc, rays, rgb_sum, count, n, scene_has_sobol != 0, error), error, err, errlen);
}
