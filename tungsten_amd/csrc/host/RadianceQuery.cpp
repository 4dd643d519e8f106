#include "RadianceQuery.hpp"
#include "../../../include/tungsten_host.h"

#include <cstdint>
#include <cstdio>

int checkRadianceQuery(const TgHipRadianceQueryDesc *desc, const void *rays, const void *rgbSum, const void *count, size_t n, bool sceneHasSobol,
                       std::string &error)
{
    if (!desc) { error = "tghip_query_radiance: no description"; return TGHIP_E_INVALID; }
    if (desc->flags & ~(TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_RADIANCE_SOBOL)) { error = "tghip_query_radiance: unknown flag bits"; return TGHIP_E_INVALID; }
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u || desc->reserved[2] != 0u) { error = "tghip_query_radiance: the reserved words must be zero"; return TGHIP_E_INVALID; }
    if (desc->spp_end <= desc->spp_begin) { error = "tghip_query_radiance: spp_end must be above spp_begin"; return TGHIP_E_INVALID; }
    if ((desc->flags & TGHIP_RADIANCE_SOBOL) && !sceneHasSobol) {
        error = "tghip_query_radiance: TGHIP_RADIANCE_SOBOL needs sobol_matrices in the scene description";
        return TGHIP_E_INVALID;
    }
    if (uint64_t(n) > 0x7FFFFFFFull) { error = "tghip_query_radiance: more than 2^31 - 1 rays"; return TGHIP_E_INVALID; }
    if (n == 0) return TGHIP_OK;                 // (an empty batch asks nothing of its arrays)
    if (!rays || !rgbSum) { error = "tghip_query_radiance: rays and rgb_sum are needed for a batch that is not empty"; return TGHIP_E_INVALID; }
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        // k_query_paths reads a ray as two 16-byte vectors; the sums and counts are written word by word
        if (reinterpret_cast<uintptr_t>(rays) & 15u) { error = "tghip_query_radiance: device rays must be 16-byte aligned"; return TGHIP_E_INVALID; }
        if ((reinterpret_cast<uintptr_t>(rgbSum) | reinterpret_cast<uintptr_t>(count)) & 3u) {
            error = "tghip_query_radiance: device rgb_sum and count must be 4-byte aligned";
            return TGHIP_E_INVALID;
        }
    }
    // the size planPass refuses a record pass at -- 2^32 samples on one device: a plain pass of that size it would cut into batches without end
    if (uint64_t(n)*(desc->spp_end - desc->spp_begin) >= (1ull << 32)) {
        error = "tghip_query_radiance: pass too large (2^32 samples or more per device): fewer rays or a shorter sample range per call";
        return TGHIP_E_UNSUPPORTED;
    }
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
    const int rc = checkRadianceQuery(desc, rays, rgb_sum, count, n, scene_has_sobol != 0, error);
    if (rc != TGHIP_OK && err && errlen) std::snprintf(err, errlen, "%s", error.c_str());
    return rc;
}
