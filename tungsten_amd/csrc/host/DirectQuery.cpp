#include "DirectQuery.hpp"
#include "QueryCheck.hpp"

static_assert(sizeof(TgHipDirect) == 32, "a TgHipDirect is two 16-byte vectors");
static_assert(sizeof(TgHipDirectQueryDesc) == 32, "TgHipDirectQueryDesc is eight words");

int checkDirectQuery(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n, const TgHostDirectScene *scene,
                     std::string &error)
{
    const QueryCheck c = {"tghip_query_direct", error};
    if (!desc) return c.refuse("no description");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_DIRECT_VOLUME, nullptr, 0);     // (the description has no reserved word)
    if (rc == TGHIP_OK) rc = c.rays(n);
    if (rc != TGHIP_OK) return rc;
    if (desc->spp_end <= desc->spp_begin) return c.refuse("spp_end must be above spp_begin");
    if (desc->skip > 1024u) return c.refuse("skip above 1024");
    if (desc->bounce > 255u) return c.refuse("bounce above 255");
    const uint32_t numMedia = scene ? scene->num_media : 0u, numLights = scene ? scene->num_lights : 0u;
    if (desc->light < -1 || (desc->light >= 0 && uint32_t(desc->light) >= numLights)) return c.refuse("light outside the scene's lights");
    if (desc->medium < TGHIP_MEDIUM_OF_CAMERA || (desc->medium >= 0 && uint32_t(desc->medium) >= numMedia))
        return c.refuse("medium index outside the scene's table");
    if (desc->medium >= 0 && scene->medium_operand && scene->medium_operand[desc->medium])
        return c.refuse("the medium entry is an operand of an interpolated transmittance, not a medium");
    if ((desc->flags & TGHIP_DIRECT_VOLUME) && !media) {
        const int32_t resolved = desc->medium == TGHIP_MEDIUM_OF_CAMERA ? (scene ? scene->camera_medium : -1) : desc->medium;
        if (resolved < 0) return c.refuse("volume mode needs a medium to start in");
    }
    // the kernels read a ray as two 16-byte vectors, a start medium as a word, and write an answer as two vectors
    rc = c.arrays(n, (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, rays, out, "rays and out", queryAddress(rays) | queryAddress(out),
                  "device rays and answers", queryAddress(media), "device start media");
    if (rc != TGHIP_OK) return rc;
    if (uint64_t(n)*uint64_t(desc->spp_end - desc->spp_begin) >= (1ull << 32))
        return c.refuse("2^32 or more (ray, sample) items in one call", TGHIP_E_UNSUPPORTED);
    return TGHIP_OK;
}

extern "C" int tgh_query_direct_check(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                                      const TgHostDirectScene *scene, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkDirectQuery(desc, rays, media, out, n, scene, error), error, err, errlen);
}
