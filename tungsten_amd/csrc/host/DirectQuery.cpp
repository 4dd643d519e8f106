#include "DirectQuery.hpp"

#include <cstdint>
#include <cstdio>

static_assert(sizeof(TgHipDirect) == 32, "a TgHipDirect is two 16-byte vectors");
static_assert(sizeof(TgHipDirectQueryDesc) == 32, "TgHipDirectQueryDesc is eight words");

int checkDirectQuery(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n, const TgHostDirectScene *scene,
                     std::string &error)
{
    if (!desc) { error = "tghip_query_direct: no description"; return TGHIP_E_INVALID; }
    if (desc->flags & ~(TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_DIRECT_VOLUME)) { error = "tghip_query_direct: unknown flag bits"; return TGHIP_E_INVALID; }
    if (uint64_t(n) > 0x7FFFFFFFull) { error = "tghip_query_direct: more than 2^31 - 1 rays"; return TGHIP_E_INVALID; }
    if (desc->spp_end <= desc->spp_begin) { error = "tghip_query_direct: spp_end must be above spp_begin"; return TGHIP_E_INVALID; }
    if (desc->skip > 1024u) { error = "tghip_query_direct: skip above 1024"; return TGHIP_E_INVALID; }
    if (desc->bounce > 255u) { error = "tghip_query_direct: bounce above 255"; return TGHIP_E_INVALID; }
    const uint32_t numMedia = scene ? scene->num_media : 0u, numLights = scene ? scene->num_lights : 0u;
    if (desc->light < -1 || (desc->light >= 0 && uint32_t(desc->light) >= numLights)) {
        error = "tghip_query_direct: light outside the scene's lights";
        return TGHIP_E_INVALID;
    }
    if (desc->medium < TGHIP_MEDIUM_OF_CAMERA || (desc->medium >= 0 && uint32_t(desc->medium) >= numMedia)) {
        error = "tghip_query_direct: medium index outside the scene's table";
        return TGHIP_E_INVALID;
    }
    if (desc->medium >= 0 && scene->medium_operand && scene->medium_operand[desc->medium]) {
        error = "tghip_query_direct: the medium entry is an operand of an interpolated transmittance, not a medium";
        return TGHIP_E_INVALID;
    }
    if ((desc->flags & TGHIP_DIRECT_VOLUME) && !media) {
        const int32_t resolved = desc->medium == TGHIP_MEDIUM_OF_CAMERA ? (scene ? scene->camera_medium : -1) : desc->medium;
        if (resolved < 0) { error = "tghip_query_direct: volume mode needs a medium to start in"; return TGHIP_E_INVALID; }
    }
    if (n == 0) return TGHIP_OK;                 // (an empty batch asks nothing of its arrays)
    if (!rays || !out) { error = "tghip_query_direct: rays and out are needed for a batch that is not empty"; return TGHIP_E_INVALID; }
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        // the kernels read a ray as two 16-byte vectors, a start medium as a word, and write an answer as two vectors
        if ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u) {
            error = "tghip_query_direct: device rays and answers must be 16-byte aligned";
            return TGHIP_E_INVALID;
        }
        if (reinterpret_cast<uintptr_t>(media) & 3u) {
            error = "tghip_query_direct: device start media must be 4-byte aligned";
            return TGHIP_E_INVALID;
        }
    }
    if (uint64_t(n)*uint64_t(desc->spp_end - desc->spp_begin) >= (1ull << 32)) {
        error = "tghip_query_direct: 2^32 or more (ray, sample) items in one call";
        return TGHIP_E_UNSUPPORTED;
    }
    return TGHIP_OK;
}

extern "C" int tgh_query_direct_check(const TgHipDirectQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                                      const TgHostDirectScene *scene, char *err, size_t errlen)
{
    std::string error;
    const int rc = checkDirectQuery(desc, rays, media, out, n, scene, error);
    if (rc != TGHIP_OK && err && errlen) std::snprintf(err, errlen, "%s", error.c_str());
    return rc;
}
