#include "TransmittanceQuery.hpp"

#include <cstdint>
#include <cstdio>

static_assert(sizeof(TgHipTransmittance) == 16, "a TgHipTransmittance is one 16-byte vector");
static_assert(sizeof(TgHipTransmittanceQueryDesc) == 32, "TgHipTransmittanceQueryDesc is eight words");

int checkTransmittanceQuery(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                            const TgHostTransmittanceScene *scene, std::string &error)
{
    if (!desc) { error = "tghip_query_transmittance: no description"; return TGHIP_E_INVALID; }
    if (desc->flags & ~(TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE | TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE)) {
        error = "tghip_query_transmittance: unknown flag bits";
        return TGHIP_E_INVALID;
    }
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u || desc->reserved[2] != 0u || desc->reserved[3] != 0u) {
        error = "tghip_query_transmittance: the reserved words must be zero";
        return TGHIP_E_INVALID;
    }
    if (uint64_t(n) > 0x7FFFFFFFull) { error = "tghip_query_transmittance: more than 2^31 - 1 rays"; return TGHIP_E_INVALID; }
    if (desc->bounce > 255u) { error = "tghip_query_transmittance: bounce above 255"; return TGHIP_E_INVALID; }
    const uint32_t numMedia = scene ? scene->num_media : 0u, numObjects = scene ? scene->num_objects : 0u;
    if (desc->medium < TGHIP_MEDIUM_OF_CAMERA || (desc->medium >= 0 && uint32_t(desc->medium) >= numMedia)) {
        error = "tghip_query_transmittance: medium index outside the scene's table";
        return TGHIP_E_INVALID;
    }
    if (desc->medium >= 0 && scene->medium_operand && scene->medium_operand[desc->medium]) {
        error = "tghip_query_transmittance: the medium entry is an operand of an interpolated transmittance, not a medium";
        return TGHIP_E_INVALID;
    }
    if (desc->end_cap < -1 || (desc->end_cap >= 0 && (uint32_t(desc->end_cap) >= numObjects || !scene->object_type))) {
        error = "tghip_query_transmittance: end cap outside the scene's objects";
        return TGHIP_E_INVALID;
    }
    if (desc->end_cap >= 0) {
        const int32_t type = scene->object_type[desc->end_cap];
        if (type == TGHIP_OBJ_INSTANCES) { error = "tghip_query_transmittance: the end cap is an instances object"; return TGHIP_E_INVALID; }
        if (type == TGHIP_OBJ_INFINITE_SPHERE || type == TGHIP_OBJ_INFINITE_SPHERE_CAP) {
            error = "tghip_query_transmittance: the end cap is an infinite emitter";
            return TGHIP_E_INVALID;
        }
    }
    if (n == 0) return TGHIP_OK;                 // (an empty batch asks nothing of its arrays)
    if (!rays || !out) { error = "tghip_query_transmittance: rays and out are needed for a batch that is not empty"; return TGHIP_E_INVALID; }
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        // the kernels read a ray as two 16-byte vectors, a start medium as a word, and write an answer as one vector
        if ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u) {
            error = "tghip_query_transmittance: device rays and answers must be 16-byte aligned";
            return TGHIP_E_INVALID;
        }
        if (reinterpret_cast<uintptr_t>(media) & 3u) {
            error = "tghip_query_transmittance: device start media must be 4-byte aligned";
            return TGHIP_E_INVALID;
        }
    }
    return TGHIP_OK;
}

extern "C" int tgh_query_transmittance_check(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                                             const TgHostTransmittanceScene *scene, char *err, size_t errlen)
{
    std::string error;
    const int rc = checkTransmittanceQuery(desc, rays, media, out, n, scene, error);
    if (rc != TGHIP_OK && err && errlen) std::snprintf(err, errlen, "%s", error.c_str());
    return rc;
}
