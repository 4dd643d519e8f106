#include "TransmittanceQuery.hpp"
#include "QueryCheck.hpp"

static_assert(sizeof(TgHipTransmittance) == 16, "a TgHipTransmittance is one 16-byte vector");
static_assert(sizeof(TgHipTransmittanceQueryDesc) == 32, "TgHipTransmittanceQueryDesc is eight words");

int checkTransmittanceQuery(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                            const TgHostTransmittanceScene *scene, std::string &error)
{
    const QueryCheck c = {"tghip_query_transmittance", error};
    if (!desc) return c.refuse("no description");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE | TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE, desc->reserved, 4);
    if (rc == TGHIP_OK) rc = c.rays(n);
    if (rc != TGHIP_OK) return rc;
    if (desc->bounce > 255u) return c.refuse("bounce above 255");
    const uint32_t numMedia = scene ? scene->num_media : 0u, numObjects = scene ? scene->num_objects : 0u;
    if (desc->medium < TGHIP_MEDIUM_OF_CAMERA || (desc->medium >= 0 && uint32_t(desc->medium) >= numMedia))
        return c.refuse("medium index outside the scene's table");
    if (desc->medium >= 0 && scene->medium_operand && scene->medium_operand[desc->medium])
        return c.refuse("the medium entry is an operand of an interpolated transmittance, not a medium");
    if (desc->end_cap < -1 || (desc->end_cap >= 0 && (uint32_t(desc->end_cap) >= numObjects || !scene->object_type)))
        return c.refuse("end cap outside the scene's objects");
    if (desc->end_cap >= 0) {
        const int32_t type = scene->object_type[desc->end_cap];
        if (type == TGHIP_OBJ_INSTANCES) return c.refuse("the end cap is an instances object");
        if (type == TGHIP_OBJ_INFINITE_SPHERE || type == TGHIP_OBJ_INFINITE_SPHERE_CAP) return c.refuse("the end cap is an infinite emitter");
    }
    // the kernels read a ray as two 16-byte vectors, a start medium as a word, and write an answer as one vector
    return c.arrays(n, (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) != 0, rays, out, "rays and out", queryAddress(rays) | queryAddress(out),
                    "device rays and answers", queryAddress(media), "device start media");
}

extern "C" int tgh_query_transmittance_check(const TgHipTransmittanceQueryDesc *desc, const void *rays, const void *media, const void *out, size_t n,
                                             const TgHostTransmittanceScene *scene, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkTransmittanceQuery(desc, rays, media, out, n, scene, error), error, err, errlen);
}
