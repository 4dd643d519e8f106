#include "VertexQuery.hpp"
#include "QueryCheck.hpp"

static_assert(sizeof(TgHipPath) == 112 && sizeof(TgHipPath) % 16 == 0, "a TgHipPath is seven 16-byte vectors");
static_assert(sizeof(TgHipVertexQueryDesc) == 32, "TgHipVertexQueryDesc is eight words");

int checkVertexQuery(const TgHipVertexQueryDesc *desc, const void *rays, const void *media, const void *paths, const void *alive, size_t n,
                     const TgHostVertexScene *scene, std::string &error)
{
    const QueryCheck c = {"tghip_query_vertex", error};
    if (!desc) return c.refuse("no description");
    int rc = c.words(desc->flags, TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_VERTEX_START, &desc->reserved, 1);
    if (rc == TGHIP_OK) rc = c.rays(n);
    if (rc != TGHIP_OK) return rc;
    if (desc->turns == 0u) return c.refuse("turns must be at least 1");
    if (desc->first_number > 1024u) return c.refuse("first_number above 1024");
    const uint32_t numMedia = scene ? scene->num_media : 0u;
    if (desc->medium < TGHIP_MEDIUM_OF_CAMERA || (desc->medium >= 0 && uint32_t(desc->medium) >= numMedia))
        return c.refuse("medium index outside the scene's table");
    if (desc->medium >= 0 && scene->medium_operand && scene->medium_operand[desc->medium])
        return c.refuse("the medium entry is an operand of an interpolated transmittance, not a medium");
    const bool start = (desc->flags & TGHIP_VERTEX_START) != 0;
    if (!start && (rays || media)) return c.refuse("rays and media are TGHIP_VERTEX_START's: without it the paths carry their rays");
    if (n == 0) return TGHIP_OK;
    if (!paths) return c.refuse("paths are needed for a batch that is not empty");
    if (start && !rays) return c.refuse("TGHIP_VERTEX_START needs rays");
    // the kernels read a ray and a state as 16-byte vectors, a start medium as a word, and the count is written as a word
    if (desc->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        if ((queryAddress(rays) | queryAddress(paths)) & 15u) return c.refuse("device rays and paths must be 16-byte aligned");
        if ((queryAddress(media) | queryAddress(alive)) & 3u) return c.refuse("device start media and alive must be 4-byte aligned");
    }
    return TGHIP_OK;
}

extern "C" int tgh_query_vertex_check(const TgHipVertexQueryDesc *desc, const void *rays, const void *media, const void *paths, const void *alive, size_t n,
                                      const TgHostVertexScene *scene, char *err, size_t errlen)
{
    std::string error;
    return queryCheckAnswer(checkVertexQuery(desc, rays, media, paths, alive, n, scene, error), error, err, errlen);
}
