// Stand-alone sanitizer run of the host-side check of a direct-lighting query (tungsten_amd/csrc/host/DirectQuery.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/direct_query_check.cpp tungsten_amd/csrc/host/DirectQuery.cpp -o tools/bin/direct_query_check
//     tools/bin/direct_query_check
//
// tgh_query_direct_check over generated good and malformed calls -- n at 0, 1, 2^31 - 1, 2^31 and 2^40, every alignment 0..15 of the three arrays and
// NULL, every flag word 0..7 and one with a high bit, sample ranges empty, reversed, of one and of 2^32 - 1 samples, skip and bounce on either side of
// their limits, every light and medium index of a small scene table (an interpolated medium with its operands, the camera in a medium or in none) and of
// no table -- each held to the rule restated here, with the message checked for being a terminated string inside its buffer.  Prints one line
// (profiles/direct_query/host_sanitizers.txt); any disagreement, and anything the sanitizers find, ends the run with a non-zero status.
#include "tungsten_host.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace {

long g_cases = 0, g_refused = 0, g_unsupported = 0;

#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::fprintf(stderr, "direct_query_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);             \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)

// the rule, restated: TGHIP_OK, TGHIP_E_INVALID or TGHIP_E_UNSUPPORTED
int expected(const TgHipDirectQueryDesc *d, const void *rays, const void *media, const void *out, unsigned long long n, const TgHostDirectScene *s)
{
    if (!d) return TGHIP_E_INVALID;
    if (d->flags & ~3u) return TGHIP_E_INVALID;
    if (n > 0x7FFFFFFFull) return TGHIP_E_INVALID;
    if (d->spp_end <= d->spp_begin || d->skip > 1024u || d->bounce > 255u) return TGHIP_E_INVALID;
    const long long lights = s ? (long long)s->num_lights : 0, numMedia = s ? (long long)s->num_media : 0;
    if (d->light < -1 || d->light >= lights) return TGHIP_E_INVALID;
    if (d->medium < -2 || d->medium >= numMedia) return TGHIP_E_INVALID;
    if (d->medium >= 0 && s->medium_operand && s->medium_operand[d->medium]) return TGHIP_E_INVALID;
    if ((d->flags & TGHIP_DIRECT_VOLUME) && !media) {
        const int resolved = d->medium == TGHIP_MEDIUM_OF_CAMERA ? (s ? s->camera_medium : -1) : d->medium;
        if (resolved < 0) return TGHIP_E_INVALID;
    }
    if (n == 0) return TGHIP_OK;
    if (!rays || !out) return TGHIP_E_INVALID;
    if (d->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        if (((uintptr_t)rays & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)media & 3u)) return TGHIP_E_INVALID;
    }
    if (n*(unsigned long long)(d->spp_end - d->spp_begin) >= (1ull << 32)) return TGHIP_E_UNSUPPORTED;
    return TGHIP_OK;
}

void one(const TgHipDirectQueryDesc &d, const void *rays, const void *media, const void *out, unsigned long long n, const TgHostDirectScene *s)
{
    char err[96];
    std::memset(err, 0x7F, sizeof err);
    const int rc = tgh_query_direct_check(&d, rays, media, out, size_t(n), s, err, sizeof err);
    const int want = expected(&d, rays, media, out, n, s);
    g_cases++;
    CHECK(rc == want);
    if (rc != TGHIP_OK) {
        (rc == TGHIP_E_UNSUPPORTED ? g_unsupported : g_refused)++;
        CHECK(std::memchr(err, 0, sizeof err) != nullptr);
        CHECK(std::strncmp(err, "tghip_query_direct: ", 20) == 0);
    }
}

}  // namespace

int main()
{
    static_assert(sizeof(TgHipDirect) == 32 && sizeof(TgHipDirectQueryDesc) == 32, "layout");
    const uint8_t operand[5] = {0, 0, 1, 1, 0};
    const TgHostDirectScene inMedium = {5u, operand, 3u, 4}, inNone = {5u, operand, 3u, -1}, plain = {2u, nullptr, 1u, 0}, empty = {0u, nullptr, 0u, -1};
    const TgHostDirectScene *tables[] = {&inMedium, &inNone, &plain, &empty, nullptr};
    const unsigned long long counts[] = {0ull, 1ull, 0x7FFFFFFFull, 0x80000000ull, 1ull << 40};
    const uintptr_t base = 0x10000;
    // the arrays: every alignment and NULL, under every flag word
    for (unsigned long long n : counts)
        for (uint32_t flags : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 0x80000001u})
            for (int which = 0; which < 3; ++which)
                for (int a = -1; a < 16; ++a) {
                    const void *p[3] = {(const void *)base, (const void *)base, (const void *)base};
                    p[which] = a < 0 ? nullptr : (const void *)(base + uintptr_t(a));
                    const TgHipDirectQueryDesc d = {flags, 7u, 0u, 2u, 0, 1u, -1, 0u};
                    one(d, p[0], p[1], p[2], n, &inMedium);
                }
    // the description's words against every table
    const uint32_t ranges[][2] = {{0u, 1u}, {0u, 0u}, {5u, 2u}, {3u, 4u}, {0u, 0xFFFFFFFFu}, {0xFFFFFFFEu, 0xFFFFFFFFu}, {0u, 2u}, {0u, 0x80000000u}};
    for (const TgHostDirectScene *s : tables)
        for (uint32_t flags : {0u, TGHIP_DIRECT_VOLUME, TGHIP_DIRECT_VOLUME | TGHIP_DEVELOP_DEVICE_POINTERS})
            for (const void *media : {(const void *)nullptr, (const void *)base})
                for (const uint32_t (&r)[2] : ranges)
                    for (int medium = -4; medium <= 6; ++medium)
                        for (int light = -3; light <= 4; ++light)
                            for (uint32_t skip : {0u, 1024u, 1025u})
                                for (uint32_t bounce : {0u, 255u, 256u})
                                    for (unsigned long long n : {0ull, 2ull, 0x7FFFFFFFull}) {
                                        const TgHipDirectQueryDesc d = {flags, 1u, r[0], r[1], medium, bounce, light, skip};
                                        one(d, (const void *)base, media, (const void *)base, n, s);
                                    }
    for (int extreme : {INT32_MIN, INT32_MAX}) {
        const TgHipDirectQueryDesc d = {0u, 1u, 0u, 1u, extreme, 1u, -1, 0u}, e = {0u, 1u, 0u, 1u, -1, 1u, extreme, 0u};
        one(d, (const void *)base, nullptr, (const void *)base, 4, &inMedium);
        one(e, (const void *)base, nullptr, (const void *)base, 4, &inMedium);
    }
    // no description, and no room for a message
    CHECK(tgh_query_direct_check(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == TGHIP_E_INVALID);
    const TgHipDirectQueryDesc bad = {8u, 0u, 0u, 1u, -1, 1u, -1, 0u};
    char tiny[4];
    CHECK(tgh_query_direct_check(&bad, (const void *)base, nullptr, (const void *)base, 1, nullptr, tiny, sizeof tiny) == TGHIP_E_INVALID && tiny[3] == 0);
    std::printf("direct_query_check: %ld calls checked: %ld refused, %ld unsupported, %ld allowed\n", g_cases + 2, g_refused + 2, g_unsupported,
                g_cases - g_refused - g_unsupported);
    return 0;
}
