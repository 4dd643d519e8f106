// Stand-alone sanitizer run of the host-side check of a vertex query (tungsten_amd/csrc/host/VertexQuery.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/vertex_query_check.cpp tungsten_amd/csrc/host/VertexQuery.cpp -o tools/bin/vertex_query_check
//     tools/bin/vertex_query_check
//
// tgh_query_vertex_check over generated good and malformed calls -- n at 0, 1, 2^31 - 1, 2^31 and 2^40, every alignment 0..15 of the four arrays and
// NULL, every flag word 0..7 and one with a high bit, turns and first_number on either side of their limits, a reserved word that is not zero, every
// medium index of a small scene table (an interpolated medium with its operands) and of no table -- each held to the rule restated here, with the
// message checked for being a terminated string inside its buffer.  Prints one line (profiles/vertex_query/host_sanitizers.txt); any disagreement, and
// anything the sanitizers find, ends the run with a non-zero status.
#include "tungsten_host.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace {

long g_cases = 0, g_refused = 0;

#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::fprintf(stderr, "vertex_query_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);             \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)

// the rule, restated: TGHIP_OK or TGHIP_E_INVALID
int expected(const TgHipVertexQueryDesc *d, const void *rays, const void *media, const void *paths, const void *alive, unsigned long long n,
             const TgHostVertexScene *s)
{
    if (!d) return TGHIP_E_INVALID;
    if ((d->flags & ~3u) || d->reserved != 0u) return TGHIP_E_INVALID;
    if (n > 0x7FFFFFFFull) return TGHIP_E_INVALID;
    if (d->turns == 0u || d->first_number > 1024u) return TGHIP_E_INVALID;
    const long long numMedia = s ? (long long)s->num_media : 0;
    if (d->medium < -2 || d->medium >= numMedia) return TGHIP_E_INVALID;
    if (d->medium >= 0 && s->medium_operand && s->medium_operand[d->medium]) return TGHIP_E_INVALID;
    const bool start = (d->flags & TGHIP_VERTEX_START) != 0;
    if (!start && (rays || media)) return TGHIP_E_INVALID;
    if (n == 0) return TGHIP_OK;
    if (!paths || (start && !rays)) return TGHIP_E_INVALID;
    if (d->flags & TGHIP_DEVELOP_DEVICE_POINTERS) {
        if (((uintptr_t)rays & 15u) || ((uintptr_t)paths & 15u) || ((uintptr_t)media & 3u) || ((uintptr_t)alive & 3u)) return TGHIP_E_INVALID;
    }
    return TGHIP_OK;
}

void one(const TgHipVertexQueryDesc &d, const void *rays, const void *media, const void *paths, const void *alive, unsigned long long n,
         const TgHostVertexScene *s)
{
    char err[112];
    std::memset(err, 0x7F, sizeof err);
    const int rc = tgh_query_vertex_check(&d, rays, media, paths, alive, size_t(n), s, err, sizeof err);
    const int want = expected(&d, rays, media, paths, alive, n, s);
    g_cases++;
    CHECK(rc == want);
    if (rc != TGHIP_OK) {
        g_refused++;
        CHECK(std::memchr(err, 0, sizeof err) != nullptr);
        CHECK(std::strncmp(err, "tghip_query_vertex: ", 20) == 0);
    }
}

}  // namespace

int main()
{
    static_assert(sizeof(TgHipPath) == 112 && sizeof(TgHipVertexQueryDesc) == 32, "layout");
    const uint8_t operand[5] = {0, 0, 1, 1, 0};
    const TgHostVertexScene table = {5u, operand}, plain = {2u, nullptr}, empty = {0u, nullptr};
    const TgHostVertexScene *tables[] = {&table, &plain, &empty, nullptr};
    const unsigned long long counts[] = {0ull, 1ull, 0x7FFFFFFFull, 0x80000000ull, 1ull << 40};
    const uintptr_t base = 0x10000;
    // the arrays: every alignment and NULL, under every flag word
    for (unsigned long long n : counts)
        for (uint32_t flags : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 0x80000002u})
            for (int which = 0; which < 4; ++which)
                for (int a = -1; a < 16; ++a)
                    for (int withRays = 0; withRays < 2; ++withRays) {
                        const void *p[4] = {withRays ? (const void *)base : nullptr, withRays ? (const void *)base : nullptr, (const void *)base, (const void *)base};
                        p[which] = a < 0 ? nullptr : (const void *)(base + uintptr_t(a));
                        const TgHipVertexQueryDesc d = {flags, 7u, 0u, 0u, 2u, 0, 1u, 0u};
                        one(d, p[0], p[1], p[2], p[3], n, &table);
                    }
    // the description's words against every table
    for (const TgHostVertexScene *s : tables)
        for (uint32_t flags : {0u, TGHIP_VERTEX_START, TGHIP_VERTEX_START | TGHIP_DEVELOP_DEVICE_POINTERS})
            for (int medium = -4; medium <= 6; ++medium)
                for (uint32_t turns : {0u, 1u, 64u, 0xFFFFFFFFu})
                    for (uint32_t first : {0u, 2u, 1024u, 1025u, 0xFFFFFFFFu})
                        for (uint32_t reserved : {0u, 1u, 0x80000000u})
                            for (unsigned long long n : {0ull, 2ull, 0x7FFFFFFFull}) {
                                const TgHipVertexQueryDesc d = {flags, 1u, 3u, 0xFFFFFFF0u, first, medium, turns, reserved};
                                const void *rays = (flags & TGHIP_VERTEX_START) ? (const void *)base : nullptr;
                                one(d, rays, nullptr, (const void *)base, nullptr, n, s);
                            }
    for (int extreme : {INT32_MIN, INT32_MAX}) {
        const TgHipVertexQueryDesc d = {TGHIP_VERTEX_START, 1u, 0u, 0u, 2u, extreme, 1u, 0u};
        one(d, (const void *)base, nullptr, (const void *)base, nullptr, 4, &table);
    }
    // no description, and no room for a message
    CHECK(tgh_query_vertex_check(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == TGHIP_E_INVALID);
    const TgHipVertexQueryDesc bad = {8u, 0u, 0u, 0u, 0u, -1, 1u, 0u};
    char tiny[4];
    CHECK(tgh_query_vertex_check(&bad, nullptr, nullptr, (const void *)base, nullptr, 1, nullptr, tiny, sizeof tiny) == TGHIP_E_INVALID && tiny[3] == 0);
    std::printf("vertex_query_check: %ld calls checked: %ld refused, %ld allowed\n", g_cases + 2, g_refused + 2, g_cases - g_refused);
    return 0;
}
