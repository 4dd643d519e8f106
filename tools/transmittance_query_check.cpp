// Stand-alone sanitizer run of the host-side check of a transmittance query (tungsten_amd/csrc/host/TransmittanceQuery.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/transmittance_query_check.cpp tungsten_amd/csrc/host/TransmittanceQuery.cpp -o tools/bin/transmittance_query_check
//     tools/bin/transmittance_query_check
//
// tgh_query_transmittance_check over the boundary values: n at 0, 1, 2^31 - 1 and 2^31, alignments of the ray, the answer and the start-medium arrays,
// every flag word 0..15, the reserved words zero and each one set, bounce at 0, 255 and 256, every medium index -3 .. num_media and every end cap
// -2 .. num_objects of a small scene table -- with an operand entry, an `instances` object and two infinite emitters in it -- and of no table at all,
// with and without a description and a message buffer.  The arrays are heap blocks of 48 bytes and the tables heap blocks of exactly their size, so a
// check that walked a batch through the pointers it should only look at, or read a table past its end, would be a sanitizer report.  Every answer is
// held to the rule written out here once more.  Exit 0 without a report is the result.
#include "tungsten_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace {

long g_cases = 0, g_refused = 0;

#define REQUIRE(cond)                                                                                                \
    do {                                                                                                             \
        if (!(cond)) {                                                                                               \
            std::fprintf(stderr, "transmittance_query_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);  \
            std::exit(1);                                                                                            \
        }                                                                                                            \
    } while (0)

const uint32_t KNOWN = TGHIP_DEVELOP_DEVICE_POINTERS | TGHIP_TRANSMITTANCE_STARTS_ON_SURFACE | TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE;

// the rule of include/tungsten_hip.h, tghip_query_transmittance
bool allowed(const TgHipTransmittanceQueryDesc *d, const void *rays, const void *media, const void *out, unsigned long long n, const TgHostTransmittanceScene *s)
{
    if (!d || (d->flags & ~KNOWN) || d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return false;
    if (n > 0x7FFFFFFFull || d->bounce > 255u) return false;
    const long long numMedia = s ? s->num_media : 0, numObjects = s ? s->num_objects : 0;
    if (d->medium < -2 || d->medium >= numMedia) return false;
    if (d->medium >= 0 && s->medium_operand && s->medium_operand[d->medium]) return false;
    if (d->end_cap < -1 || d->end_cap >= numObjects) return false;
    if (d->end_cap >= 0) {
        const int32_t t = s->object_type[d->end_cap];
        if (t == TGHIP_OBJ_INSTANCES || t == TGHIP_OBJ_INFINITE_SPHERE || t == TGHIP_OBJ_INFINITE_SPHERE_CAP) return false;
    }
    if (n == 0) return true;
    if (!rays || !out) return false;
    if (!(d->flags & TGHIP_DEVELOP_DEVICE_POINTERS)) return true;
    return reinterpret_cast<uintptr_t>(rays) % 16u == 0 && reinterpret_cast<uintptr_t>(out) % 16u == 0 && reinterpret_cast<uintptr_t>(media) % 4u == 0;
}

void one(const TgHipTransmittanceQueryDesc &d, const void *rays, const void *media, const void *out, unsigned long long n, const TgHostTransmittanceScene *s)
{
    char msg[200];
    ++g_cases;
    std::memset(msg, 0x55, sizeof(msg));
    const int rc = tgh_query_transmittance_check(&d, rays, media, out, size_t(n), s, msg, sizeof(msg));
    const bool ok = allowed(&d, rays, media, out, n, s);
    REQUIRE(rc == (ok ? TGHIP_OK : TGHIP_E_INVALID));
    if (!ok) {
        ++g_refused;
        REQUIRE(std::strncmp(msg, "tghip_query_transmittance: ", 27) == 0 && std::strlen(msg) < sizeof(msg));
        char tiny[4];                           // a buffer shorter than the message: filled, terminated, not overrun
        REQUIRE(tgh_query_transmittance_check(&d, rays, media, out, size_t(n), s, tiny, sizeof(tiny)) == TGHIP_E_INVALID && std::strcmp(tiny, "tgh") == 0);
    }
    REQUIRE(tgh_query_transmittance_check(&d, rays, media, out, size_t(n), s, nullptr, 0) == rc);
}

}  // namespace

int main()
{
    static_assert(sizeof(TgHipTransmittance) == 16 && sizeof(TgHipTransmittanceQueryDesc) == 32, "layout");
    static const unsigned long long counts[] = {0ull, 1ull, 0x7FFFFFFFull, 0x80000000ull};
    // 16-byte aligned blocks (operator new gives that much on every platform this builds on; checked)
    std::unique_ptr<char[]> rayBlock(new char[48]), outBlock(new char[48]), mediaBlock(new char[48]);
    char *rayBase = rayBlock.get() + (16u - reinterpret_cast<uintptr_t>(rayBlock.get()) % 16u) % 16u;
    char *outBase = outBlock.get() + (16u - reinterpret_cast<uintptr_t>(outBlock.get()) % 16u) % 16u;
    char *mediaBase = mediaBlock.get() + (16u - reinterpret_cast<uintptr_t>(mediaBlock.get()) % 16u) % 16u;
    REQUIRE(reinterpret_cast<uintptr_t>(rayBase) % 16u == 0 && reinterpret_cast<uintptr_t>(outBase) % 16u == 0);
    // a scene of five media -- entry 1 interpolated, its operands 2 and 3 -- and seven objects
    std::unique_ptr<uint8_t[]> operand(new uint8_t[5]);
    std::unique_ptr<int32_t[]> types(new int32_t[7]);
    const uint8_t operandValues[5] = {0, 0, 1, 1, 0};
    const int32_t typeValues[7] = {TGHIP_OBJ_QUAD, TGHIP_OBJ_INSTANCES, TGHIP_OBJ_SPHERE, TGHIP_OBJ_INFINITE_SPHERE, TGHIP_OBJ_MESH, TGHIP_OBJ_INFINITE_SPHERE_CAP, TGHIP_OBJ_DISK};
    std::memcpy(operand.get(), operandValues, sizeof(operandValues));
    std::memcpy(types.get(), typeValues, sizeof(typeValues));
    const TgHostTransmittanceScene full = {5u, operand.get(), 7u, types.get()}, noOperands = {5u, nullptr, 7u, types.get()}, empty = {0u, nullptr, 0u, nullptr};
    const TgHostTransmittanceScene *tables[] = {&full, &noOperands, &empty, nullptr};

    // the description's own words and the arrays
    for (uint32_t flags = 0; flags < 16; ++flags)
        for (uint32_t reserved = 0; reserved < 5; ++reserved)           // 0: all zero, 1..4: word 0..3 set
            for (unsigned long long n : counts)
                for (int ra = 0; ra < 16; ra += (ra < 4 ? 1 : 4))
                    for (int oa = 0; oa < 16; oa += (oa < 4 ? 1 : 4))
                        for (int ma = -1; ma < 4; ++ma)                 // -1: no per-ray media
                            for (int nulls = 0; nulls < 4; ++nulls) {   // bit 0: no rays, bit 1: no out
                                if (nulls && (ra || oa)) continue;
                                TgHipTransmittanceQueryDesc d = {flags, -1, -1, 0u, {reserved == 1 ? 1u : 0u, reserved == 2 ? 0x80000000u : 0u, reserved == 3 ? 7u : 0u, reserved == 4 ? 1u : 0u}};
                                one(d, (nulls & 1) ? nullptr : rayBase + ra, ma < 0 ? nullptr : mediaBase + ma, (nulls & 2) ? nullptr : outBase + oa, n, &full);
                            }
    // the words that are read against the scene's tables
    for (const TgHostTransmittanceScene *s : tables)
        for (int32_t medium = -3; medium <= 6; ++medium)
            for (int32_t cap = -2; cap <= 8; ++cap)
                for (uint32_t bounce : {0u, 255u, 256u, 0xFFFFFFFFu})
                    for (unsigned long long n : {0ull, 1ull}) {
                        TgHipTransmittanceQueryDesc d = {TGHIP_TRANSMITTANCE_ENDS_ON_SURFACE, medium, cap, bounce, {0u, 0u, 0u, 0u}};
                        one(d, rayBase, nullptr, outBase, n, s);
                    }
    for (int32_t extreme : {int32_t(0x7FFFFFFF), int32_t(-0x7FFFFFFF - 1)}) {
        TgHipTransmittanceQueryDesc d = {0u, extreme, -1, 0u, {0u, 0u, 0u, 0u}}, e = {0u, -1, extreme, 0u, {0u, 0u, 0u, 0u}};
        one(d, rayBase, nullptr, outBase, 1, &full);
        one(e, rayBase, nullptr, outBase, 1, &full);
    }
    char msg[200];
    REQUIRE(tgh_query_transmittance_check(nullptr, rayBase, nullptr, outBase, 1, &full, msg, sizeof(msg)) == TGHIP_E_INVALID && std::strstr(msg, "no description"));
    REQUIRE(tgh_query_transmittance_check(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == TGHIP_E_INVALID);
    std::printf("transmittance_query_check: %ld calls checked: %ld refused, %ld allowed\n", g_cases + 2, g_refused + 2, g_cases - g_refused);
    return 0;
}
