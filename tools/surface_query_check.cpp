// Stand-alone sanitizer run of the host-side check of a surface query (tungsten_amd/csrc/host/SurfaceQuery.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/surface_query_check.cpp tungsten_amd/csrc/host/SurfaceQuery.cpp -o tools/bin/surface_query_check
//     tools/bin/surface_query_check
//
// tgh_query_surface_check over the boundary values: n at 0, 1, 2^31 - 1 and 2^31, every alignment 0..15 of the ray and of the answer array, every flag
// word 0..7, the reserved words zero and each one set, with and without a description and a message buffer.  The arrays are heap blocks of 48 bytes --
// less than two rays, half an answer --, so a check that walked a batch through the pointers it should only look at would be a sanitizer report.
// Every answer is held to the rule written out here once more.  Exit 0 without a report is the result.
#include "tungsten_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace {

long g_cases = 0, g_refused = 0;

#define REQUIRE(cond)                                                                                          \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            std::fprintf(stderr, "surface_query_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);  \
            std::exit(1);                                                                                      \
        }                                                                                                      \
    } while (0)

// the rule of include/tungsten_hip.h, tghip_query_surface
bool allowed(const TgHipSurfaceQueryDesc *d, const void *rays, const void *out, unsigned long long n)
{
    if (!d || (d->flags & ~TGHIP_DEVELOP_DEVICE_POINTERS) || d->reserved[0] || d->reserved[1] || d->reserved[2]) return false;
    if (n > 0x7FFFFFFFull) return false;
    if (n == 0) return true;
    if (!rays || !out) return false;
    if (!(d->flags & TGHIP_DEVELOP_DEVICE_POINTERS)) return true;
    return reinterpret_cast<uintptr_t>(rays) % 16u == 0 && reinterpret_cast<uintptr_t>(out) % 16u == 0;
}

}  // namespace

int main()
{
    static_assert(sizeof(TgHipSurface) == 96 && sizeof(TgHipSurfaceQueryDesc) == 16, "layout");
    static const unsigned long long counts[] = {0ull, 1ull, 0x7FFFFFFFull, 0x80000000ull};
    // 16-byte aligned blocks (operator new gives that much on every platform this builds on; checked)
    std::unique_ptr<char[]> rayBlock(new char[48]), outBlock(new char[48]);
    char *rayBase = rayBlock.get() + (16u - reinterpret_cast<uintptr_t>(rayBlock.get()) % 16u) % 16u;
    char *outBase = outBlock.get() + (16u - reinterpret_cast<uintptr_t>(outBlock.get()) % 16u) % 16u;
    REQUIRE(reinterpret_cast<uintptr_t>(rayBase) % 16u == 0 && reinterpret_cast<uintptr_t>(outBase) % 16u == 0);
    char msg[160];
    for (uint32_t flags = 0; flags < 8; ++flags)
        for (uint32_t reserved = 0; reserved < 4; ++reserved)           // 0: all zero, 1 / 2 / 3: word 0 / 1 / 2 set
            for (unsigned long long n : counts)
                for (int ra = 0; ra < 16; ++ra)
                    for (int oa = 0; oa < 16; ++oa)
                        for (int nulls = 0; nulls < 4; ++nulls) {       // bit 0: no rays, bit 1: no out
                            if (nulls && (ra || oa)) continue;
                            ++g_cases;
                            TgHipSurfaceQueryDesc d = {flags, {reserved == 1 ? 1u : 0u, reserved == 2 ? 0x80000000u : 0u, reserved == 3 ? 7u : 0u}};
                            const void *rays = (nulls & 1) ? nullptr : rayBase + ra, *out = (nulls & 2) ? nullptr : outBase + oa;
                            std::memset(msg, 0x55, sizeof(msg));
                            const int rc = tgh_query_surface_check(&d, rays, out, size_t(n), msg, sizeof(msg));
                            const bool ok = allowed(&d, rays, out, n);
                            REQUIRE(rc == (ok ? TGHIP_OK : TGHIP_E_INVALID));
                            if (!ok) {
                                ++g_refused;
                                REQUIRE(std::strncmp(msg, "tghip_query_surface: ", 21) == 0 && std::strlen(msg) < sizeof(msg));
                                char tiny[4];                           // a buffer shorter than the message: filled, terminated, not overrun
                                REQUIRE(tgh_query_surface_check(&d, rays, out, size_t(n), tiny, sizeof(tiny)) == TGHIP_E_INVALID && std::strcmp(tiny, "tgh") == 0);
                            }
                            REQUIRE(tgh_query_surface_check(&d, rays, out, size_t(n), nullptr, 0) == rc);
                        }
    REQUIRE(tgh_query_surface_check(nullptr, rayBase, outBase, 1, msg, sizeof(msg)) == TGHIP_E_INVALID && std::strstr(msg, "no description"));
    REQUIRE(tgh_query_surface_check(nullptr, nullptr, nullptr, 0, nullptr, 0) == TGHIP_E_INVALID);
    std::printf("surface_query_check: %ld calls checked: %ld refused, %ld allowed\n", g_cases + 2, g_refused + 2, g_cases - g_refused);
    return 0;
}
