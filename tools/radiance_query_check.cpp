// Stand-alone sanitizer run of the host side of tghip_query_radiance (tungsten_amd/csrc/host/RadianceQuery.cpp over PassPlan.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan tools/radiance_query_check.cpp tungsten_amd/csrc/host/RadianceQuery.cpp \
//         tungsten_amd/csrc/host/PassPlan.cpp -o tools/bin/radiance_query_check
//     tools/bin/radiance_query_check
//
// checkRadianceQuery, the virtual image and the plan of the query's pass for batches of n rays around every edge -- 0, 1, one row of the image and its
// neighbours, one tile and its neighbours, a prime, 2^16 + 1, 2^31 - 1 -- and several sample ranges, under the options a context may hold.  For each:
// the image holds the rays (w h >= n) with less than a row of padding, the pass's pixel slots walk the image so that the pixel index of ray i's slot
// is i, every batch's items and the call's samples fit 32 bits -- or the call is refused, which it must be exactly from 2^32 samples on.  Exit 0
// without a report is the result.
#include "../tungsten_amd/csrc/host/RadianceQuery.hpp"

#include <cstdio>
#include <cstdlib>

namespace {

long g_cases = 0;

#define REQUIRE(cond)                                                                                            \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "radiance_query_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);   \
            std::exit(1);                                                                                        \
        }                                                                                                        \
    } while (0)

// slotPixel (csrc/hip/pt_kernels.h) for an unsharded pass: pixel slot j of the batch -> pixel index, or -1 outside the image
int64_t pixelOfSlot(const PassPlan &p, const PassBatch &b, uint32_t w, uint32_t h, uint32_t j)
{
    const uint32_t tile = b.firstTile + (j >> 8), inTile = j & 255u;
    if (tile >= p.numTiles) return -1;
    const uint32_t x = (tile % p.tilesX)*16u + (inTile & 15u), y = (tile/p.tilesX)*16u + (inTile >> 4);
    return (x < w && y < h) ? int64_t(x) + int64_t(y)*w : -1;
}

} // namespace

int main()
{
    static const uint64_t counts[] = {0, 1, 15, 16, 17, 255, 256, 257, 997, 65537, 0x7FFFFFFFull};
    static const uint32_t ranges[][2] = {{0, 1}, {3, 4}, {0, 8}, {5, 21}, {0, 256}, {7, 7 + 65536}, {0, 0xFFFFFFFFu}};
    static const uint64_t maxItemsOf[] = {256, 4096, 1ull << 26};
    static const uint64_t maxSlotsOf[] = {2048, 1ull << 23};
    long refused = 0, planned = 0, unplanned = 0;
    PassPlan plan;                                             // reused, as the context reuses its own
    std::string error;
    char dummy[64];
    const void *aligned = reinterpret_cast<const void *>((reinterpret_cast<uintptr_t>(dummy) + 15u) & ~uintptr_t(15));
    for (uint64_t n64 : counts)
        for (const uint32_t (&range)[2] : ranges)
            for (uint32_t flags = 0; flags < 4; ++flags)
                for (uint64_t maxItems : maxItemsOf)
                    for (uint64_t maxSlots : maxSlotsOf) {
                        ++g_cases;
                        const size_t n = size_t(n64);
                        TgHipRadianceQueryDesc desc = TgHipRadianceQueryDesc();
                        desc.flags = flags; desc.seed = 0xBA5EBA11u; desc.spp_begin = range[0]; desc.spp_end = range[1]; desc.sobol_seed = 12345u;
                        const uint64_t spp = range[1] - range[0], samples = n64*spp;
                        const int rc = checkRadianceQuery(&desc, aligned, aligned, aligned, n, true, error);
                        if (n64 && samples >= (1ull << 32)) {
                            REQUIRE(rc == TGHIP_E_UNSUPPORTED && error.find("2^32 samples") != std::string::npos);
                            ++refused;
                            continue;
                        }
                        REQUIRE(rc == TGHIP_OK);
                        if (n == 0) continue;                  // (an empty batch has no image and plans nothing)
                        const RadianceQueryImage im = radianceQueryImage(n);
                        const uint64_t pixels = uint64_t(im.width)*im.height;
                        REQUIRE(im.width >= 1 && im.height >= 1 && pixels >= n64 && pixels - n64 < im.width);
                        REQUIRE(pixels <= 0x80000000ull);      // the pixel index fits the 32 bits the kernels keep it in
                        const TgHipPassDesc pass = radianceQueryPass(desc);
                        REQUIRE(pass.spp_begin == range[0] && pass.spp_end == range[1] && pass.seed == desc.seed && pass.shard_count == 1);
                        REQUIRE(pass.flags == ((flags & TGHIP_RADIANCE_SOBOL) ? TGHIP_PASS_SOBOL : 0u) && !pass.record_index && !pass.record_count);
                        const PassPlanOptions opt = {maxItems, maxSlots, 1u};
                        // (a tiny "max_items" cuts a large call into millions of batches, as it cuts a large pass: planned here up to 2^16 of them)
                        const uint64_t allItems = ((pixels + 255u)/256u)*256u*spp;
                        if (allItems/std::max<uint64_t>(maxItems, 1024u) > (1ull << 16)) { ++unplanned; continue; }
                        REQUIRE(planRadianceQuery(desc, n, opt, plan, error) == TGHIP_OK);
                        ++planned;
                        REQUIRE(!plan.empty && !plan.recordPass && !plan.auxPass && plan.chunk == 1 && plan.spp == spp && plan.sppBegin == range[0]);
                        REQUIRE(plan.tilesX == (im.width + 15)/16 && plan.tilesY == (im.height + 15)/16 && uint64_t(plan.numTiles) == uint64_t(plan.tilesX)*plan.tilesY);
                        REQUIRE(plan.totalItems == uint64_t(plan.numTiles)*256u*spp && plan.totalItems < (1ull << 41));
                        // the batches: items within 32 bits, the samples of every tile covered once, in rising order per tile
                        uint64_t items = 0;
                        for (const PassBatch &b : plan.batches) {
                            REQUIRE(b.pixSlots % 256u == 0 && b.pixSlots > 0 && b.firstTile + b.pixSlots/256u <= plan.numTiles);
                            REQUIRE(uint64_t(b.pixSlots)*b.chunks == uint64_t(b.totalItems) && uint64_t(b.totalItems) <= std::max<uint64_t>(maxItems, 256u*4u));
                            REQUIRE(b.sppBegin < b.sppEnd && b.chunks == b.sppEnd - b.sppBegin);
                            items += b.totalItems;
                        }
                        REQUIRE(items == plan.totalItems);
                        // pixel index == ray index: the first and the last 1024 slots of the first and the last batch (all slots of small images) map to
                        // their own numbers, the slots past the image to none
                        const PassBatch *ends[2] = {&plan.batches.front(), &plan.batches.back()};
                        for (const PassBatch *b : ends)
                            for (uint32_t j = 0; j < b->pixSlots; j = (j == 1023u && b->pixSlots > 2048u) ? b->pixSlots - 1024u : j + 1u) {
                                const uint64_t ray = uint64_t(b->firstTile)*256u + j;       // tiles of the one-column image follow each other in ray order
                                const int64_t pixel = pixelOfSlot(plan, *b, im.width, im.height, j);
                                REQUIRE(pixel == (ray < pixels ? int64_t(ray) : -1));
                            }
                    }
    // the refusals, each with its own message
    TgHipRadianceQueryDesc d = TgHipRadianceQueryDesc();
    d.spp_end = 1;
    REQUIRE(checkRadianceQuery(nullptr, aligned, aligned, aligned, 1, true, error) == TGHIP_E_INVALID && error.find("no description") != std::string::npos);
    REQUIRE(checkRadianceQuery(&d, nullptr, aligned, aligned, 1, true, error) == TGHIP_E_INVALID && error.find("rays and rgb_sum") != std::string::npos);
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, nullptr, 1, true, error) == TGHIP_OK);
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, aligned, size_t(0x80000000ull), true, error) == TGHIP_E_INVALID && error.find("2^31 - 1") != std::string::npos);
    d.flags = TGHIP_RADIANCE_SOBOL;
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, aligned, 1, false, error) == TGHIP_E_INVALID && error.find("sobol_matrices") != std::string::npos);
    d.flags = 4u;
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, aligned, 1, true, error) == TGHIP_E_INVALID && error.find("unknown flag") != std::string::npos);
    d.flags = 0; d.reserved[2] = 1;
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, aligned, 1, true, error) == TGHIP_E_INVALID && error.find("reserved") != std::string::npos);
    d.reserved[2] = 0; d.spp_begin = 1;
    REQUIRE(checkRadianceQuery(&d, aligned, aligned, aligned, 1, true, error) == TGHIP_E_INVALID && error.find("spp_end") != std::string::npos);
    std::printf("radiance_query_check: %ld calls: %ld planned, %ld refused for their size, %ld accepted and left unplanned\n", g_cases, planned, refused, unplanned);
    return 0;
}
