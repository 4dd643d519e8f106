// Stand-alone sanitizer run of the host-side pass plan (tungsten_amd/csrc/host/PassPlan.cpp), no device and no Python:
//
//     g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/pass_plan_check.cpp tungsten_amd/csrc/host/PassPlan.cpp -o tools/bin/pass_plan_check
//     tools/bin/pass_plan_check
//
// planPass over a fixed-seed grid of small images, shard counts, options and random per-record sample counts (zeros among them).  The input arrays
// are heap blocks of exactly their size, so a read past a record array is a sanitizer report.  Every case is planned twice -- into ONE plan object
// reused through the whole run, as the context reuses its own, and into a fresh one -- and the two must agree field by field.  The partition properties
// are re-checked here: the shards' tile lists partition the tiles, the batches of a plain pass cover (owned tile x sample index) once, the batches of a
// record pass tile the gap-free enumeration at group boundaries, `sorted` is the owned records with a count above 0 by descending count with ties in
// record order.  Exit 0 without a report is the result.
#include "../tungsten_amd/csrc/host/PassPlan.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)      // [0, n)
{
    g_state = g_state*6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((g_state >> 33) % n);
}

long g_cases = 0;

#define REQUIRE(cond)                                                                                       \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::fprintf(stderr, "pass_plan_check: case %ld, line %d: %s\n", g_cases, __LINE__, #cond);   \
            std::exit(1);                                                                                   \
        }                                                                                                   \
    } while (0)

bool sameBatch(const PassBatch &a, const PassBatch &b)
{
    return a.sppBegin == b.sppBegin && a.sppEnd == b.sppEnd && a.chunks == b.chunks && a.pixSlots == b.pixSlots && a.totalItems == b.totalItems &&
           a.firstTile == b.firstTile && a.itemBase == b.itemBase;
}

// what a reader of the plan looks at, given its flags
void requireSame(const PassPlan &a, const PassPlan &b)
{
    REQUIRE(a.empty == b.empty && a.tilesX == b.tilesX && a.tilesY == b.tilesY && a.numTiles == b.numTiles);
    REQUIRE(a.shardCount == b.shardCount && a.shardSkew == b.shardSkew && a.ownedTiles == b.ownedTiles);
    if (a.shardCount > 1) REQUIRE(a.ownedList == b.ownedList);
    REQUIRE(a.recordPass == b.recordPass && a.varianceW == b.varianceW && a.numRecords == b.numRecords);
    REQUIRE(a.spp == b.spp && a.sppBegin == b.sppBegin && a.auxPass == b.auxPass && a.lumFloats == b.lumFloats);
    if (a.recordPass) REQUIRE(a.recIndex == b.recIndex && a.recCount == b.recCount && a.recLum == b.recLum);
    REQUIRE(a.batches.size() == b.batches.size() && a.totalItems == b.totalItems && a.batchItems == b.batchItems && a.shortBatch == b.shortBatch);
    REQUIRE(a.chunk == b.chunk && a.group == b.group && a.chunksAll == b.chunksAll);
    if (a.empty) return;
    for (size_t i = 0; i < a.batches.size(); ++i) REQUIRE(sameBatch(a.batches[i], b.batches[i]));
    if (a.recordPass) REQUIRE(a.sorted == b.sorted && a.chunkStart == b.chunkStart && a.recordItems == b.recordItems && a.hintEntries == b.hintEntries);
}

void checkPlain(const PassPlan &p, const TgHipPassDesc &pass, uint64_t maxItems)
{
    const uint32_t spp = pass.spp_end - pass.spp_begin;
    std::vector<uint8_t> seen(size_t(p.ownedTiles)*spp, 0);
    for (const PassBatch &b : p.batches) {
        REQUIRE(b.pixSlots % 256u == 0 && b.pixSlots > 0 && b.itemBase == 0);
        REQUIRE(pass.spp_begin <= b.sppBegin && b.sppBegin < b.sppEnd && b.sppEnd <= pass.spp_end);
        REQUIRE(b.firstTile + b.pixSlots/256u <= p.ownedTiles);
        REQUIRE(b.chunks == (b.sppEnd - b.sppBegin + p.chunk - 1)/p.chunk && (b.chunks % p.group == 0 || b.sppEnd == pass.spp_end));
        REQUIRE(uint64_t(b.totalItems) == uint64_t(b.pixSlots)*b.chunks && b.totalItems <= p.batchItems);
        REQUIRE(b.totalItems <= maxItems || (b.pixSlots == 256u && b.chunks <= p.group));
        for (uint32_t t = b.firstTile; t < b.firstTile + b.pixSlots/256u; ++t)
            for (uint32_t s = b.sppBegin; s < b.sppEnd; ++s)
                seen[size_t(t)*spp + (s - pass.spp_begin)]++;
    }
    for (uint8_t n : seen) REQUIRE(n == 1);
}

void checkRecords(const PassPlan &p, const TgHipPassDesc &pass, uint64_t maxItems)
{
    const uint32_t shardCount = pass.shard_count ? pass.shard_count : 1;
    std::vector<uint8_t> owned(p.numRecords);
    uint64_t lum = 0;
    for (uint32_t r = 0; r < p.numRecords; ++r) {
        const uint32_t rx = r % p.varianceW, ry = r/p.varianceW;
        owned[r] = tghip_tile_owner(rx/4, ry/4, shardCount) == pass.shard_index;
        REQUIRE(p.recLum[r] == lum);
        if (owned[r]) lum += 16ull*p.recCount[r];
    }
    REQUIRE(lum == p.lumFloats);
    if (p.empty) return;
    // sorted: each owned record with a count above 0 once, descending, ties in record order
    std::vector<uint8_t> listed(p.numRecords, 0);
    for (size_t i = 0; i < p.sorted.size(); ++i) {
        const uint32_t r = p.sorted[i];
        REQUIRE(r < p.numRecords && owned[r] && p.recCount[r] > 0 && !listed[r]);
        listed[r] = 1;
        if (i) REQUIRE(p.recCount[p.sorted[i - 1]] > p.recCount[r] || (p.recCount[p.sorted[i - 1]] == p.recCount[r] && p.sorted[i - 1] < r));
    }
    for (uint32_t r = 0; r < p.numRecords; ++r) REQUIRE(listed[r] == (owned[r] && p.recCount[r] > 0));
    // chunk starts: chunk c holds 16 items per owned record with more than c*chunk samples
    REQUIRE(p.chunkStart.size() == size_t(p.chunksAll) + 2 && p.chunkStart[0] == 0 && p.chunkStart[p.chunksAll + 1] == 0xFFFFFFFFu);
    for (uint32_t c = 0; c < p.chunksAll; ++c) {
        uint32_t alive = 0;
        for (uint32_t r = 0; r < p.numRecords; ++r) alive += owned[r] && p.recCount[r] > uint64_t(c)*p.chunk;
        REQUIRE(p.chunkStart[c + 1] - p.chunkStart[c] == alive*16u);
    }
    REQUIRE(p.chunkStart[p.chunksAll] == p.recordItems && p.hintEntries == size_t((p.recordItems + 63)/64) + 1);
    // batches: [0, recordItems) in consecutive ranges that end on group boundaries
    // (every chunk below chunksAll holds an item -- spp is the largest owned count --, so the starts rise strictly)
    uint64_t at = 0;
    uint32_t c = 0;                                            // the group boundary `at` lies on: chunkStart[min(c, chunksAll)] == at
    for (size_t i = 0; i < p.batches.size(); ++i) {
        const PassBatch &b = p.batches[i];
        REQUIRE(b.itemBase == at && b.totalItems > 0 && b.sppBegin == 0 && b.sppEnd == p.spp && b.chunks == p.chunksAll);
        at += b.totalItems;
        uint32_t groups = 0;
        while (c < p.chunksAll && p.chunkStart[std::min(c, p.chunksAll)] < at) { c += p.group; ++groups; }
        REQUIRE(p.chunkStart[std::min(c, p.chunksAll)] == at);
        if (b.totalItems > maxItems) REQUIRE(groups == 1);     // more than max_items: one group only
        if (i + 1 < p.batches.size())                          // ... and as many groups as fit
            REQUIRE(p.chunkStart[std::min(c + p.group, p.chunksAll)] - b.itemBase > maxItems);
        REQUIRE(b.totalItems <= p.batchItems);
    }
    REQUIRE(at == p.recordItems && p.totalItems == p.recordItems);
}

} // namespace

int main()
{
    static const uint32_t sizes[][2] = {{8, 8}, {16, 16}, {40, 24}, {33, 17}, {64, 48}, {100, 36}};
    static const uint64_t maxItemsOf[] = {256, 1024, 1ull << 26};
    static const uint32_t chunkOf[] = {0, 1, 2, 4};
    PassPlan reused;
    long refused = 0, empty = 0;
    std::string error;
    for (size_t si = 0; si < sizeof(sizes)/sizeof(sizes[0]); ++si) {
        const uint32_t w = sizes[si][0], h = sizes[si][1];
        const uint32_t numTiles = ((w + 15)/16)*((h + 15)/16), numRecords = ((w + 3)/4)*((h + 3)/4);
        const uint32_t shardCounts[] = {0, 1, 2, 3, 8, 15, numTiles + 1};
        for (uint32_t shardCount : shardCounts) {
            // the shards' lists partition the tiles
            std::vector<uint8_t> tileSeen(numTiles, 0);
            for (uint32_t shard = 0; shard < std::max(shardCount, 1u); ++shard) {
                for (int round = 0; round < 12; ++round) {
                    ++g_cases;
                    TgHipPassDesc pass = TgHipPassDesc();
                    pass.spp_begin = rnd(9);
                    pass.spp_end = pass.spp_begin + (rnd(4) ? rnd(18) : 0u);
                    pass.shard_index = shard; pass.shard_count = shardCount;
                    const uint32_t kind = rnd(4);              // 0: plain, 1: aux, 2: uniform records, 3: per-record counts
                    pass.flags = kind == 1 ? TGHIP_PASS_AUX : kind >= 2 ? TGHIP_PASS_RECORDS : 0u;
                    // (new[]: blocks of exactly numRecords entries)
                    std::unique_ptr<uint32_t[]> index(new uint32_t[numRecords]), count(new uint32_t[numRecords]);
                    if (kind == 3) {
                        const uint32_t top = rnd(3) == 0 ? 1u : rnd(2) ? 24u : 70000u;      // (70000: past the 2^16 switch of the sort)
                        for (uint32_t r = 0; r < numRecords; ++r) { index[r] = rnd(1000); count[r] = rnd(3) ? rnd(top) : 0u; }
                        pass.record_index = index.get(); pass.record_count = count.get();
                    }
                    const PassPlanOptions opt = {maxItemsOf[rnd(3)], rnd(2) ? (1ull << 23) : 2048ull, chunkOf[rnd(4)]};
                    REQUIRE(checkPass(pass, w, h, false, error) == TGHIP_OK);
                    PassPlan fresh;
                    const int rc = planPass(pass, w, h, opt, fresh, error);
                    REQUIRE(planPass(pass, w, h, opt, reused, error) == rc);
                    if (rc != TGHIP_OK) { REQUIRE(rc == TGHIP_E_UNSUPPORTED); ++refused; continue; }
                    requireSame(reused, fresh);
                    REQUIRE(fresh.shortBatch == (!fresh.empty && 2u*fresh.batchItems <= opt.maxSlots));
                    if (shardCount > 1 && round == 0)
                        for (uint32_t t : fresh.ownedList) { REQUIRE(t < numTiles && !tileSeen[t]); tileSeen[t] = 1; }
                    for (size_t i = 1; shardCount > 1 && i < fresh.ownedList.size(); ++i) REQUIRE(fresh.ownedList[i - 1] < fresh.ownedList[i]);
                    REQUIRE(fresh.ownedTiles == (shardCount > 1 ? uint32_t(fresh.ownedList.size()) : numTiles));
                    if (fresh.empty) { REQUIRE(fresh.batches.empty()); ++empty; }
                    if (kind >= 2) checkRecords(fresh, pass, std::max<uint64_t>(opt.maxItems, 256));
                    else if (!fresh.empty) checkPlain(fresh, pass, std::max<uint64_t>(opt.maxItems, 256));
                }
            }
            if (shardCount > 1)
                for (uint8_t s : tileSeen) REQUIRE(s == 1);
        }
    }
    // a sample range that ends near 2^32: the batches' 32-bit sample counter must not wrap back below the range's end (a plan without end), and the
    // batches must cover the range once, in order
    {
        ++g_cases;
        TgHipPassDesc pass = TgHipPassDesc();
        pass.spp_begin = 5; pass.spp_end = 0xFFFFFFFFu; pass.shard_count = 1;
        const PassPlanOptions opt = {1ull << 26, 1ull << 23, 0};
        REQUIRE(planPass(pass, 16, 16, opt, reused, error) == TGHIP_OK && !reused.empty && reused.batches.size() < (1u << 20));
        uint64_t at = pass.spp_begin;
        for (const PassBatch &b : reused.batches) { REQUIRE(b.sppBegin == at && b.sppEnd > b.sppBegin && b.firstTile == 0 && b.pixSlots == 256u); at = b.sppEnd; }
        REQUIRE(at == pass.spp_end);
    }
    std::printf("pass_plan_check: %ld passes planned: %ld empty, %ld refused\n", g_cases, empty, refused);
    return 0;
}
