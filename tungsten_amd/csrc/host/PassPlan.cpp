#include "PassPlan.hpp"

#include <algorithm>

int checkPass(const TgHipPassDesc &pass, uint32_t w, uint32_t h, bool sceneHasSobol, std::string &error)
{
    if (pass.spp_end < pass.spp_begin || (pass.shard_count && pass.shard_index >= pass.shard_count)) {
        error = "invalid pass description";
        return TGHIP_E_INVALID;
    }
    if (pass.flags & ~(TGHIP_PASS_SOBOL | TGHIP_PASS_RECORDS | TGHIP_PASS_AUX | TGHIP_PASS_SAMPLES)) { error = "unknown pass flags"; return TGHIP_E_INVALID; }
    if ((pass.flags & TGHIP_PASS_SOBOL) && (!sceneHasSobol || !pass.tile_seeds)) {
        error = "TGHIP_PASS_SOBOL needs sobol_matrices in the scene description and tile_seeds in the pass";
        return TGHIP_E_INVALID;
    }
    if ((pass.record_count != nullptr) != (pass.record_index != nullptr) || (pass.record_count && !(pass.flags & TGHIP_PASS_RECORDS))) {
        error = "record_index and record_count go together and need TGHIP_PASS_RECORDS";
        return TGHIP_E_INVALID;
    }
    if ((pass.flags & TGHIP_PASS_SAMPLES) && (pass.record_count || uint64_t(w)*h*(pass.spp_end - pass.spp_begin)*3u >= (1ull << 31))) {
        error = "TGHIP_PASS_SAMPLES keeps W*H*spp*3 floats (< 2^31) and does not combine with per-record sample counts";
        return TGHIP_E_INVALID;
    }
    return TGHIP_OK;
}

int planPass(const TgHipPassDesc &pass, uint32_t w, uint32_t h, const PassPlanOptions &opt, PassPlan &out, std::string &error)
{
    out.empty = true;
    out.batches.clear();
    out.totalItems = out.batchItems = 0;
    out.shortBatch = false;
    out.chunk = out.group = out.chunksAll = 0;
    const uint32_t shardCount = pass.shard_count ? pass.shard_count : 1;
    const uint32_t tilesX = (w + 15)/16, tilesY = (h + 15)/16;
    const uint32_t numTiles = tilesX*tilesY;
    out.shardCount = shardCount;
    out.tilesX = tilesX; out.tilesY = tilesY; out.numTiles = numTiles;
    // the shard's tiles (tghip_tile_owner: a diagonal interleave), row-major; the device indexes this list (PassParams::owned_tiles)
    out.shardSkew = tghip_shard_skew(shardCount);
    auto ownsTile = [&](uint32_t tx, uint32_t ty) { return tghip_tile_owner(tx, ty, shardCount) == pass.shard_index; };
    uint32_t ownedTiles = numTiles;
    if (shardCount > 1) {
        if (out.ownedKey[0] != w || out.ownedKey[1] != h || out.ownedKey[2] != pass.shard_index || out.ownedKey[3] != shardCount) {
            std::vector<uint32_t> &list = out.ownedList;
            list.clear();
            for (uint32_t ty = 0; ty < tilesY; ++ty)
                for (uint32_t tx = 0; tx < tilesX; ++tx)
                    if (ownsTile(tx, ty)) list.push_back(tx + ty*tilesX);
            out.ownedKey[0] = w; out.ownedKey[1] = h; out.ownedKey[2] = pass.shard_index; out.ownedKey[3] = shardCount;
            out.ownedStale = true;
        }
        ownedTiles = uint32_t(out.ownedList.size());
    }
    out.ownedTiles = ownedTiles;
    uint32_t spp = pass.spp_end - pass.spp_begin, sppBegin = pass.spp_begin;
    const bool recordPass = (pass.flags & TGHIP_PASS_RECORDS) != 0;
    const uint32_t varianceW = (w + 3)/4;
    const uint32_t numRecords = varianceW*((h + 3)/4);
    out.recordPass = recordPass;
    out.varianceW = varianceW; out.numRecords = numRecords;
    out.lumFloats = 0;
    out.recordItems = 0;
    out.hintEntries = 0;
    if (recordPass) {
        // per record: first sample index, samples per pixel, offset of its 16 x count luminance block.  The sample
        // range of the batches below becomes relative to each record's first index: [0, max count of an owned record).
        std::vector<uint32_t> &idx = out.recIndex, &cnt = out.recCount, &off = out.recLum;
        idx.resize(numRecords); cnt.resize(numRecords); off.resize(numRecords);
        uint64_t total = 0;
        uint32_t maxCount = 0;
        for (uint32_t r = 0; r < numRecords; ++r) {
            uint32_t rx = r % varianceW, ry = r/varianceW;
            bool owned = ownsTile(rx >> 2, ry >> 2);
            idx[r] = pass.record_index ? pass.record_index[r] : pass.spp_begin;
            cnt[r] = pass.record_count ? pass.record_count[r] : spp;
            off[r] = uint32_t(total);
            if (owned) {
                total += uint64_t(cnt[r])*16u;
                maxCount = std::max(maxCount, cnt[r]);
            }
            if (total >= (1ull << 32)) {
                error = "pass too large for SampleRecord keeping (more than 2^32 samples per device): lower spp_step";
                return TGHIP_E_UNSUPPORTED;
            }
        }
        spp = maxCount;
        sppBegin = 0;
        out.lumFloats = total;
    }
    out.spp = spp; out.sppBegin = sppBegin;
    const uint32_t sppEnd = sppBegin + spp;
    // TGHIP_PASS_AUX: one work item per pixel, so that a pixel's samples reach OutputBuffer::addSample in index order (auxAdd)
    out.auxPass = (pass.flags & TGHIP_PASS_AUX) != 0;
    if (ownedTiles == 0 || spp == 0)
        return TGHIP_OK;

    // Samples per work item: 4 when the pass is long (256 spp at 720p: 59 M items over 8 M slots) -- but a slot works its item's samples
    // off one after the other, so a SHORT pass cut into 4-sample items is a few long sequential chains on a half-empty pool: the 16-spp
    // passes of the as-shipped materialtest (3.7 M items) ran at half the throughput of one 256-spp pass.  Such passes -- and one rank's
    // share of a multi-GPU render -- get smaller items, down to one sample each, so that the items outnumber the slots about twice.
    uint32_t chunk = out.auxPass ? std::max(spp, 1u) : opt.chunkSamples;
    if (chunk == 0) {
        uint64_t passSamples = 0;
        if (recordPass) {
            uint64_t c16 = 0;
            for (uint32_t r = 0; r < numRecords; ++r) {
                const uint32_t rx = r % varianceW, ry = r/varianceW;
                if (ownsTile(rx >> 2, ry >> 2)) c16 += out.recCount[r];
            }
            passSamples = c16*16u;
        } else {
            passSamples = uint64_t(ownedTiles)*256u*spp;
        }
        // One sample or four, nothing in between: k_resolve adds one-sample items up in groups of four, so both choices -- and with them
        // the unsharded pass and every shard of it, which pick by their OWN sample counts -- round a pixel's sum alike (pt_wavefront.h:
        // k_resolve; tests/test_gpu_parity.py::test_shards_and_batches_round_like_the_whole_pass).  An explicit "chunk_samples" of 2 or 3
        // gives up that property, not the result's validity.
        chunk = (passSamples >> 24) >= 3 ? 4u : 1u;
    }
    const uint32_t group = chunk == 1u ? 4u : 1u;
    out.chunk = chunk; out.group = group;
    const uint64_t maxItems = std::max<uint64_t>(opt.maxItems, 256);
    uint64_t recordItems = 0;
    if (recordPass) {
        // Gap-free work items for uneven per-record sample counts (PassParams): owned records sorted by descending count,
        // chunk c covers the first chunkStart[c + 1] - chunkStart[c] pixel slots of that order.
        std::vector<uint32_t> &sorted = out.sorted, &start = out.chunkStart;
        const std::vector<uint32_t> &cnt = out.recCount;
        sorted.clear();
        for (uint32_t r = 0; r < numRecords; ++r) {
            uint32_t rx = r % varianceW, ry = r/varianceW;
            if (ownsTile(rx >> 2, ry >> 2) && cnt[r] > 0)
                sorted.push_back(r);
        }
        // descending by count, ties in record order (a counting sort: the counts of a pass are small integers)
        if (spp < (1u << 16)) {
            std::vector<uint32_t> &bucket = out.bucket;
            bucket.assign(size_t(spp) + 2, 0u);
            for (uint32_t r : sorted) bucket[spp - cnt[r] + 1]++;
            for (size_t i = 1; i < bucket.size(); ++i) bucket[i] += bucket[i - 1];
            std::vector<uint32_t> &tmp = out.sortTmp;
            tmp.resize(sorted.size());
            for (uint32_t r : sorted) tmp[bucket[spp - cnt[r]]++] = r;
            sorted.swap(tmp);
        } else {
            std::stable_sort(sorted.begin(), sorted.end(), [&cnt](uint32_t a, uint32_t b) { return cnt[a] > cnt[b]; });
        }
        const uint32_t numChunks = (spp + chunk - 1)/chunk;
        start.assign(size_t(numChunks) + 2, 0u);
        size_t alive = sorted.size();                // records with cnt > c*chunk: a prefix of `sorted`
        for (uint32_t c = 0; c < numChunks; ++c) {
            while (alive > 0 && cnt[sorted[alive - 1]] <= uint64_t(c)*chunk) --alive;
            recordItems += uint64_t(alive)*16u;
            if (recordItems >= (1ull << 32)) {
                error = "pass too large for SampleRecord keeping (more than 2^32 work items per device): lower spp_step";
                return TGHIP_E_UNSUPPORTED;
            }
            start[c + 1] = uint32_t(recordItems);
        }
        start[numChunks + 1] = 0xFFFFFFFFu;          // sentinel for the device's `while (w >= start[c + 1])`
        // (the hint table -- for every 64 items the chunk their first one lies in, 230 k entries for a 16-spp pass at 720p -- is filled by a launch
        // from the chunk starts: building and uploading it on the host was a third of the host's set-up time between two passes)
        out.hintEntries = size_t((recordItems + 63)/64) + 1;
        out.recordItems = recordItems;
        if (recordItems == 0)
            return TGHIP_OK;
    }

    // Batches: work items = (pixel slot of an owned tile) x (chunk of `chunk` sample indices).  One batch
    // holds at most maxItems items (16 B of partial sum each); larger passes are split by sample range first,
    // then by tiles.  (Record passes: consecutive ranges of the gap-free enumeration above.)
    const uint32_t chunksAll = (spp + chunk - 1)/chunk;
    out.chunksAll = chunksAll;
    uint32_t tilesPerBatch = ownedTiles, chunksPerBatch = chunksAll;
    if (!recordPass && uint64_t(ownedTiles)*256*chunksAll > maxItems) {
        chunksPerBatch = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(chunksAll, maxItems/(uint64_t(ownedTiles)*256))));
        chunksPerBatch = std::max(group, chunksPerBatch/group*group);          // whole groups of k_resolve
        if (uint64_t(ownedTiles)*256*chunksPerBatch > maxItems)
            tilesPerBatch = uint32_t(std::max<uint64_t>(1, maxItems/(256ull*chunksPerBatch)));
    }
    if (recordPass) {
        // consecutive ranges of the gap-free enumeration that hold whole groups of chunks (the items of chunk c are
        // [start[c], start[c + 1])), as many groups as fit maxItems, at least one
        const std::vector<uint32_t> &start = out.chunkStart;
        auto push = [&](uint64_t begin, uint64_t end) {
            out.batches.push_back(PassBatch{0u, spp, chunksAll, 1u /* unused by the record enumeration */, uint32_t(end - begin), 0u, uint32_t(begin)});
            out.batchItems = std::max(out.batchItems, end - begin);
        };
        uint64_t begin = 0;
        for (uint32_t c = 0; c < chunksAll; c += group) {
            const uint64_t end = start[std::min(c + group, chunksAll)];
            if (end - begin > maxItems && start[c] > begin) { push(begin, start[c]); begin = start[c]; }
        }
        push(begin, recordItems);
        out.totalItems = recordItems;
    } else {
        // (64 bits: a range that ends near 2^32 must not wrap the counter back below its end)
        for (uint64_t sppFirst64 = sppBegin; sppFirst64 < sppEnd; sppFirst64 += uint64_t(chunksPerBatch)*chunk) {
            const uint32_t sppFirst = uint32_t(sppFirst64);
            const uint32_t sppLast = uint32_t(std::min<uint64_t>(sppFirst64 + uint64_t(chunksPerBatch)*chunk, sppEnd));
            for (uint32_t first = 0; first < ownedTiles; first += tilesPerBatch) {
                PassBatch b;
                b.sppBegin = sppFirst; b.sppEnd = sppLast;
                b.chunks = (sppLast - sppFirst + chunk - 1)/chunk;
                b.pixSlots = std::min(tilesPerBatch, ownedTiles - first)*256;
                b.totalItems = b.pixSlots*b.chunks;
                b.firstTile = first;
                b.itemBase = 0;
                out.batches.push_back(b);
            }
        }
        out.totalItems = uint64_t(ownedTiles)*256*chunksAll;
        out.batchItems = uint64_t(tilesPerBatch)*256*chunksPerBatch;
    }
    // A pass whose work items fill less than half the pool never refills a slot: it is one long drain, every iteration of which
    // pays the fixed cost of its launches.  Such passes (the 16-spp passes of the as-shipped materialtest: 3.7 M items) run on ONE
    // stream with 4 workgroups per CU -- 431 against 372 Msamples/s with four parts.  (One rank's share of an 8-GPU render of the
    // metric's workload, 7.4 M items, stays on four parts.)
    out.shortBatch = 2u*out.batchItems <= opt.maxSlots;
    out.empty = false;
    return TGHIP_OK;
}
