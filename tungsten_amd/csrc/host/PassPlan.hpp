// What tghip_render_pass and tghip_wait decide about a pass before anything touches the device: the refusals of a malformed description, the tiles the
// shard owns, the per-record arrays of an adaptive pass and its gap-free item enumeration, the samples per work item and the cut of the pass into
// batches.  Plain host arithmetic over TgHipPassDesc: no device, no context (include/tungsten_host.h: tgh_pass_plan runs it on its own).
#ifndef TGAMD_PASSPLAN_HPP_
#define TGAMD_PASSPLAN_HPP_

#include "../../../include/tungsten_hip.h"

#include <cstdint>
#include <string>
#include <vector>

// the options of a context that change how a pass is cut (tghip_set_option)
struct PassPlanOptions {
    uint64_t maxItems;        // "max_items": work items per batch (at least 256)
    uint64_t maxSlots;        // "max_slots": the path pool's size, which a short batch is measured against
    uint32_t chunkSamples;    // "chunk_samples": samples per work item; 0 = one or four, by the size of the pass
};

// what differs between the PassParams of one pass's batches
struct PassBatch {
    uint32_t sppBegin, sppEnd;     // sample range (record passes: relative to each record's first index, the whole range in every batch)
    uint32_t chunks;               // chunks of `chunk` samples in that range
    uint32_t pixSlots;             // pixel slots of the batch's tiles (record passes: 1, unused)
    uint32_t totalItems;
    uint32_t firstTile;            // first of the batch's tiles in the shard's list
    uint32_t itemBase;             // record passes: the batch's first item in the gap-free enumeration
};

// Lives in the context and is reused from pass to pass: the vectors keep their capacity.
struct PassPlan {
    bool empty = true;             // nothing to render: the shard owns no tile, or no owned pixel gets a sample
    uint32_t tilesX = 0, tilesY = 0, numTiles = 0;
    uint32_t shardCount = 1, shardSkew = 0;
    // the shard's tiles (tghip_tile_owner: a diagonal interleave), row-major; kept from pass to pass under ownedKey = {W, H, shard index, shard count}.
    // Unsharded passes own every tile and keep no list.  ownedStale: planPass rebuilt the list; whoever keeps a copy of it clears the flag.
    uint32_t ownedTiles = 0;
    std::vector<uint32_t> ownedList;
    uint32_t ownedKey[4] = {0, 0, 0, 0};
    bool ownedStale = false;

    // TGHIP_PASS_RECORDS: per record its first sample index, its samples per pixel and the offset of its 16 x count luminance block; the owned records
    // with a count above 0 sorted by descending count, ties in record order; chunk c of that order holds the items [chunkStart[c], chunkStart[c + 1]),
    // with 0xFFFFFFFF behind the last start
    bool recordPass = false;
    uint32_t varianceW = 0, numRecords = 0;
    std::vector<uint32_t> recIndex, recCount, recLum, sorted, chunkStart;
    uint64_t lumFloats = 0;
    uint64_t recordItems = 0;
    size_t hintEntries = 0;        // for every 64 items the chunk their first one lies in, plus one
    std::vector<uint32_t> bucket, sortTmp;   // counting sort of the owned records by sample count

    uint32_t spp = 0, sppBegin = 0;   // the sample range as the batches see it (record passes: [0, max count of an owned record))
    uint32_t chunk = 0, group = 0;    // samples per work item, and the chunks k_resolve adds up together (4 one-sample items, or 1)
    uint32_t chunksAll = 0;
    bool auxPass = false;             // TGHIP_PASS_AUX: one work item per pixel
    std::vector<PassBatch> batches;
    uint64_t totalItems = 0;          // of the whole pass
    uint64_t batchItems = 0;          // of its largest batch
    bool shortBatch = false;          // the batches fill less than half the pool
};

// The refusals of tghip_render_pass that need no context: TGHIP_OK, or TGHIP_E_INVALID with the reason in `error`.
int checkPass(const TgHipPassDesc &pass, uint32_t w, uint32_t h, bool sceneHasSobol, std::string &error);
// Plans a pass checkPass accepted, for a w x h image: fills `out` and returns TGHIP_OK, or refuses a pass whose luminance floats or work items do not
// fit 32 bits (TGHIP_E_UNSUPPORTED, the reason in `error`).  Reads record_index / record_count (ceil(w/4)*ceil(h/4) entries each) when given.
int planPass(const TgHipPassDesc &pass, uint32_t w, uint32_t h, const PassPlanOptions &opt, PassPlan &out, std::string &error);

#endif
