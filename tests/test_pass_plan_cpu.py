"""The host-side plan of a pass (tungsten_amd/csrc/host/PassPlan.cpp, through tgh_pass_plan_*): what tghip_render_pass refuses and what tghip_wait decides
before it touches the device -- the shard's tiles, the per-record arrays and the gap-free enumeration of an adaptive pass, the samples per work item, the
batches.  No device.

Every expectation is a brute-force statement of the rule, written here as loops and searches over tiles, records and sample indices ("the largest
number of whole groups that fits"), not as the closed forms of the C++.

One case the rules cannot produce: the second 2^32 refusal ("work items per device").  A record with n samples per pixel contributes 16*n luminance
floats and 16*ceil(n/chunk) work items, and chunk >= 1 always, so the items of a pass never outnumber its luminance floats -- a pass that trips the
second refusal has tripped the first.  The refusal stays in the code as it was; every record case below asserts items <= floats, and the first
refusal is tested on both sides of 2^32."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tungsten_amd as tg
from tungsten_amd import capi

INVALID, UNSUPPORTED = capi.TGHIP_E_INVALID, capi.TGHIP_E_UNSUPPORTED
SOBOL, RECORDS, AUX, SAMPLES = capi.TGHIP_PASS_SOBOL, capi.TGHIP_PASS_RECORDS, capi.TGHIP_PASS_AUX, capi.TGHIP_PASS_SAMPLES
SENTINEL = 0xFFFFFFFF
MAX_SLOTS = 1 << 23


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


class Plan(object):
    """A plan's scalars (.info), batches (list of dicts) and arrays (numpy copies, None where the plan has none)."""


def plan(w, h, spp_begin=0, spp_end=0, shard=(0, 1), flags=0, tile_seeds=None, rec_index=None, rec_count=None,
         max_items=1 << 26, max_slots=MAX_SLOTS, chunk_samples=0, sobol_scene=True):
    """(return code, Plan or None, message) of tgh_pass_plan_create."""
    keep = []
    d = capi.TgHipPassDesc()
    d.spp_begin, d.spp_end, d.seed, d.shard_index, d.shard_count, d.flags = spp_begin, spp_end, 1, shard[0], shard[1], flags
    for name, a in (("tile_seeds", tile_seeds), ("record_index", rec_index), ("record_count", rec_count)):
        if a is not None:
            arr, ptr = _u32(a)
            keep.append(arr)
            setattr(d, name, ptr)
    rc = C.c_int(12345)
    err = C.create_string_buffer(512)
    p = tg.lib.tgh_pass_plan_create(C.byref(d), w, h, int(sobol_scene), max_items, max_slots, chunk_samples, C.byref(rc), err, len(err))
    if not p:
        assert rc.value < 0
        return rc.value, None, err.value.decode()
    assert rc.value == 0
    try:
        out = Plan()
        out.info = capi.TgHostPassPlan()
        tg.lib.tgh_pass_plan_info(p, C.byref(out.info))
        n = C.c_uint32(0)
        b = tg.lib.tgh_pass_plan_batches(p, C.byref(n))
        out.batches = [dict((f, getattr(b[i], f)) for f, _ in capi.TgHostPassBatch._fields_) for i in range(n.value)]

        def arr(fn, count=None):
            if count is None:
                ptr = fn(p, C.byref(n))
                count = n.value
            else:
                ptr = fn(p)
            return np.ctypeslib.as_array(ptr, shape=(count,)).copy() if ptr else None
        out.owned = arr(tg.lib.tgh_pass_plan_owned_tiles)
        out.rec_index = arr(tg.lib.tgh_pass_plan_rec_index, out.info.num_records)
        out.rec_count = arr(tg.lib.tgh_pass_plan_rec_count, out.info.num_records)
        out.rec_lum = arr(tg.lib.tgh_pass_plan_rec_lum, out.info.num_records)
        out.sorted = arr(tg.lib.tgh_pass_plan_sorted)
        out.starts = arr(tg.lib.tgh_pass_plan_chunk_starts)
        return 0, out, ""
    finally:
        tg.lib.tgh_pass_plan_free(p)


# ---- the rules, by brute force ------------------------------------------------------------------------------------

def tiles_of(w, h):
    tx = len(range(0, w, 16))
    ty = len(range(0, h, 16))
    return tx, ty


def skew_of(count):
    """the smallest odd prime that does not divide the shard count"""
    for p in (3, 5, 7, 11, 13, 17):
        if count % p:
            return p
    return 1


def owned_tiles(w, h, index, count):
    """the shard's tiles, row-major: tile (x, y) belongs to shard (x + y*skew) mod count"""
    tx, ty = tiles_of(w, h)
    return [x + y*tx for y in range(ty) for x in range(tx) if (x + y*skew_of(count)) % count == index]


def chunks_in(first, last, chunk):
    """chunks of `chunk` consecutive sample indices that [first, last) touches, counted"""
    return len(set((i - first)//chunk for i in range(first, last)))


def expected_plain_cut(owned, chunks_all, chunk, group, max_items):
    """(tiles per batch, chunks per batch): a pass that does not fit one batch is cut by sample range first -- the largest number of whole groups
    that fits the batch and the pass, one group at least -- and then, if a single such range over all tiles still does not fit, by tiles."""
    if owned*256*chunks_all <= max_items:
        return owned, chunks_all
    groups = 1
    while (groups + 1)*group <= chunks_all and owned*256*(groups + 1)*group <= max_items:
        groups += 1
    per_batch = groups*group
    tiles = owned
    if owned*256*per_batch > max_items:
        tiles = 1
        while (tiles + 1)*256*per_batch <= max_items:
            tiles += 1
    return tiles, per_batch


SHARD_COUNTS = {(40, 24): (1, 2, 8, 3, 15, 7), (16, 16): (1, 2, 3), (8, 8): (1, 2)}     # 7 > 6 tiles, 2 and 3 > 1 tile: some shard owns nothing


def test_skews_and_owned_tiles_partition_the_image():
    assert [skew_of(n) for n in (2, 8, 3, 15)] == [3, 3, 5, 7]
    for (w, h), counts in SHARD_COUNTS.items():
        tx, ty = tiles_of(w, h)
        for count in counts:
            seen = []
            for index in range(count):
                rc, p, msg = plan(w, h, 0, 1, shard=(index, count))
                assert rc == 0, msg
                i = p.info
                assert (i.tiles_x, i.tiles_y, i.num_tiles, i.shard_count) == (tx, ty, tx*ty, count)
                if count == 1:
                    assert p.owned is None and i.owned_tiles == tx*ty
                    seen += list(range(tx*ty))
                    continue
                assert i.shard_skew == skew_of(count)
                want = owned_tiles(w, h, index, count)
                got = [] if p.owned is None else list(p.owned)
                assert got == want and i.owned_tiles == len(want), (w, h, index, count)
                assert got == sorted(got)                      # row-major within the shard
                assert bool(i.empty) == (not want)
                seen += got
            assert sorted(seen) == list(range(tx*ty)), (w, h, count)       # every tile in exactly one shard
    assert any(not owned_tiles(40, 24, k, 7) for k in range(7))


def check_plain(w, h, begin, spp, shard, max_items, chunk_samples, flags=0, max_slots=MAX_SLOTS):
    case = (w, h, begin, spp, shard, max_items, chunk_samples, flags)
    rc, p, msg = plan(w, h, begin, begin + spp, shard=shard, flags=flags, max_items=max_items, chunk_samples=chunk_samples, max_slots=max_slots)
    assert rc == 0, (case, msg)
    i = p.info
    owned = len(owned_tiles(w, h, *shard))
    assert (i.owned_tiles, i.spp, i.spp_begin, i.record_pass) == (owned, spp, begin, 0), case
    assert bool(i.aux_pass) == bool(flags & AUX)
    if owned == 0 or spp == 0:
        assert i.empty and not p.batches and i.total_items == 0 and i.batch_items == 0, case
        return p
    assert not i.empty, case
    if flags & AUX:
        chunk = spp                                            # one work item per pixel
    elif chunk_samples:
        chunk = chunk_samples
    else:
        chunk = 4 if owned*256*spp >= 3 << 24 else 1           # four-sample items from 3 * 2^24 pass samples on
    group = 4 if chunk == 1 else 1                             # k_resolve adds one-sample items up in fours
    assert (i.chunk, i.group) == (chunk, group), case
    chunks_all = chunks_in(begin, begin + spp, chunk)
    assert i.chunks_all == chunks_all and i.total_items == owned*256*chunks_all, case
    # every (owned tile, sample index) exactly once
    cover = np.zeros((owned, spp), dtype=np.int32)
    for b in p.batches:
        assert b["pix_slots"] % 256 == 0 and b["pix_slots"] > 0 and b["item_base"] == 0, case
        t0, t1 = b["first_tile"], b["first_tile"] + b["pix_slots"]//256
        assert begin <= b["spp_begin"] < b["spp_end"] <= begin + spp and t1 <= owned, case
        cover[t0:t1, b["spp_begin"] - begin:b["spp_end"] - begin] += 1
        assert b["chunks"] == chunks_in(b["spp_begin"], b["spp_end"], chunk), case
        assert (b["spp_begin"] - begin) % (chunk*group) == 0, case          # a range starts on a group boundary ...
        assert b["chunks"] % group == 0 or b["spp_end"] == begin + spp, case   # ... and holds whole groups, except the last one
        assert b["total_items"] == b["pix_slots"]*b["chunks"], case
        if b["total_items"] > max_items:
            assert b["pix_slots"] == 256 and b["chunks"] <= group, case     # only one tile by one group may exceed the limit
        assert b["total_items"] <= i.batch_items, case
    assert (cover == 1).all(), case
    # exactly the cut the rules give, sample ranges outermost
    tiles, per_batch = expected_plain_cut(owned, chunks_all, chunk, group, max_items)
    assert i.batch_items == tiles*256*per_batch, case
    want = [(s, min(s + per_batch*chunk, begin + spp), t, min(tiles, owned - t)*256)
            for s in range(begin, begin + spp, per_batch*chunk) for t in range(0, owned, tiles)]
    assert [(b["spp_begin"], b["spp_end"], b["first_tile"], b["pix_slots"]) for b in p.batches] == want, case
    assert bool(i.short_batch) == (2*i.batch_items <= max_slots), case
    return p


def test_plain_passes_are_cut_into_batches_that_cover_them_once():
    n = 0
    for (w, h), counts in SHARD_COUNTS.items():
        for count in counts:
            for index in range(count):
                for max_items, spp, begin, chunk_samples in itertools.product((256, 1024), (0, 1, 3, 4, 5, 16), (0, 7), (0, 1, 2, 4)):
                    check_plain(w, h, begin, spp, (index, count), max_items, chunk_samples)
                    n += 1
    assert n > 3000
    # both cuts really happened: by sample range (several ranges over all tiles) and by tiles
    p = check_plain(40, 24, 0, 16, (0, 1), 1024, 1)
    assert len(p.batches) == 24 and len(set(b["spp_begin"] for b in p.batches)) == 4 and p.info.batch_items == 1024    # one group of one tile each
    p = check_plain(16, 16, 7, 16, (0, 1), 1024, 1)
    assert [b["spp_begin"] for b in p.batches] == [7, 11, 15, 19]
    p = check_plain(40, 24, 0, 5, (0, 1), 256, 4)
    assert len(p.batches) == 12 and all(b["total_items"] == 256 for b in p.batches)
    # max_items below the floor of 256 counts as 256
    assert [b for b in check_plain(16, 16, 0, 4, (0, 1), 256, 4).batches] == plan(16, 16, 0, 4, max_items=1, chunk_samples=4)[1].batches


def test_aux_passes_are_one_item_per_pixel():
    for spp, begin, max_items in itertools.product((1, 5, 16), (0, 7), (256, 1024, 1 << 26)):
        p = check_plain(40, 24, begin, spp, (0, 1), max_items, 0, flags=AUX)
        assert p.info.chunk == spp and p.info.chunks_all == 1 and all(b["chunks"] == 1 for b in p.batches)
        check_plain(40, 24, begin, spp, (1, 2), max_items, 4, flags=AUX)


def test_automatic_chunk_choice_at_720p():
    """Plain passes allocate no arrays.  80 x 45 tiles x 256 pixel slots: 921 600 samples per spp, so 3 << 24 pass samples lie between 54 and 55 spp."""
    assert 54*3600*256 < 3 << 24 <= 55*3600*256
    for spp, chunk, group in ((16, 1, 4), (256, 4, 1), (54, 1, 4), (55, 4, 1)):
        p = check_plain(1280, 720, 0, spp, (0, 1), 1 << 26, 0)
        assert (p.info.chunk, p.info.group) == (chunk, group), spp
    # a shard picks by its OWN sample count: half the tiles, so the threshold lies at twice the spp
    assert check_plain(1280, 720, 0, 109, (0, 2), 1 << 26, 0).info.chunk == 1
    assert check_plain(1280, 720, 0, 110, (0, 2), 1 << 26, 0).info.chunk == 4
    # short: 2 * batch items <= max_slots, both sides
    items = 6*256*4
    assert check_plain(40, 24, 0, 4, (0, 1), 1 << 26, 1, max_slots=2*items).info.short_batch
    assert not check_plain(40, 24, 0, 4, (0, 1), 1 << 26, 1, max_slots=2*items - 1).info.short_batch


# ---- record passes ---------------------------------------------------------------------------------------------------

def records_of(w, h):
    rw, rh = len(range(0, w, 4)), len(range(0, h, 4))
    return rw, rh


def owned_records(w, h, index, count):
    """per record: does its 4x4 pixel block lie in a tile of the shard?"""
    rw, rh = records_of(w, h)
    tx, _ = tiles_of(w, h)
    mine = set(owned_tiles(w, h, index, count)) if count > 1 else None
    return np.array([mine is None or ((rx*4)//16 + ((ry*4)//16)*tx) in mine for ry in range(rh) for rx in range(rw)], dtype=bool)


def check_records(w, h, counts, shard, max_items, chunk_samples, begin=3, spp=0, index=None, max_slots=MAX_SLOTS):
    """counts None: the uniform record pass [begin, begin + spp)"""
    rw, rh = records_of(w, h)
    nrec = rw*rh
    case = (w, h, None if counts is None else list(counts[:8]), shard, max_items, chunk_samples)
    if counts is None:
        rc, p, msg = plan(w, h, begin, begin + spp, shard=shard, flags=RECORDS, max_items=max_items, chunk_samples=chunk_samples, max_slots=max_slots)
        counts, index = np.full(nrec, spp, dtype=np.int64), np.full(nrec, begin, dtype=np.int64)
    else:
        counts = np.asarray(counts, dtype=np.int64)
        index = np.arange(nrec, dtype=np.int64)*3 + 1 if index is None else np.asarray(index)
        rc, p, msg = plan(w, h, 1000, 1000, shard=shard, flags=RECORDS, rec_index=index, rec_count=counts, max_items=max_items,
                          chunk_samples=chunk_samples, max_slots=max_slots)            # spp_begin / spp_end are ignored
    assert rc == 0, (case, msg)
    i = p.info
    assert i.record_pass and (i.variance_w, i.num_records) == (rw, nrec), case
    owned = owned_records(w, h, *shard)
    assert (p.rec_index == index).all() and (p.rec_count == counts).all(), case
    # luminance blocks: 16 floats per sample per pixel of an owned record, one behind the other in record order
    lum, total = [], 0
    for r in range(nrec):
        lum.append(total)
        if owned[r]:
            total += 16*int(counts[r])
    assert list(p.rec_lum) == lum and i.lum_floats == total, case
    spp = int(counts[owned].max()) if owned.any() else 0
    assert (i.spp, i.spp_begin) == (spp, 0), case
    if spp == 0:
        assert i.empty and not p.batches, case
        return p
    assert not i.empty, case
    alive = [r for r in range(nrec) if owned[r] and counts[r] > 0]
    assert list(p.sorted) == sorted(alive, key=lambda r: (-counts[r], r)), case       # descending by count, ties in record order
    if chunk_samples:
        chunk = chunk_samples
    else:
        chunk = 4 if 16*int(counts[owned].sum()) >= 3 << 24 else 1
    group = 4 if chunk == 1 else 1
    assert (i.chunk, i.group) == (chunk, group), case
    # chunk c holds one item per pixel of every owned record that still has a sample at c*chunk
    mine = counts[owned]
    nchunks = len(range(0, spp, chunk))
    starts, items = [0], 0
    for c in range(nchunks):
        items += 16*int((mine > c*chunk).sum())
        starts.append(items)
    assert i.chunks_all == nchunks and list(p.starts) == starts + [SENTINEL], case
    assert i.record_items == items == i.total_items and i.hint_entries == len(range(0, items, 64)) + 1, case
    assert items <= total, case                               # (the module's note on the second 2^32 refusal)
    # batches: consecutive ranges of the enumeration that tile [0, items), cut at group boundaries
    boundaries = [starts[c] for c in range(0, nchunks, group)] + [items]
    at = 0
    for k, b in enumerate(p.batches):
        assert (b["spp_begin"], b["spp_end"], b["chunks"], b["first_tile"]) == (0, spp, nchunks, 0), case
        assert b["item_base"] == at and b["total_items"] > 0, case
        at += b["total_items"]
        assert at in boundaries, case
        nxt = min(x for x in boundaries if x > b["item_base"])
        if b["total_items"] > max_items:
            assert at == nxt, case                             # more than max_items: one group only
        if k + 1 < len(p.batches):
            after = min(x for x in boundaries if x > at)
            assert after - b["item_base"] > max_items, case    # ... and as many groups as fit
    assert at == items, case
    assert i.batch_items == max(b["total_items"] for b in p.batches), case
    assert bool(i.short_batch) == (2*i.batch_items <= max_slots), case
    return p


def test_record_passes():
    rng = np.random.RandomState(7)
    for (w, h), shards in (((40, 24), ((0, 1), (0, 2), (1, 2), (2, 3), (4, 8), (11, 15), (6, 7), (5, 7))), ((8, 8), ((0, 1), (1, 2)))):
        nrec = records_of(w, h)[0]*records_of(w, h)[1]
        single = np.zeros(nrec, dtype=np.int64)
        single[nrec//2] = 9
        ties = np.array([(3, 7, 3, 0, 7)[r % 5] for r in range(nrec)])
        patterns = {"equal": np.full(nrec, 5), "zero": np.zeros(nrec, dtype=np.int64), "single": single, "ties": ties,
                    "ramp": np.arange(nrec, 0, -1) + 2, "random": rng.randint(0, 20, nrec)}
        for shard in shards:
            for max_items, chunk_samples in itertools.product((256, 1024), (0, 1, 2, 4)):
                for name, counts in patterns.items():
                    check_records(w, h, counts, shard, max_items, chunk_samples)
                for spp in (0, 1, 5, 16):
                    check_records(w, h, None, shard, max_items, chunk_samples, begin=7, spp=spp)
    # the record cut really happens, and several batches hold more than one group
    p = check_records(40, 24, np.full(60, 16), (0, 1), 1024, 1)
    assert [b["total_items"] for b in p.batches] == [3840]*4                           # 960 items per chunk: one group of four exceeds 1024
    p = check_records(8, 8, np.full(4, 16), (0, 1), 1024, 1)
    assert [b["total_items"] for b in p.batches] == [1024]                             # 64 items per chunk: all four groups fit
    p = check_records(8, 8, np.full(4, 16), (0, 1), 256, 1)
    assert [b["total_items"] for b in p.batches] == [256]*4
    # a shard that owns nothing
    assert check_records(40, 24, np.full(60, 5), (6, 7), 1024, 0).info.empty


@pytest.mark.parametrize("top", [65535, 65536])
def test_record_sort_on_both_sides_of_its_switch(top):
    """Below 2^16 samples per pixel the records are sorted by counting, from there on by comparing: the same order either way."""
    p = check_records(8, 8, [3, top, 3, top], (0, 1), 1 << 26, 4)
    assert list(p.sorted) == [1, 3, 0, 2]
    p = check_records(8, 8, [top, 0, top - 1, top], (0, 1), 1 << 26, 0)
    assert list(p.sorted) == [0, 3, 2]


def test_automatic_chunk_choice_of_record_passes():
    """By 16 x the owned counts' sum, on both sides of 3 << 24: 256 records of a 64 x 64 image."""
    counts = np.full(256, (3 << 24)//16//256)
    assert 16*counts.sum() == 3 << 24
    assert check_records(64, 64, counts, (0, 1), 1 << 26, 0).info.chunk == 4
    counts[5] -= 1
    assert check_records(64, 64, counts, (0, 1), 1 << 26, 0).info.chunk == 1
    # a shard counts its own records only
    full = np.full(256, 2*((3 << 24)//16//256))
    assert check_records(64, 64, full, (0, 2), 1 << 26, 0).info.chunk == 4
    full[owned_records(64, 64, 0, 2).argmax()] -= 1
    assert check_records(64, 64, full, (0, 2), 1 << 26, 0).info.chunk == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_passes_past_2_to_32_samples_are_refused():
    rc, p, msg = plan(64, 64, flags=RECORDS, rec_index=np.zeros(256), rec_count=np.full(256, 1 << 24))
    assert rc == UNSUPPORTED and "2^32 samples per device" in msg and "lower spp_step" in msg
    # 256 records x 16 pixels x 2^20 samples = 2^32 exactly is refused, one sample less is planned
    counts = np.full(256, 1 << 20)
    rc, p, msg = plan(64, 64, flags=RECORDS, rec_index=np.zeros(256), rec_count=counts)
    assert rc == UNSUPPORTED and "2^32 samples per device" in msg
    counts[255] -= 1
    rc, p, msg = plan(64, 64, flags=RECORDS, rec_index=np.zeros(256), rec_count=counts, chunk_samples=1)
    assert rc == 0 and p.info.lum_floats == (1 << 32) - 16 == p.info.record_items
    # records of other shards do not count
    big = np.where(owned_records(64, 64, 0, 2), 1 << 19, 1 << 24)
    rc, p, msg = plan(64, 64, shard=(0, 2), flags=RECORDS, rec_index=np.zeros(256), rec_count=big)
    assert rc == 0 and p.info.lum_floats == 16*(1 << 19)*int(owned_records(64, 64, 0, 2).sum())
    # the uniform record pass
    rc, p, msg = plan(64, 64, 0, 1 << 20, flags=RECORDS)
    assert rc == UNSUPPORTED and "2^32 samples per device" in msg


def test_check_pass_refusals():
    seeds, idx, cnt = np.arange(6), np.zeros(60), np.full(60, 2)
    valid = dict(spp_begin=2, spp_end=6, shard=(1, 2), flags=SOBOL | RECORDS, tile_seeds=seeds, rec_index=idx, rec_count=cnt)
    assert plan(40, 24, **valid)[0] == 0

    def refused(piece, code=INVALID, **change):
        kw = dict(valid)
        kw.update(change)
        rc, p, msg = plan(40, 24, **kw)
        assert rc == code and p is None and piece in msg, (change, rc, msg)
    refused("invalid pass description", spp_end=1)
    refused("invalid pass description", shard=(2, 2))
    refused("invalid pass description", shard=(7, 2))
    refused("unknown pass flags", flags=SOBOL | RECORDS | 16)
    refused("unknown pass flags", flags=1 << 31)
    refused("TGHIP_PASS_SOBOL needs sobol_matrices", sobol_scene=False)
    refused("TGHIP_PASS_SOBOL needs sobol_matrices", tile_seeds=None)
    refused("record_index and record_count go together", rec_index=None)
    refused("record_index and record_count go together", rec_count=None)
    refused("need TGHIP_PASS_RECORDS", flags=SOBOL)
    refused("does not combine with per-record sample counts", flags=SOBOL | RECORDS | SAMPLES)
    # TGHIP_PASS_SAMPLES: W*H*spp*3 floats below 2^31 -- 960 pixels: 745 654 spp at most
    assert 960*3*745654 < 1 << 31 <= 960*3*745655
    assert plan(40, 24, 1, 1 + 745654, flags=SAMPLES)[0] == 0
    rc, p, msg = plan(40, 24, 1, 1 + 745655, flags=SAMPLES)
    assert rc == INVALID and "TGHIP_PASS_SAMPLES keeps W*H*spp*3 floats (< 2^31)" in msg
    # shard_count 0 means the whole image, and a Sobol pass of a scene with matrices is fine without records
    rc, p, msg = plan(40, 24, 0, 4, shard=(5, 0), flags=SOBOL, tile_seeds=seeds)
    assert rc == 0 and p.info.shard_count == 1 and p.info.owned_tiles == 6
    # no description, and the optional outputs
    err = C.create_string_buffer(64)
    rc = C.c_int(0)
    assert not tg.lib.tgh_pass_plan_create(None, 40, 24, 1, 256, 256, 0, C.byref(rc), err, len(err)) and rc.value == INVALID
    d = capi.TgHipPassDesc(spp_end=4)
    p = tg.lib.tgh_pass_plan_create(C.byref(d), 40, 24, 0, 256, 256, 0, None, None, 0)
    assert p
    tg.lib.tgh_pass_plan_free(p)
    tg.lib.tgh_pass_plan_free(None)
    assert not tg.lib.tgh_pass_plan_batches(None, None) and not tg.lib.tgh_pass_plan_sorted(None, None)
