// psim_payload.h -- the host arithmetic of the payload exchange (a sharded
// full-strategy handle ships the ORSet rows its STATE and GOSSIP records name:
// psim_engine.hip).  Counts in, offsets out; no device
// calls, so a stand-alone program can run it under a host sanitizer
// (tests/payload_layout_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace psim {

// words of one owner's row of the (owner, slot) bitmap over an arena of `cap`
// rows: a multiple of 64, so that a wave's 64 words belong to one owner
inline uint32_t payload_bitmap_words(uint32_t cap) {
    const uint64_t w = ((uint64_t)cap + 31) / 32;
    return (uint32_t)((w + 63) / 64 * 64 + (w ? 0 : 64));
}

// the sender's payload buffer: owner g's rows at [off[g], off[g + 1]) (rows
// of rowlen words), `rows` in all
struct PayLayout {
    std::vector<uint64_t> off;
    uint64_t rows = 0;
    uint32_t rowlen = 0;
};
inline PayLayout payload_offsets(const uint64_t* cnt, uint32_t G, uint32_t rowlen) {
    PayLayout l;
    l.rowlen = rowlen;
    l.off.assign((size_t)G + 1, 0);
    for (uint32_t g = 0; g < G; g++) l.off[g + 1] = l.off[g] + cnt[g];
    l.rows = l.off[G];
    return l;
}

// the receiver's import buffer: source g's rows from base[g] on, in
// source-shard order; false if the total does not fit the 31 bits word 7
// leaves beside its tag
inline bool payload_import_bases(const uint64_t* cnt, uint32_t G, std::vector<uint32_t>& base, uint64_t* total) {
    base.assign((size_t)G + 1, 0);
    uint64_t t = 0;
    for (uint32_t g = 0; g < G; g++) {
        base[g] = (uint32_t)t;
        t += cnt[g];
        if (t >= 0x80000000ull) return false;
    }
    base[G] = (uint32_t)t;
    *total = t;
    return true;
}

// exchange traffic of the rows one shard sends: every row to another shard
inline uint64_t payload_bytes(const uint64_t* cnt, uint32_t G, uint32_t self, uint32_t rowlen) {
    uint64_t rows = 0;
    for (uint32_t g = 0; g < G; g++) rows += g == self ? 0 : cnt[g];
    return rows * rowlen * 4;
}

}  // namespace psim
