// The host arithmetic of the payload exchange (partisan_amd/csrc/psim_payload.h)
// in a stand-alone program, so that it runs under a host sanitizer
// (tests/test_payload_layout.py builds it with -fsanitize=address,undefined):
// bitmap widths, the sender's per-owner offsets, the receiver's per-source
// bases and the 31-bit limit of word 7, the byte accounting.  Every sender's
// region for an owner must be what that owner's import bases expect.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../partisan_amd/csrc/psim_payload.h"

using namespace psim;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                \
        }                                                            \
    } while (0)

static uint64_t next(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

int main() {
    // bitmap words: enough bits, a multiple of 64, never zero
    for (uint32_t cap : {0u, 1u, 31u, 32u, 33u, 2047u, 2048u, 2049u, 65536u, 0x7FFFFFFFu}) {
        const uint32_t bw = payload_bitmap_words(cap);
        CHECK(bw % 64 == 0 && bw >= 64);
        CHECK((uint64_t)bw * 32 >= cap);
        CHECK((uint64_t)bw * 32 < (uint64_t)cap + 64 * 32 + 32);
    }
    uint64_t seed = 7;
    for (uint32_t G : {1u, 2u, 3u, 7u, 64u}) {
        for (uint32_t rowlen : {4u, 264u, 528u, 6256u}) {
            // cnt[s][d]: the rows shard s packs for owner d (none for itself)
            std::vector<std::vector<uint64_t>> cnt(G, std::vector<uint64_t>(G));
            for (uint32_t s = 0; s < G; s++)
                for (uint32_t d = 0; d < G; d++) cnt[s][d] = s == d ? 0 : next(seed) % 100000;
            std::vector<PayLayout> lay;
            for (uint32_t s = 0; s < G; s++) {
                lay.push_back(payload_offsets(cnt[s].data(), G, rowlen));
                const PayLayout& l = lay.back();
                CHECK(l.off.size() == G + 1 && l.off[0] == 0 && l.rowlen == rowlen);
                uint64_t sum = 0;
                for (uint32_t d = 0; d < G; d++) {
                    CHECK(l.off[d] == sum);
                    sum += cnt[s][d];
                }
                CHECK(l.rows == sum && l.off[G] == sum);
                CHECK(payload_bytes(cnt[s].data(), G, s, rowlen) == sum * rowlen * 4);
            }
            for (uint32_t d = 0; d < G; d++) {
                std::vector<uint64_t> in(G);
                for (uint32_t s = 0; s < G; s++) in[s] = cnt[s][d];
                std::vector<uint32_t> base;
                uint64_t total = 0;
                CHECK(payload_import_bases(in.data(), G, base, &total));
                CHECK(base.size() == G + 1 && base[0] == 0 && base[G] == total);
                // a buffer of `total` rows takes every source's region whole
                std::vector<uint8_t> seen(total, 0);
                for (uint32_t s = 0; s < G; s++) {
                    CHECK(lay[s].off[d + 1] - lay[s].off[d] == in[s]);
                    for (uint64_t r = 0; r < in[s]; r++) {
                        CHECK(base[s] + r < total && !seen[base[s] + r]);
                        seen[base[s] + r] = 1;
                    }
                }
            }
        }
    }
    {   // word 7 keeps 31 bits for the row index
        std::vector<uint64_t> in = {0x40000000ull, 0x3FFFFFFFull};
        std::vector<uint32_t> base;
        uint64_t total = 0;
        CHECK(payload_import_bases(in.data(), 2, base, &total) && total == 0x7FFFFFFFull);
        in[1]++;
        CHECK(!payload_import_bases(in.data(), 2, base, &total));
    }
    std::puts("payload layout ok");
    return 0;
}
