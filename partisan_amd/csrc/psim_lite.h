// psim_lite.h -- the text of k_lite_quarter / k_lite_half, as templates, for
// the two TUs that instantiate it: psim_lite.hip (the two kernels) and
// psim_consume.hip (the quarter body as the third part of k_hv_phase, which
// must see all three bodies in one TU so that each inlines with its own
// register budget).  Everything is in psim::lite's anonymous namespace: the
// names here (writeback, body, load_desc, STAGE, ...) shadow psim_consume.hip's.
//
// k_lite_quarter / k_lite_half: the SHUFFLE-exchange phase of
// k_relay's lite list (hv:1091-1136 terminals, replies and relays, then a due
// passive_view_maintenance start hv:572-607) with several nodes per wave, one
// per lane group: FOUR per wave, one per 16-lane DPP row (k_lite_quarter, the
// default), or TWO, one per 32-lane half (k_lite_half, PSIM_LITE_HALF=1, A/B).
//
// The wave-per-node kernel (k_consume_lite, psim_consume.hip; PSIM_LITE_WAVE=1,
// A/B) spent its time on one node's serial chain of dependent scalar and
// vector steps: 8.9 k SALU against 9.4 k VALU instructions per wave, issuing
// on 30 % of its cycles (profiles/r03/p38/sq_kernels.txt).  Every list here is
// at most 32 entries (passive <= 30, active <= 8, exchanges <= 8), so a group
// of 32 or 16 lanes carries a node, and every value that was wave-uniform -- a
// node's draw counter, view sizes, the element a step picks -- lives in a VGPR
// that holds the same value across its group.  List operations become
// per-group VALU work with no SALU decisions:
//   membership / count   the group's ballot bits (Grp::mask) and v_bcnt
//   element j            ds_bpermute within the group (Grp::get)
//   lane J, a constant   Grp::getc<J>: ds_swizzle (32) or DPP row_newbcast (16)
//   insert in to_list    a prefix predicate on the bucket tags and DPP shifts
//     order              (Pas<W>::step)
//   sublist(shuffle)     one Philox draw per entry, each entry's rank among
//                        the group's keys (an exact recount on a top-32-bit tie)
// so one instruction stream advances every node of the wave.  The handlers
// are written once, for a lane group Grp<W>; what depends on how the passive
// view (<= 30 entries, cap 32) sits in registers -- one entry a lane of a
// half, two a lane of a row -- is Pas<W>, the only type with two versions.
//
// Correctness conditions of everything below:
//   - every cross-lane read (get, getc, get0, the DPP shifts) is its own
//     statement, executed with its whole group active: a source lane outside
//     the exec mask reads as 0, so none sits on the right of a per-lane && or ?:
//   - control flow diverges only between groups (exec-masked), never inside one
//   - the half's DPP shifts are whole-wave shifts (psim_wave.h from_prev /
//     from_next): a half's lane 31 reads the other half's lane 0 only where
//     no select takes it, and lane 32 (its lane 0) never takes lane 31's value
//   - a row's shifts are row_shr:1 / row_shl:1: the row's end lanes take a
//     fill value, so nothing leaks between the nodes of a wave
// The handlers are the wave kernel's -- the same draws, records, sequence
// numbers, digest, stats and rows -- which the GPU parity tests check against
// the oracle for all three kernels.
//
// Reference: hv = src/partisan_hyparview_peer_service_manager.erl
#pragma once
#include <utility>

#include "psim_device.h"
#include "psim_kernels.h"
#include "psim_wave.h"

namespace psim {
namespace lite {
namespace {

#ifndef PSIM_HALF_WPB
#define PSIM_HALF_WPB 4
#endif
#ifndef PSIM_HALF_WAVES
#define PSIM_HALF_WAVES 4
#endif
#ifndef PSIM_QUARTER_WPB
#define PSIM_QUARTER_WPB 4
#endif
#ifndef PSIM_QUARTER_WAVES
#define PSIM_QUARTER_WAVES 4
#endif
// 1: the next node's rows reach LDS by LDS-DMA, issued before this node's
// body (rows_dma / rows_read below); 0: by loads into registers issued after
// the body, the text before it, for A/B (profiles/lite_rows_lds/ab_log.txt)
#ifndef PSIM_LITE_ROWS_LDS
#define PSIM_LITE_ROWS_LDS 1
#endif
#ifndef PSIM_QUARTER_STAGE    // (16 against 8: no difference, profiles/lite_quarter/ab_log.txt)
#define PSIM_QUARTER_STAGE 8
#endif

// f(J) for J = 0 .. N - 1, J a compile-time constant
template <class F, int... J>
DEV void unroll_seq(F&& f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}
template <int N, class F>
DEV void unroll(F&& f) {
    unroll_seq(f, std::make_integer_sequence<int, N>{});
}

// ------------------------------------------------------- the lane group --
// W lanes that carry one node.  Shared by both widths:
template <uint32_t W>
struct GrpBase {
    static constexpr uint32_t N = 64 / W;             // groups (nodes) per wave
    static constexpr uint32_t SCR = 32;               // scratch words per group
    static constexpr uint32_t PREF = W / 8;           // inbox records whose exchanges are prefetched
    static constexpr uint32_t FLUSH = W / 4;          // records flushed per pass (16-B pieces, four a record)
    DEV static uint32_t lane() { return __lane_id() & (W - 1); }
    DEV static uint32_t base() { return __lane_id() & (64 - W); }
    DEV static uint32_t idx() { return base() / W; }  // the group's index in the wave
    // lane j (< W, per lane) of this lane's group
    DEV static uint32_t get(uint32_t v, uint32_t j) {
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((base() + (j & (W - 1))) << 2), (int)v);
    }
    DEV static uint64_t get64(uint64_t v, uint32_t j) {
        return ((uint64_t)get((uint32_t)(v >> 32), j) << 32) | get((uint32_t)v, j);
    }
};
template <uint32_t W>
struct Grp;
// a 32-lane half
template <>
struct Grp<32> : GrpBase<32> {
    static constexpr uint32_t WPB = PSIM_HALF_WPB;    // waves per block
    static constexpr uint32_t STAGE = 16;             // staged records per group
    // the 32 ballot bits of this lane's half
    DEV static uint32_t mask(bool p) {
        const uint64_t b = __ballot(p);
        return (__lane_id() & 32u) ? (uint32_t)(b >> 32) : (uint32_t)b;
    }
    DEV static bool any(bool p) { return mask(p) != 0u; }
    // lane J (a constant) of this lane's half: ds_swizzle in bitmask mode
    // (and 0, or J: each 32-lane group reads its lane J) -- no address
    // register, so the unrolled loops below keep no per-J constants live
    template <int J>
    DEV static uint32_t getc(uint32_t v) {
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, J << 5);
    }
    // lane 0 of this lane's half: two v_readlane, no LDS round trip -- the
    // merge's dependent chain waits on this broadcast at every step
    DEV static uint32_t get0(uint32_t v) {
        const uint32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 32);
        return base() ? b : a;
    }
    // the group's lane l + 1 (whole-wave: lane 31 takes the other half's lane 0)
    DEV static uint32_t next(uint32_t v) { return from_next(v); }
    // kMagic[n] for a per-group n in [1, 31] (exact modulo): lane l holds kMagic[l]
    struct Magic { uint32_t km; };
    DEV static Magic magic_lanes() { return {kMagic[lane() == 0 ? 64 : lane()]}; }
    DEV static uint32_t magic(Magic m, uint32_t n) { return get(m.km, n); }
};
// a 16-lane row, which is exactly one DPP row: every fixed-lane cross-lane
// read of the half (ds_swizzle through LDS, or two v_readlane and a select)
// is one VALU DPP op confined to the node's own row
template <>
struct Grp<16> : GrpBase<16> {
    static constexpr uint32_t WPB = PSIM_QUARTER_WPB;
    static constexpr uint32_t STAGE = PSIM_QUARTER_STAGE;
    // the 16 ballot bits of this lane's row
    DEV static uint32_t mask(bool p) { return (uint32_t)(__ballot(p) >> base()) & 0xFFFFu; }
    DEV static bool any(bool p) { return mask(p) != 0u; }
    // lane J (a constant) of this lane's row: DPP row_newbcast:J
    template <int J>
    DEV static uint32_t getc(uint32_t v) {
        static_assert(J >= 0 && J < 16, "a row has 16 lanes");
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + J, 0xF, 0xF, false);
    }
    DEV static uint32_t get0(uint32_t v) { return getc<0>(v); }
    // the row's lane l - 1 / l + 1 (DPP row_shr:1 / row_shl:1); the row's
    // first / last lane, which has no such neighbour, takes `fill`
    DEV static uint32_t prev(uint32_t v, uint32_t fill) {
        return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x111, 0xF, 0xF, false);
    }
    DEV static uint32_t next(uint32_t v, uint32_t fill) {
        return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x101, 0xF, 0xF, false);
    }
    DEV static uint32_t next(uint32_t v) { return next(v, 0u); }
    // lane l holds kMagic[l] and kMagic[16 + l]
    struct Magic { uint32_t km0, km1; };
    DEV static Magic magic_lanes() { return {kMagic[lane()], kMagic[16 + lane()]}; }
    DEV static uint32_t magic(Magic m, uint32_t n) {
        const uint32_t km = (n & 16u) ? m.km1 : m.km0;
        return get(km, n);
    }
};

// the group's share of the wave's LDS (pointers already offset to it)
template <uint32_t W>
struct Lds {
    unsigned long long* sst;         // the block's stats (NST)
    uint32_t* srec;                  // STAGE records x 16 words
    uint32_t* skey;                  // STAGE route keys
    uint32_t* scr;                   // SCR words of scratch
#if PSIM_LITE_ROWS_LDS
    uint32_t* rows;                  // the wave's Rows<W> area (one for its groups: a DMA's lanes are the wave's)
    const uint32_t* tab;             // the block's table of the X4 DMA's pieces (rows_table)
#endif
    typename Grp<W>::Magic KM;
#ifdef PSIM_STAMPS
    unsigned long long* stl;         // 32 phase sums (LDS), shared by the wave's groups
    uint64_t t_last;
#endif
};

// Diagnostic build only (-DPSIM_STAMPS, `make stamps`): s_memtime between
// phase boundaries, even groups of a wave into slots 0-15, odd ones into
// 16-31 (slot + phase; two rows share a slot, hence the LDS atomic), summed
// over all waves into g_stamps_half (debug_stamps_half; profiles/stamps.py).
// A phase every group runs is charged to each; one only another group runs
// goes to this group's next stamp.  (Used where G names the group.)
#ifdef PSIM_STAMPS
__device__ unsigned long long g_stamps_half[32];
#define LSTAMP(w, k)                                                                 \
    do {                                                                             \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                            \
        if (G::lane() == 0)                                                          \
            atomicAdd(&(w).stl[(G::idx() & 1u) * 16 + (k)], (unsigned long long)(t_ - (w).t_last)); \
        (w).t_last = t_;                                                             \
    } while (0)
#else
#define LSTAMP(w, k) do { } while (0)
#endif

// a node's counters (each group counts its own nodes'; its lane 0 adds them
// to the block's stats at the kernel's end), and the wave's digest
struct Cnt {                          // (summed over the group's nodes: < 2^16 each)
    uint32_t dl;                     // SHUFFLE | SHUFFLE_REPLY << 16 delivered
    uint32_t em;                     // SHUFFLE | SHUFFLE_REPLY << 16 emitted
    uint32_t pb;                     // nodes | bound violations << 16
    uint32_t fail;
    uint64_t digest;                 // lane j < 16 of a group sums word j of its records
};

// ------------------------------------------------------ the passive view --
// The passive view in registers, or its tagged form: an entry and its bucket
// as one tag, bucket << 27 | id (ids < 2^27, KEY_DST_MASK), TSENT past the
// count.  The entries of a bucket <= t's are the tags <= t's bucket |
// 0x07FFFFFF, a prefix of the to_list order (sets v1); membership is tag
// equality (a candidate past the count is TSENT and matches the empty
// entries: a no-op).
constexpr uint32_t TSENT = 0xFFFFFFFFu, IDM = (1u << 27) - 1;
DEV uint32_t tag_of(const uint8_t* bt, uint32_t id, bool live) {
    const uint32_t b = live ? bucket16(bt, id) : 0u;
    return live ? (b << 27) | id : TSENT;
}
DEV uint32_t id_of(uint32_t tag) { return tag == TSENT ? 0u : tag & IDM; }

template <uint32_t W>
struct Pas;
// one entry a lane: lane l holds passive[l]
template <>
struct Pas<32> {
    using G = Grp<32>;
    using Row = uint32_t;
    uint32_t P;
    DEV static Row load(const uint32_t* row) { return row[G::lane()]; }
    DEV void store(uint32_t* row) const { row[G::lane()] = P; }
    DEV void set(Row r, uint32_t n) { P = G::lane() < n ? r : 0u; }
    DEV Pas tagged(const uint8_t* bt, uint32_t n) const { return {tag_of(bt, P, G::lane() < n)}; }
    DEV Pas untagged() const { return {id_of(P)}; }
    DEV bool has(uint32_t tt) const { return G::any(P == tt); }
    // One add_to_passive step on the tagged view: with `ev` the entry at k
    // goes, then t goes in at its bucket's position -- one select per lane
    // among its own, its predecessor's and its successor's tag and t's.  A
    // member (`mem`: never with `ev`) is a no-op.
    DEV void step(uint32_t& n, uint32_t& dirty, uint32_t tt, bool mem, bool ev, uint32_t k) {
        const uint32_t l = G::lane();
        const uint32_t pv = from_prev(P), nx = from_next(P);
        // entries of a bucket <= t's, then t's position once lane k is gone
        const uint32_t c = (uint32_t)__popc(G::mask(P <= (tt | IDM)));
        const uint32_t p = c - ((ev && k < c) ? 1u : 0u);
        const bool gone = ev && l >= k, gone1 = ev && l >= k + 1;   // (l - 1 >= k)
        const uint32_t F = l < p ? (gone ? nx : P) : l == p ? tt : (gone1 ? P : pv);
        P = mem ? P : F;
        n += (mem ? 0u : 1u) - (ev ? 1u : 0u);
        dirty |= mem ? 0u : 1u;
    }
    template <class Node>
    DEV static uint32_t sublist(Node& x, Lds<32>& w, uint32_t k, uint32_t& OUT, uint32_t on);
};
// two entries a lane: entry e sits in lane e >> 1, slot e & 1 (P0: even
// entries, P1: odd), so a row is one uint2 load per lane, entry e - 1 is the
// lane's own slot 0 or the previous lane's slot 1, and entry e + 1 the mirror
template <>
struct Pas<16> {
    using G = Grp<16>;
    using Row = uint2;
    uint32_t P0, P1;
    DEV static Row load(const uint32_t* row) { return reinterpret_cast<const uint2*>(row)[G::lane()]; }
    DEV void store(uint32_t* row) const { reinterpret_cast<uint2*>(row)[G::lane()] = make_uint2(P0, P1); }
    DEV void set(Row r, uint32_t n) {
        P0 = 2 * G::lane() < n ? r.x : 0u;
        P1 = 2 * G::lane() + 1 < n ? r.y : 0u;
    }
    DEV Pas tagged(const uint8_t* bt, uint32_t n) const {
        return {tag_of(bt, P0, 2 * G::lane() < n), tag_of(bt, P1, 2 * G::lane() + 1 < n)};
    }
    DEV Pas untagged() const { return {id_of(P0), id_of(P1)}; }
    DEV bool has(uint32_t tt) const { return G::any(P0 == tt || P1 == tt); }
    // One add_to_passive step on the tagged view, in two shifts that need no
    // count over the row:
    //   evict   with `ev`, entries k.. move down one: entry e >= k takes entry
    //           e + 1 -- slot 0 its lane's slot 1, slot 1 the next lane's slot 0
    //           (the row's last slot takes TSENT)
    //   insert  an entry outside the prefix of buckets <= t's takes t when its
    //           predecessor is inside (or it is entry 0), its predecessor
    //           otherwise -- slot 1's is its lane's slot 0, slot 0's the
    //           previous lane's slot 1
    // A member (`mem`: never with `ev`) makes every entry "inside": a no-op.
    DEV void step(uint32_t& n, uint32_t& dirty, uint32_t tt, bool mem, bool ev, uint32_t k) {
        const uint32_t l = G::lane(), e0 = 2 * l, e1 = 2 * l + 1;
        const uint32_t kk = ev ? k : 0xFFu;
        const uint32_t nx = G::next(P0, TSENT);
        const uint32_t D0 = e0 >= kk ? P1 : P0, D1 = e1 >= kk ? nx : P1;
        const uint32_t lim = mem ? TSENT : (tt | IDM);
        const uint32_t pv = G::prev(D1, 0u);              // (entry 0's "predecessor" is inside)
        const bool in0 = D0 <= lim, in1 = D1 <= lim, inp = pv <= lim;
        const uint32_t b0 = inp ? tt : pv, b1 = in0 ? tt : D0;
        P0 = in0 ? D0 : b0;
        P1 = in1 ? D1 : b1;
        n += (mem ? 0u : 1u) - (ev ? 1u : 0u);
        dirty |= mem ? 0u : 1u;
    }
    template <class Node>
    DEV static uint32_t sublist(Node& x, Lds<16>& w, uint32_t k, uint32_t& OUT, uint32_t on);
};

// one node per group: everything here is per lane, equal across the group
template <uint32_t W>
struct Node {
    uint32_t me, ob, ib, ik;
    uint32_t fl;                     // the due timers (DESC_* bits, k_desc) | HF_PDIRTY | partition << 8
                                     // | header word 9's bytes 2-3 << 16 (kept for the writeback)
    uint32_t act_n, pas_n;
    uint64_t rng;                    // the Philox draw counter
    uint32_t A;                      // lane l: active[l] (l < 8)
    Pas<W> pas;                      // the passive view
    uint32_t AF;                     // bit j: active member j is up in this node's group (k_relay's
                                     // RoundArgs::lite_cm); bits 8..: the outbox's slots,
                                     // obase[row + 1] - ob (out_cap), saturating at 2^24 - 1
    uint32_t seq, flushed;
    uint64_t dcb;                    // draw cache: lane l holds the draw of counter dcb + l
    uint32_t DCL, DCH;
};
constexpr uint32_t HF_PDIRTY = 16;  // Node::fl: the passive view changed
template <uint32_t W>
DEV uint32_t local_row(const Node<W>& x) { return x.me - kargs().lo; }
// the node's outbox slots: no store goes past them (a record past the bound
// is not stored -- the engine fails the round on the bound check)
template <uint32_t W>
DEV uint32_t out_cap(const Node<W>& x) { return x.AF >> 8; }

// ------------------------------------------------------------------ RNG --
// a W-deep draw cache (a merge's <= 8 eviction draws, a relay's and a start's
// single draws, the one-entry-a-lane sublists' keys)
template <uint32_t W>
DEV void dc_fill(Node<W>& x, uint64_t base) {
    const uint64_t v = draw58_at(base + Grp<W>::lane(), x.me, kargs().seed);
    x.DCL = (uint32_t)v; x.DCH = (uint32_t)(v >> 32);
    x.dcb = base;
}
// the cache covers draws [base, base + n), n <= W
template <uint32_t W>
DEV void dc_cover(Node<W>& x, uint64_t base, uint32_t n) {
    if (base < x.dcb || base + n > x.dcb + W) dc_fill(x, base);
}
template <uint32_t W>
DEV uint64_t draw(Node<W>& x) {
    using G = Grp<W>;
    const uint64_t c = x.rng++;
    dc_cover(x, c, 1);
    const uint32_t i = (uint32_t)(c - x.dcb);
    return ((uint64_t)G::get(x.DCH, i) << 32) | G::get(x.DCL, i);
}
// rand:uniform(n), n < 32 (OTP rand.erl ?uniform_range on 58-bit draws)
template <uint32_t W>
DEV uint32_t uniform_n(Node<W>& x, const Lds<W>& w, uint32_t n) {
    const uint64_t two58 = 1ull << 58;
    const uint32_t M = Grp<W>::magic(w.KM, n);
    for (;;) {
        const uint64_t v = draw(x);
        if (v < n) return (uint32_t)v + 1;
        const uint32_t i = mod_small_m(v, n, M);
        if (v - i <= two58 - n) return i + 1;
    }
}

// select_random/2 (hv:1346-1356) over a one-entry-a-lane view:
// rand:uniform(length(View -- Omit)), no draw when nothing is eligible
template <uint32_t W>
DEV uint32_t select_random(Node<W>& x, const Lds<W>& w, uint32_t V, uint32_t n, uint32_t o0, uint32_t o1) {
    using G = Grp<W>;
    const uint32_t l = G::lane();
    const uint32_t M = G::mask(l < n && V != o0 && V != o1);
    const uint32_t cnt = (uint32_t)__popc(M);
    if (cnt == 0) return PSIM_NONE;
    const uint32_t k = uniform_n(x, w, cnt) - 1;
    // the k-th eligible lane: the one with k eligible lanes below it (no
    // loop of up to k steps, whose count differs between the groups)
    const bool hit = ((M >> l) & 1u) && (uint32_t)__popc(M & ((1u << l) - 1u)) == k;
    return G::get(V, (uint32_t)__ffs(G::mask(hit)) - 1);
}

// lists:sublist(shuffle(to_list(View)), K) (hv:1359-1361, :1586-1587) of a
// one-entry-a-lane view of n <= MAXN entries: one rand:uniform() key per
// element (element l draws counter rng + l), the K smallest (key, element)
// pairs in order, appended to OUT at lanes on..
template <int MAXN, uint32_t W>
DEV uint32_t sublist(Node<W>& x, Lds<W>& w, uint32_t V, uint32_t n, uint32_t k, uint32_t& OUT, uint32_t on) {
    using G = Grp<W>;
    static_assert(MAXN <= (int)W, "one entry and one cached draw a lane");
    const uint32_t l = G::lane();
    const uint64_t base = x.rng;
    dc_cover(x, base, n);
    const uint32_t src = (uint32_t)(base - x.dcb) + l;                // (lanes >= n: unused)
    const uint64_t v = ((uint64_t)G::get(x.DCH, src) << 32) | G::get(x.DCL, src);
    const uint64_t key = l < n ? v >> 5 : ~0ull;
    const uint32_t m = n < k ? n : k;
    const uint32_t hi = (uint32_t)(key >> 21);
    // rank on the top 32 of the 53 key bits (n <= MAXN: lanes >= n hold ~0
    // and count for no lane below n); two lanes of one rank -- a tie, about
    // once in 10^7 sublists -- show as a rank slot another lane took, and the
    // ranks are recounted exactly on (key, element)
    uint32_t rank = 0;
    unroll<MAXN>([&](auto J) {
        const uint32_t hj = G::template getc<J>(hi);
        rank += hj < hi ? 1u : 0u;
        // (at most eight swizzles in flight: the scheduler would otherwise
        // issue all of them first and hold MAXN results in registers)
        if constexpr (J % 8 == 7 && J + 1 < MAXN) __builtin_amdgcn_sched_barrier(0);
    });
    uint32_t* s = w.scr;
    if (l < n) s[rank] = l;
    __builtin_amdgcn_wave_barrier();
    const uint32_t owner = s[rank & 31];
    __builtin_amdgcn_wave_barrier();
    if (G::any(l < n && owner != l)) {
        rank = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t kj = G::get64(key, j);
            const uint32_t ej = G::get(V, j);
            rank += (kj < key || (kj == key && ej < V)) ? 1u : 0u;
        }
    }
    if (l < n && rank < m) s[rank] = V;
    __builtin_amdgcn_wave_barrier();
    const uint32_t got = s[(l - on) & 31];
    __builtin_amdgcn_wave_barrier();
    OUT = (l >= on && l < on + m) ? got : OUT;
    x.rng = base + n;
    return on + m;
}
template <class Node>
DEV uint32_t Pas<32>::sublist(Node& x, Lds<32>& w, uint32_t k, uint32_t& OUT, uint32_t on) {
    return lite::sublist<PSIM_PASSIVE_CAP - 2>(x, w, x.pas.P, x.pas_n, k, OUT, on);
}
// the same of the two-entries-a-lane view (n <= 30): entry e draws counter
// rng + e -- each lane its two entries', two independent Philox chains
// computed in place, not through the 16-deep cache -- and is ranked among the
// row's 30 keys by two row broadcasts a source lane.  The tie test and the
// exact recount are the one-entry form's (a tie is about once in 10^7
// sublists: no scenario reaches it, so the two stay structurally the same --
// a rank slot another entry took sends the row to the recount on (key, element))
template <class Node>
DEV uint32_t Pas<16>::sublist(Node& x, Lds<16>& w, uint32_t k, uint32_t& OUT, uint32_t on) {
    const uint32_t P0 = x.pas.P0, P1 = x.pas.P1;
    const uint32_t l = G::lane(), n = x.pas_n, e0 = 2 * l, e1 = 2 * l + 1;
    const uint64_t base = x.rng;
    const uint64_t v0 = draw58_at(base + e0, x.me, kargs().seed);
    const uint64_t v1 = draw58_at(base + e1, x.me, kargs().seed);
    const uint64_t key0 = e0 < n ? v0 >> 5 : ~0ull, key1 = e1 < n ? v1 >> 5 : ~0ull;
    const uint32_t m = n < k ? n : k;
    const uint32_t hi0 = (uint32_t)(key0 >> 21), hi1 = (uint32_t)(key1 >> 21);
    uint32_t rank0 = 0, rank1 = 0;
    unroll<(PSIM_PASSIVE_CAP - 2) / 2>([&](auto J) {
        const uint32_t a = G::getc<J>(hi0), b = G::getc<J>(hi1);
        rank0 += (a < hi0 ? 1u : 0u) + (b < hi0 ? 1u : 0u);
        rank1 += (a < hi1 ? 1u : 0u) + (b < hi1 ? 1u : 0u);
    });
    uint32_t* s = w.scr;
    if (e0 < n) s[rank0] = e0;
    if (e1 < n) s[rank1] = e1;
    __builtin_amdgcn_wave_barrier();
    const uint32_t own0 = s[rank0 & 31], own1 = s[rank1 & 31];
    __builtin_amdgcn_wave_barrier();
    if (G::any((e0 < n && own0 != e0) || (e1 < n && own1 != e1))) {
        rank0 = 0; rank1 = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t ks = (j & 1u) ? key1 : key0;
            const uint32_t es = (j & 1u) ? P1 : P0;
            const uint64_t kj = G::get64(ks, j >> 1);
            const uint32_t ej = G::get(es, j >> 1);
            rank0 += (kj < key0 || (kj == key0 && ej < P0)) ? 1u : 0u;
            rank1 += (kj < key1 || (kj == key1 && ej < P1)) ? 1u : 0u;
        }
    }
    if (e0 < n && rank0 < m) s[rank0] = P0;
    if (e1 < n && rank1 < m) s[rank1] = P1;
    __builtin_amdgcn_wave_barrier();
    const uint32_t got = s[(l - on) & 31];
    __builtin_amdgcn_wave_barrier();
    OUT = (l >= on && l < on + m) ? got : OUT;
    x.rng = base + n;
    return on + m;
}

// lists:usort of E's lanes with `valid` (at most 8: lanes 0-7): E gets the
// sorted distinct values in lanes 0.., zeros above; returns their count
template <uint32_t W>
DEV uint32_t usort(Lds<W>& w, uint32_t& E, bool valid) {
    using G = Grp<W>;
    const uint32_t l = G::lane();
    const uint32_t v = valid ? E : PSIM_NONE;
    bool dup = false;
    unroll<8>([&](auto J) {
        const uint32_t vj = G::template getc<J>(v);
        dup |= ((uint32_t)J < l) & (vj == v);
    });
    const uint32_t u = valid && !dup ? v : PSIM_NONE;                 // first occurrences
    uint32_t rank = 0;
    unroll<8>([&](auto J) {
        const uint32_t uj = G::template getc<J>(u);
        rank += uj < u ? 1u : 0u;
    });
    const uint32_t c = (uint32_t)__popc(G::mask(u != PSIM_NONE));
    uint32_t* s = w.scr;
    if (u != PSIM_NONE) s[rank] = u;
    __builtin_amdgcn_wave_barrier();
    const uint32_t got = s[l];
    __builtin_amdgcn_wave_barrier();
    E = l < c ? got : 0u;
    return c;
}

// ------------------------------------------------------------- emission --
template <uint32_t W>
DEV void flush(Node<W>& x, Lds<W>& w) {
    using G = Grp<W>;
    const uint32_t l = G::lane();
    const uint32_t cnt = x.seq - x.flushed;                           // <= STAGE
    const uint32_t cap = out_cap(x);
    __builtin_amdgcn_wave_barrier();
    // 16-B piece l & 3 of record l >> 2, W / 4 records a pass
    for (uint32_t j0 = 0; j0 < cnt; j0 += G::FLUSH) {
        const uint32_t j = j0 + (l >> 2);
        if (j < cnt && x.flushed + j < cap)
            reinterpret_cast<uint4*>(kargs().rec_out + x.ob + x.flushed + j)[l & 3] =
                reinterpret_cast<const uint4*>(w.srec + j * 16)[l & 3];
    }
    if (l < cnt && x.flushed + l < cap) kargs().okey[x.ob + x.flushed + l] = w.skey[l];
    __builtin_amdgcn_wave_barrier();
    x.flushed = x.seq;
}

// one record (psim_device.h Msg) into the group's staging buffer: its lanes
// 0-15 write the 16 words, lanes 8-15 taking the exchange ids of lanes 0-7
// (DPP row_shr:8, inside the group's first row)
template <uint32_t W>
DEV void emit(Node<W>& x, Lds<W>& w, Cnt& c, uint32_t dst, uint32_t type, uint32_t ttl, uint32_t EX, uint32_t nex) {
    using G = Grp<W>;
    const uint32_t l = G::lane();
    const uint32_t k = x.seq - x.flushed;                             // < STAGE
    const uint32_t tt = type | (ttl << 8) | (nex << 16);
    const uint32_t exv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)EX, 0x118, 0xF, 0xF, true);
    const uint32_t word = l == 0 ? dst : l == 1 ? x.me : l == 2 ? tt : l == 3 ? x.seq
                        : l < 8 ? 0u : (l - 8 < nex ? exv : 0u);
    if (W == 16 || l < 16) {
        w.srec[k * 16 + l] = word;
        c.digest += (uint64_t)word * digest_mul(l);      // (l < 16: record word l's multiplier)
    }
    if (l == 0) w.skey[k] = dst | (max_emit(type) << KEY_DST_BITS);
    x.seq++;
    c.em += type == PSIM_MSG_SHUFFLE ? 1u : 0x10000u;
    if (k + 1 == G::STAGE) flush(x, w);
}

// maybe_connect + find (partisan_util.erl:75-134): the peer runs and no
// partition separates the two.  Every lite send goes to an active member
// (k_relay sends a walk that ends at a Sender outside the active view to
// k_consume), read from the connection cache; others from the pair array.
template <uint32_t W>
DEV bool connect_ok(const Node<W>& x, uint32_t dst) {
    using G = Grp<W>;
    KArgs& a = kargs();
    if (dst >= a.n_nodes || dst == x.me) return false;
    const uint32_t m = G::mask(G::lane() < x.act_n && x.A == dst);
    if (m) return (x.AF >> (__ffs(m) - 1)) & 1u;
    return (uint32_t)a.upart[dst] == ((x.fl >> 8) & 0xFFu);
}

// do_send_message/3 (hv:1274-1343) after maybe_connect: the dispatch draw of
// partisan_util:dispatch_pid/1 (util:190-195), then the record
template <uint32_t W>
DEV void hv_send(Node<W>& x, Lds<W>& w, Cnt& c, uint32_t dst, uint32_t type, uint32_t ttl, uint32_t EX, uint32_t nex) {
    if (!connect_ok(x, dst)) { c.fail++; return; }
    x.rng++;
    emit(x, w, c, dst, type, ttl, EX, nex);
}

// ------------------------------------------------------- view updates --
// merge_exchange/2 (hv:1590-1595): add_to_passive/2 (hv:1423-1448) for each
// of usort(Exchange) -- Active -- [Myself], in order, one candidate a lane.
// A full passive view evicts select_random(Passive, [Myself]) first:
// rand:uniform(|Passive|), Myself never being in Passive.  With |Passive| =
// max_passive_size at every eviction the draws are taken together (lane i:
// the i-th eviction's index); one the ?uniform_range test would reject
// (p ~ 2^-53, reached by no scenario) sends the group down the same steps
// with rand:uniform drawn one at a time, redraws included.
// sorted: EX is already usort'ed -- a SHUFFLE's exchange (hv:586: every
// shuffle start sends lists:usort(Exchange0), and relays pass it on
// unchanged) -- so the candidates are its valid lanes in order, compacted
// through LDS (no 8 x 8 rank: terminals are half of the merges)
#ifndef PSIM_MERGE_SORTED     // (0: every merge through usort, for A/B)
#define PSIM_MERGE_SORTED 1
#endif
template <uint32_t W>
DEV void merge_exchange(Node<W>& x, Lds<W>& w, uint32_t EX, uint32_t nex, bool sorted) {
    using G = Grp<W>;
    KArgs& a = kargs();
    const uint32_t l = G::lane();
    // (lanes past the active count hold PSIM_NONE, which is no id)
    const uint32_t AS = l < x.act_n ? x.A : PSIM_NONE;
    bool in_act = false;
    unroll<PSIM_ACTIVE_CAP>([&](auto J) {
        const uint32_t aj = G::template getc<J>(AS);
        in_act |= aj == EX;
    });
    uint32_t T = EX;
    const bool valid = l < nex && EX != x.me && !in_act;
    uint32_t mt;
    if (PSIM_MERGE_SORTED && sorted) {
        const uint32_t vm = G::mask(valid);
        uint32_t* sc = w.scr;
        if (valid) sc[__popc(vm & ((1u << l) - 1u))] = EX;
        __builtin_amdgcn_wave_barrier();
        mt = (uint32_t)__popc(vm);
        const uint32_t got = sc[l];
        __builtin_amdgcn_wave_barrier();
        T = l < mt ? got : 0u;
    } else {
        mt = usort(w, T, valid);
    }
    if (!mt) return;
    const uint32_t maxp = a.max_passive;
    const uint8_t* bt = a.btab;
    Pas<W> pt = x.pas.tagged(bt, x.pas_n);
    const uint32_t TG = tag_of(bt, T, l < mt);                // the candidates' tags
    const uint64_t c0 = x.rng;
    dc_cover(x, c0, mt);
    const uint32_t src = (uint32_t)(c0 - x.dcb) + l;
    const uint64_t v = ((uint64_t)G::get(x.DCH, src) << 32) | G::get(x.DCL, src);
    const uint32_t KI = mod_small_m(v, maxp, G::magic(w.KM, maxp));
    const bool par = !G::any(l < mt && v >= maxp && v - KI > (1ull << 58) - maxp);
    uint32_t used = 0, n = x.pas_n, dirty = 0;
    if (par) {
        // branch-free steps, unrolled: candidate I of the group (a no-op past
        // mt or when already a member) evicts the index in K's lane 0 when
        // the view is full, then goes in at its bucket's position
        uint32_t K = KI;                             // the next eviction's index in the group's lane 0
        uint32_t TT[PSIM_EXCHANGE_CAP];
        unroll<PSIM_EXCHANGE_CAP>([&](auto I) { TT[I] = G::template getc<I>(TG); });
        // a half's swizzles go through LDS: every candidate's tag fetched up
        // front is one LDS wait, not one a step (the half's step chain waited
        // on its swizzle each step; phase 0.505 -> 0.502 ms,
        // profiles/r05/ab_log.txt).  A row's broadcasts are VALU ops.
        if constexpr (W == 32) __builtin_amdgcn_sched_barrier(0);
        unroll<PSIM_EXCHANGE_CAP>([&](auto I) {
            const uint32_t tt = TT[I];               // (past mt: TSENT, a no-op)
            const bool mem = pt.has(tt);
            const bool ev = !mem && n >= maxp;       // select_random(Passive, [Myself]) + remove
            const uint32_t k = G::get0(K);
            const uint32_t kn = G::next(K);
            K = ev ? kn : K;
            used += ev ? 1u : 0u;
            pt.step(n, dirty, tt, mem, ev, k);
        });
    } else {
        for (uint32_t i = 0; i < mt; i++) {          // step by step, with ?uniform_range redraws
            const uint32_t tt = G::get(TG, i);
            const bool mem = pt.has(tt);
            if (mem) continue;
            const bool ev = n >= maxp;
            uint32_t k = 0;
            if (ev) {
                x.rng = c0 + used;
                k = uniform_n(x, w, n) - 1;
                used = (uint32_t)(x.rng - c0);
            }
            pt.step(n, dirty, tt, false, ev, k);
        }
    }
    x.pas_n = n;
    x.pas = pt.untagged();
    x.fl |= dirty ? HF_PDIRTY : 0u;
    x.rng = c0 + used;
}

// ---------------------------------------------------------- the node --
// With the rows by LDS-DMA a register reloaded from scratch inside the body
// costs the prefetch: scratch shares the in-order memory counter, so the wait
// for the reload waits for the DMAs.  What the node loop's functions derive
// from the lane id alone (an address offset such as 4 (l & 7), as 64 bits) the
// compiler hoists out of the loop and then spills; PER_NODE(l) has it worked
// out again per node instead, a VALU operation or two.
#if PSIM_LITE_ROWS_LDS
#define PER_NODE(l) asm volatile("" : "+v"(l))
#else
#define PER_NODE(l) do { } while (0)
#endif
// inputs of a group's node: its descriptor, header words, rows, the first
// inbox records (all lanes of a group load the same addresses, or their own
// element of a row)
template <uint32_t W>
struct In {
    uint4 D;
    uint32_t r0, r1, w9, A, part;
    typename Pas<W>::Row P;          // this lane's share of the passive row
    uint32_t cm, oe;                 // k_relay's connection bits | its emitted count << 8; obase[row + 1] (low word)
    uint32_t SRC, TT;                // lane l: sender and type word of inbox record l
    uint32_t EXP;                    // lane l: exchange id l & 7 of inbox record l >> 3
};

// (the descriptor comes from a load issued before the previous node's
// writeback: issued after those stores, its wait drained them -- the memory
// counter is in order -- at every node)
DEV uint4 load_desc(KArgs& a, const uint32_t (&lc)[4], uint32_t i, bool live) {
    return live ? a.desc_lite[lite_at(a, lc, i)] : make_uint4(0, 0, 0, 0);
}
// the node's rows: header words, active and passive rows, partition byte
// (for the next node issued after this one's body, so that they are not
// held in registers across it)
template <uint32_t W>
DEV void load_rows(KArgs& a, In<W>& in, bool live) {
    const uint32_t l = Grp<W>::lane();
    const size_t li = live ? in.D.x - a.lo : 0;
    const uint32_t* hrow = reinterpret_cast<const uint32_t*>(a.hdr + li);
    in.r0 = hrow[0]; in.r1 = hrow[1]; in.w9 = hrow[9];
    in.A = l < PSIM_ACTIVE_CAP ? a.act[li * PSIM_ACTIVE_CAP + l] : 0u;
    in.P = Pas<W>::load(a.pas + li * PSIM_PASSIVE_CAP);
    in.part = a.part[live ? in.D.x : 0];
    in.cm = a.lite_cm[li];
    in.oe = reinterpret_cast<const uint32_t*>(a.obase + li + 1)[0];   // (totals < 2^32 slots)
}
#if PSIM_LITE_ROWS_LDS
// The same rows by LDS-DMA (global_load_lds: a load with no destination
// register), so that the next node's can be issued BEFORE this node's body
// and land while it runs, holding no VGPR across it -- and with them the
// descriptor of the node after that one, whose load-and-wait otherwise sits
// behind the writeback's stores on the one in-order memory counter.  A DMA
// writes LDS at a wave-uniform base + lane x size, whatever the exec mask: the
// area is laid out by lane and is the wave's, and a group that has left the
// loop simply leaves its entries unwritten.
// Three DMAs a node, in words from the wave's area:
//   X4   one 16-B piece a lane -- a group's lanes at W * 4 * its index:
//          lanes 0-7   the passive row's eight pieces        words  0-31
//          lanes 8-9   the active row's two                         32-39
//          lanes 10-11 header words 0-3 (0, 1: the draw counter)    40-43
//                      and 8-11 (9: the view sizes)                 44-47
//          lane 12     obase[row], obase[row + 1]                   48-51
//          lanes 13..  the descriptor of the node after             52-55, ...
//        so a lane reads back its share of the passive row as from the row
//        itself (Pas<W>::load), its active entry and the group-uniform words
//   CM   lite_cm[row], 2 B zero-extended to the lane's own word: every lane of
//        the group fetches it, and reads back its own copy
//   PT   the partition byte, 1 B, likewise
// (a sub-word DMA writes a word a lane, as the load does a register.)  Every
// piece lies inside its array: no over-read of an aligned-down word.
template <uint32_t W>
struct Rows {
    static constexpr uint32_t X4 = 0, CM = 64 * 4, PT = CM + 64, WORDS = PT + 64;   // a wave's
    static constexpr uint32_t PAS = 0, ACT = 32, H0 = 40, H9 = 45, OE = 50, DESC = 52;   // in a group's X4 words
    static_assert(DESC + 4 <= W * 4, "a group's pieces: 14 lanes of its W");
};
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
// A lane's piece of the X4 DMA is base + (index << shift): the block's table
// (Carve::TAB, filled once by rows_table) holds for lane l of a group
// {base (the piece's offset in the row added), shift = log2 of the array's row
// bytes, 1 where the index is the list entry and not the node's row}.  In
// registers these would be four VGPRs live -- or spilled -- across the whole
// loop, and worked out per node a chain of selects over five pointers.
template <uint32_t W>
DEV void rows_table(KArgs& a, uint32_t* tab) {
    static_assert(PSIM_PASSIVE_CAP * 4 == 1 << 7 && PSIM_ACTIVE_CAP * 4 == 1 << 5 && sizeof(Hdr) == 1 << 6 &&
                  sizeof(*a.obase) == 1 << 3 && sizeof(*a.desc_lite) == 1 << 4, "the shifts below");
    for (uint32_t l = threadIdx.x; l < W; l += blockDim.x) {
        uint64_t b;
        uint32_t sh;
        if (l < 8) { b = (uint64_t)a.pas + l * 16; sh = 7; }
        else if (l < 10) { b = (uint64_t)a.act + (l - 8) * 16; sh = 5; }
        else if (l < 12) { b = (uint64_t)a.hdr + (l - 10) * 32; sh = 6; }
        else if (l < 13) { b = (uint64_t)a.obase; sh = 3; }
        else { b = (uint64_t)a.desc_lite; sh = 4; }
        tab[4 * l] = (uint32_t)b; tab[4 * l + 1] = (uint32_t)(b >> 32);
        tab[4 * l + 2] = sh; tab[4 * l + 3] = l < 13 ? 0u : 1u;
    }
}
// Issue the DMAs: the rows of the node of descriptor D (row 0 for a group
// without one: the result is unused) and entry `dn` of the list.  The caller
// has waited for the area's last reads.
// (`lid`: the lane id, laundered per node by the caller so that what is
// derived from it -- here and in rows_read -- is recomputed per node, a few
// VALU operations, and not hoisted out of the loop into registers held, or
// spilled, across the body: a reload after the writeback's stores waits for
// them.)
template <uint32_t W>
DEV void rows_dma(KArgs& a, const Lds<W>& w, uint32_t lid, const uint4& D, bool live, uint32_t dn) {
    using R = Rows<W>;
    const uint32_t li = live ? D.x - a.lo : 0u;
    const uint4 t = reinterpret_cast<const uint4*>(w.tab)[lid & (W - 1)];
    const uint64_t src = (((uint64_t)t.y << 32) | t.x) + ((uint64_t)(t.w ? dn : li) << t.z);
    __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(w.rows + R::X4), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(a.lite_cm + li), (lds_ptr_t)(w.rows + R::CM), 2, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(a.part + (live ? D.x : 0u)), (lds_ptr_t)(w.rows + R::PT), 1, 0, 0);
}
// the landed rows into `in` (after the wait for the DMAs)
template <uint32_t W>
DEV void rows_read(const Lds<W>& w, uint32_t lid, In<W>& in) {
    using R = Rows<W>;
    const uint32_t l = lid & (W - 1);
    const uint32_t* const g = w.rows + R::X4 + (lid & (64 - W)) * 4;   // the group's W * 4 words
    in.r0 = g[R::H0]; in.r1 = g[R::H0 + 1]; in.w9 = g[R::H9];
    in.A = g[R::ACT + (l & (PSIM_ACTIVE_CAP - 1))];
    in.A = l < PSIM_ACTIVE_CAP ? in.A : 0u;
    in.P = reinterpret_cast<const typename Pas<W>::Row*>(g + R::PAS)[l];    // (as Pas<W>::load of the row)
    in.oe = g[R::OE];                                                  // (totals < 2^32 slots)
    in.cm = w.rows[R::CM + lid] & 0xFFFFu;
    in.part = w.rows[R::PT + lid] & 0xFFu;
}

// the landed descriptor (zeros for a group without that node)
template <uint32_t W>
DEV uint4 desc_read(const Lds<W>& w, uint32_t lid, bool live) {
    using R = Rows<W>;
    const uint4 d = *reinterpret_cast<const uint4*>(w.rows + R::X4 + (lid & (64 - W)) * 4 + R::DESC);
    return live ? d : make_uint4(0, 0, 0, 0);
}
#endif
// the descriptor's inbox heads (issued a node ahead)
template <uint32_t W>
DEV In<W> load_in(KArgs& a, const uint4& D) {
    uint32_t l = Grp<W>::lane();
    PER_NODE(l);
    In<W> in;
    in.D = D;
    in.r0 = in.r1 = in.w9 = in.A = in.part = in.cm = in.oe = 0;
    in.P = {};
    // the first W records' senders and type words, the first W / 8's
    // exchanges (one load instruction each, issued a node ahead)
    const uint32_t ik = in.D.z & DESC_CNT_MASK;
    const Msg* r = a.rec_in + in.D.y + (l < ik ? l : 0u);      // (the inbox has a spare record)
    const uint2 st = *reinterpret_cast<const uint2*>(&r->src);
    in.SRC = l < ik ? st.x : 0u;
    in.TT = l < ik ? st.y : (uint32_t)PSIM_MSG_PT_BROADCAST;
    in.EXP = a.rec_in[in.D.y + ((l >> 3) < ik ? (l >> 3) : 0u)].ex[l & 7];
    return in;
}

template <uint32_t W>
DEV void begin(Node<W>& x, const In<W>& in) {
    const uint32_t l = Grp<W>::lane();
    x.me = in.D.x; x.ib = in.D.y;
    x.ik = in.D.z & DESC_CNT_MASK; x.ob = in.D.w;
    x.fl = (in.D.z >> 28) | (in.part << 8) | (in.w9 & 0xFFFF0000u);
    x.rng = ((uint64_t)in.r1 << 32) | in.r0;
    x.act_n = in.w9 & 0xFF; x.pas_n = (in.w9 >> 8) & 0xFF;
    x.A = l < x.act_n ? in.A : 0u;
    x.pas.set(in.P, x.pas_n);
    // after the records k_relay's lane emitted for the node's leading SHUFFLE
    // relays (RoundArgs::lite_cm's high byte; the inbox run starts past them)
    x.seq = in.cm >> 8; x.flushed = x.seq;
    x.dcb = ~0ull;
}

// the HyParView phase of a lite node (psim_consume.hip body_lite)
template <uint32_t W>
DEV void body(Node<W>& x, Lds<W>& w, Cnt& c, const In<W>& in) {
    using G = Grp<W>;
    KArgs& a = kargs();
    uint32_t l = G::lane();
    PER_NODE(l);
    // the inbox in canonical order, W records at a time: lane l holds record
    // cb + l's sender and type word, and the loop visits the HyParView
    // records among them (Plumtree ones are k_ptl's)
    for (uint32_t cb = 0; cb < x.ik; cb += W) {
      uint32_t SRC = in.SRC, TT = in.TT;
      if (cb) {
          const bool has = cb + l < x.ik;
          const uint2 st = *reinterpret_cast<const uint2*>(&a.rec_in[x.ib + (has ? cb + l : 0u)].src);
          SRC = has ? st.x : 0u;
          TT = has ? st.y : (uint32_t)PSIM_MSG_PT_BROADCAST;
      }
      uint32_t M = G::mask((TT & 0xFF) < PSIM_MSG_PT_BROADCAST);
      while (M) {
        const uint32_t j = (uint32_t)__ffs(M) - 1;
        M &= M - 1;
        const uint32_t p = G::get(SRC, j), tt = G::get(TT, j);
        const uint32_t ep = G::get(in.EXP, (j << 3) | (l & 7));     // (the first records: prefetched)
        const uint32_t q = cb + j;
        uint32_t ex = q < G::PREF ? ep : a.rec_in[x.ib + q].ex[l & 7];
        const uint32_t nex = (tt >> 16) & 0xFF, ttl = (tt >> 8) & 0xFF;
        const uint32_t type = tt & 0xFF;
        ex = l < nex ? ex : 0u;
        const bool reply = type == PSIM_MSG_SHUFFLE_REPLY;          // hv:1091-1093
        const bool relay = !reply && ttl > 0 && x.act_n > 1;         // hv:1095-1136
        c.dl += reply ? 0x10000u : 1u;
        LSTAMP(w, 6);
        if (relay) {
            const uint32_t r = select_random(x, w, x.A, x.act_n, p, x.me);
            if (r != PSIM_NONE) hv_send(x, w, c, r, PSIM_MSG_SHUFFLE, ttl - 1, ex, nex);
            LSTAMP(w, 1);
        } else {
            if (!reply) {                             // the walk ends here: reply to Sender
                uint32_t RESP = 0;
                const uint32_t nr = Pas<W>::sublist(x, w, nex, RESP, 0);
                LSTAMP(w, 2);
                hv_send(x, w, c, p, PSIM_MSG_SHUFFLE_REPLY, 0, RESP, nr);
                LSTAMP(w, 3);
            }
            merge_exchange(x, w, ex, nex, !reply);
            LSTAMP(w, 4);
        }
      }
    }
    if (x.fl & DESC_SHUFFLE) {                        // hv:572-607
        uint32_t EX = l == 0 ? x.me : 0u;
        uint32_t m = 1;
        m = sublist<PSIM_ACTIVE_CAP>(x, w, x.A, x.act_n, a.k_active, EX, m);
        m = Pas<W>::sublist(x, w, a.k_passive, EX, m);
        const uint32_t nex = usort(w, EX, l < m);
        const uint32_t t = select_random(x, w, x.A, x.act_n, x.me, x.me);
        if (t != PSIM_NONE) hv_send(x, w, c, t, PSIM_MSG_SHUFFLE, a.arwl, EX, nex);
        LSTAMP(w, 5);
    }
}

// a group's counters into the block's stats (once, at the kernel's end: the
// per-node LDS atomics cost a writeback's worth of issue slots)
template <uint32_t W>
DEV void count(Lds<W>& w, const Cnt& c) {
    if (Grp<W>::lane() != 0) return;
    unsigned long long* st = w.sst;
    if (c.pb & 0xFFFFu) atomicAdd(&st[ST_PROC], (unsigned long long)(c.pb & 0xFFFFu));
    if (c.pb >> 16) atomicAdd(&st[ST_BOUND], (unsigned long long)(c.pb >> 16));
    if (c.dl & 0xFFFFu) atomicAdd(&st[ST_DELIV + PSIM_MSG_SHUFFLE], (unsigned long long)(c.dl & 0xFFFFu));
    if (c.dl >> 16) atomicAdd(&st[ST_DELIV + PSIM_MSG_SHUFFLE_REPLY], (unsigned long long)(c.dl >> 16));
    if (c.em & 0xFFFFu) atomicAdd(&st[ST_EMIT + PSIM_MSG_SHUFFLE], (unsigned long long)(c.em & 0xFFFFu));
    if (c.em >> 16) atomicAdd(&st[ST_EMIT + PSIM_MSG_SHUFFLE_REPLY], (unsigned long long)(c.em >> 16));
    if (c.fail) atomicAdd(&st[ST_FAIL], (unsigned long long)c.fail);
}

// the draw counter and passive size in the header, the passive row when it
// changed, the outbox count and the records (the flag byte, the active row,
// the id maps and the Plumtree rows are unchanged)
template <uint32_t W>
DEV void writeback(Node<W>& x, Lds<W>& w, Cnt& c) {
    KArgs& a = kargs();
    const uint32_t l = Grp<W>::lane();
    const uint32_t li = local_row(x);
    uint32_t* hrow = reinterpret_cast<uint32_t*>(a.hdr + li);
    const uint32_t w9 = (x.fl & 0xFFFF0000u) | (x.pas_n << 8) | x.act_n;
    if (l < 3) hrow[l == 2 ? 9 : l] = l == 0 ? (uint32_t)x.rng : l == 1 ? (uint32_t)(x.rng >> 32) : w9;
    if (x.fl & HF_PDIRTY) x.pas.store(a.pas + (size_t)li * PSIM_PASSIVE_CAP);
    flush(x, w);
    if (l == 0) a.ocnt[li] = x.seq;
    c.pb += 1u + (x.seq > out_cap(x) ? 0x10000u : 0u);
    if ((c.dl | c.em | c.pb) & 0x80008000u) {        // (a 16-bit half past 2^15: flush early)
        count(w, c);
        c.dl = 0; c.em = 0; c.pb = 0; c.fail = 0;
    }
}

// ------------------------------------------------------- the kernel body --
// the block's LDS, in words from a 16-byte aligned base: the stats, then per
// group STAGE records of 16 words, STAGE route keys and SCR words of scratch
// (the caller carves: the kernel's own array, or k_hv_phase's, which the
// bodies of its block ranges share -- static arrays of inlined bodies add up)
template <uint32_t W>
struct Carve {
    using G = Grp<W>;
    static constexpr uint32_t SREC = (NST * 2 + 3) & ~3u, SKEY = SREC + G::WPB * G::N * G::STAGE * 16,
                              SCR = SKEY + G::WPB * G::N * G::STAGE,
#if PSIM_LITE_ROWS_LDS        // ... then per wave the Rows<W> area of the next node's rows
                              // and the block's table of the pieces (rows_table)
                              ROWS = SCR + G::WPB * G::N * G::SCR, TAB = ROWS + G::WPB * Rows<W>::WORDS,
                              WORDS = TAB + W * 4;
    static_assert(ROWS % 4 == 0 && TAB % 4 == 0, "the DMA's 16-B pieces, the table's 16-B entries");
#else
                              WORDS = SCR + G::WPB * G::N * G::SCR;
#endif
    // four blocks a CU stay resident (4 waves/SIMD in blocks of four waves): 160 KiB / 4
    static_assert(WORDS * 4 <= 40960, "the block's LDS: four blocks of it per CU at 4 waves/SIMD");
};
// Block `bid` of `nblk`: the launch's own index and grid in k_lite_quarter /
// k_lite_half, the lite range's in k_hv_phase (psim_consume.hip).
template <uint32_t W>
DEV void lite_kernel(const uint32_t bid, const uint32_t nblk, uint32_t* const pool) {
    using G = Grp<W>;
    constexpr uint32_t WPB = G::WPB, STAGE = G::STAGE;
    // the LDS carve of a wave: per group STAGE records of 16 words, STAGE
    // route keys and SCR words of scratch
    static_assert(STAGE >= 1 && STAGE <= 16, "flush writes a group's staged route keys one per lane");
    static_assert((STAGE * 16 * 4) % 16 == 0, "a group's staging area is read in 16-B pieces");
    static_assert(sizeof(Msg) == 16 * 4, "a record is one word per lane of a group's first row");
    static_assert(PSIM_PASSIVE_CAP == 32, "the passive row is one entry a lane of a half, two a lane of a row");
    static_assert(PSIM_ACTIVE_CAP <= 8 && PSIM_EXCHANGE_CAP == 8,
                  "a record's exchange ids move from lanes 0-7 to lanes 8-15 (row_shr:8)");
    static_assert(G::SCR >= PSIM_PASSIVE_CAP, "a sublist scatters one word per passive entry");
    static_assert(WPB * G::N * (STAGE * 16 + STAGE + G::SCR) * 4 + NST * 8 <= 64 * 1024,
                  "the block's LDS: four blocks of it per CU at 4 waves/SIMD");
    if (*kargs().ctl) return;                         // an aborted batch (run_batch)
    unsigned long long* const sst = reinterpret_cast<unsigned long long*>(pool);
    uint32_t* const srecs = pool + Carve<W>::SREC;
    uint32_t* const skeys = pool + Carve<W>::SKEY;
    uint32_t* const scrs = pool + Carve<W>::SCR;
#ifdef PSIM_STAMPS
    __shared__ unsigned long long stls[WPB][32];
    for (int i = threadIdx.x; i < (int)(WPB * 32); i += blockDim.x) (&stls[0][0])[i] = 0;
#endif
    for (int i = threadIdx.x; i < NST; i += blockDim.x) sst[i] = 0;
#if PSIM_LITE_ROWS_LDS
    rows_table<W>(kargs(), pool + Carve<W>::TAB);
#endif
    __syncthreads();
    const uint32_t wid = threadIdx.x >> 6, g = G::idx();
    Lds<W> w;
    w.sst = sst;
    w.srec = srecs + (wid * G::N + g) * (STAGE * 16);
    w.skey = skeys + (wid * G::N + g) * STAGE;
    w.scr = scrs + (wid * G::N + g) * G::SCR;
    w.KM = G::magic_lanes();
#ifdef PSIM_STAMPS
    w.stl = stls[wid];
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    Cnt c = {};
    // group g of global wave gw takes list entries N gw + g, + N nw, ...
    const uint32_t nw = nblk * WPB;
    const uint32_t first = G::N * (bid * WPB + wid) + g;
    const uint32_t step = G::N * nw;
    uint32_t lc[4], na;
    lite_counts(kargs(), lc, na);
#if PSIM_LITE_ROWS_LDS        // (the list's counts are wave-uniform: in SGPRs, not in VGPRs that spill)
    for (uint32_t k = 0; k < 4; k++) lc[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)lc[k]);
    na = lc[0] + lc[1] + lc[2] + lc[3];
    // (the area's base is wave-uniform: the DMAs' M0)
    w.rows = pool + Carve<W>::ROWS + (uint32_t)__builtin_amdgcn_readfirstlane((int)wid) * Rows<W>::WORDS;
    w.tab = pool + Carve<W>::TAB;
    // The memory counter (vmcnt) is one, in order, for loads, DMAs and stores,
    // and the waits on the DMAs are this loop's own:
    //   top     the area's reads of node i, which begin() consumes; the inbox
    //           heads of node i + 1 (ordinary loads, as before); a wait for
    //           the reads (lgkmcnt) and then the DMAs of node i + 1's rows and
    //           node i + 2's descriptor, which overwrite the area
    //   body    the DMAs land behind it.  An ordinary load's result used in it
    //           (an inbox past W records, an exchange past PREF, connect_ok's
    //           pair) waits for the DMAs too: correct, and rare
    //   end     one wait for everything, before the writeback's stores; the
    //           inbox heads are taken here (`pin`), since a use the compiler
    //           sinks past the stores waits for those too, and the descriptor
    //           is read from the area
    // so that nothing waits on the stores but the next node's end-of-body wait.
    if (first < na) {
        Node<W> x;
        In<W> in = load_in<W>(kargs(), load_desc(kargs(), lc, first, true));
        rows_dma(kargs(), w, __lane_id(), in.D, true, lite_at(kargs(), lc, first + step < na ? first + step : first));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint4 Dn = desc_read(w, __lane_id(), first + step < na);
        for (uint32_t i = first; i < na; i += step) {
            LSTAMP(w, 8);
            uint32_t lid = __lane_id();
            PER_NODE(lid);
            rows_read(w, lid, in);
            begin(x, in);
            // the connection bits and the outbox bound, fetched with the rows
            x.AF = (in.cm & 0xFFu) | (min(in.oe - x.ob, 0xFFFFFFu) << 8);
            // the next node's inputs, in flight while this one runs
            const uint32_t nx = i + step, nnx = i + 2 * step;
            In<W> inn = load_in<W>(kargs(), Dn);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            rows_dma(kargs(), w, lid, Dn, nx < na, lite_at(kargs(), lc, nnx < na ? nnx : i));
            LSTAMP(w, 0);
            body(x, w, c, in);
            LSTAMP(w, 9);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(inn.SRC), "+v"(inn.TT), "+v"(inn.EXP));   // pin
            Dn = desc_read(w, lid, nnx < na);
            writeback(x, w, c);
            LSTAMP(w, 7);
            in = inn;
        }
        count(w, c);
    }
#else
    if (first < na) {
        Node<W> x;
        In<W> in = load_in<W>(kargs(), load_desc(kargs(), lc, first, true));
        load_rows(kargs(), in, true);
        uint4 Dn = load_desc(kargs(), lc, first + step < na ? first + step : first, first + step < na);
        for (uint32_t i = first; i < na; i += step) {
            LSTAMP(w, 8);
            begin(x, in);
            // the connection bits and the outbox bound, loaded with the rows
            x.AF = (in.cm & 0xFFu) | (min(in.oe - x.ob, 0xFFFFFFu) << 8);
            // the next node's inputs, in flight while this one runs
            const uint32_t nx = i + step, nnx = i + 2 * step;
            In<W> inn = load_in<W>(kargs(), Dn);
            LSTAMP(w, 0);
            body(x, w, c, in);
            LSTAMP(w, 9);
            Dn = load_desc(kargs(), lc, nnx < na ? nnx : i, nnx < na);
            load_rows(kargs(), inn, nx < na);
            writeback(x, w, c);
            LSTAMP(w, 7);
            in = inn;
        }
        count(w, c);
    }
#endif
    // the digest partials of every lane
    {
        uint64_t dg = c.digest;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dg += __shfl_xor(dg, off);
        if (__lane_id() == 0 && dg) atomicAdd(&sst[ST_DIGEST], (unsigned long long)dg);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NST; i += blockDim.x)
        kargs().stat_lite[(size_t)bid * NST + i] = sst[i];
#ifdef PSIM_STAMPS
    if (threadIdx.x < 32) {
        unsigned long long t = 0;
        for (uint32_t k = 0; k < WPB; k++) t += stls[k][threadIdx.x];
        if (t) atomicAdd(&g_stamps_half[threadIdx.x], t);
    }
#endif
}

}  // namespace
}  // namespace lite
}  // namespace psim
