// psim_metrics.hip -- the read-only analyses of the overlay behind eight
// getters of include/partisan_gpu_sim.h; no round runs any of it:
//   psim_get_histograms           HyParView's views, the tracked broadcast, components
//   psim_get_strategy_histograms  the pluggable strategies' views (SCAMP's as a CSR)
//   psim_get_graph_metrics        clustering, and a BFS from 64 sources at once
//   psim_get_resilience           that BFS over 64 mass-failure cases
//   psim_get_gossip_reach         ... pushed over at most `fanout` links a node
//   psim_get_tree_metrics         a Plumtree root's eager tree against the overlay
//   psim_get_relay_reach          the transitive unicast's relay flood, 64 cases
//   psim_get_latency_metrics      link costs, cheapest paths by latency from 64 sources
// Each waits for every shard's stream, works on the first shard's, and is a
// collective on ranks.  Shared by the analyses: Links (a link set as rows) and
// link_set (its host side), tree_set (a root's eager links), bfs_levels (the
// word BFS's level loop), wave_or / tile_add (per-bit counts of a wave's
// words), getter_begin, level_cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psim_host.h"
#include "psim_wave.h"

using namespace psim;

namespace {

// A link set as rows: node i's cnt[i] ids at adj + off[i] -- a CSR: the
// pluggable handles' overlay, a broadcast tree -- or, off == nullptr, at
// adj + i * PSIM_ACTIVE_CAP: HyParView's rows.
struct Links {
    const uint32_t* off;
    const uint8_t* cnt;
    const uint32_t* adj;
    DEV size_t slot(uint32_t i) const { return off ? (size_t)off[i] : (size_t)i * PSIM_ACTIVE_CAP; }   // of i's first link
    DEV const uint32_t* row(uint32_t i) const { return adj + slot(i); }
    DEV const uint32_t* csr_row(uint32_t i) const { return adj + off[i]; }   // (a kernel of one form only: no test)
    DEV const uint32_t* hv_row(uint32_t i) const { return adj + (size_t)i * PSIM_ACTIVE_CAP; }
};

DEV uint32_t sh_wave_sum(uint32_t v) {
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
DEV uint64_t wave_or(uint64_t w) {
    uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
    for (int d = 32; d; d >>= 1) { lo |= (uint32_t)__shfl_xor((int)lo, d); hi |= (uint32_t)__shfl_xor((int)hi, d); }
    return ((uint64_t)hi << 32) | lo;
}
// the wave's lanes holding bit j of w, for every j of todo = wave_or(w), into
// the block's 64-word tile: one ballot per such bit
DEV void tile_add(unsigned long long* tile, uint64_t w, uint64_t todo) {
    while (todo) {                                    // (uniform)
        const int j = ffs64(todo);
        todo &= todo - 1;
        const uint32_t c = popc(ballot((w >> j) & 1));
        if (lane_id() == 0) atomicAdd(&tile[j], (unsigned long long)c);
    }
}
DEV void tile_add(unsigned long long* tile, uint64_t w) { tile_add(tile, w, wave_or(w)); }
// A lane's count of up to 255 words per bit, as 8 counter planes: plane b
// holds bit b of the count of every bit j.  plane_inc counts the word m;
// tile_add_planes adds the wave's counts of every bit j of todo into the tile
DEV void plane_inc(unsigned long long (&pl)[8], unsigned long long m) {
#pragma unroll
    for (int b = 0; b < 8; b++) { const unsigned long long t = pl[b] & m; pl[b] ^= m; m = t; }
}
DEV void tile_add_planes(unsigned long long* tile, const unsigned long long (&pl)[8], uint64_t todo) {
    while (todo) {                                    // (uniform)
        const int j = ffs64(todo);
        todo &= todo - 1;
        uint32_t s = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) s += popc(ballot((pl[b] >> j) & 1)) << b;
        if (lane_id() == 0) atomicAdd(&tile[j], (unsigned long long)s);
    }
}

// --------------------------------------------------------- overlay stats --
// psim_get_histograms: per live node its view sizes, the in-degree links it
// contributes (global id arrays, summed over shards / RCCL ranks) and the
// tracked broadcast's delivery.  hist layout: 5 histograms of
// PSIM_HIST_BINS, then n_up, delivered, last_round, active_links.
enum { H_AIN = 0, H_PIN = 1, H_AOUT = 2, H_PFILL = 3, H_HOP = 4, H_NUP = 5 * PSIM_HIST_BINS,
       H_DELIV, H_LAST, H_LINKS, H_N };

__device__ __forceinline__ uint32_t hbin(uint32_t v) { return v < PSIM_HIST_BINS ? v : PSIM_HIST_BINS - 1; }

__global__ void k_hist_out(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ act,
                           const uint32_t* __restrict__ pas, const uint8_t* __restrict__ flags, uint32_t lo,
                           uint32_t n, uint64_t tbit, uint32_t* indeg_a, uint32_t* indeg_p,
                           unsigned long long* hist) {
    __shared__ unsigned long long sh[H_N];
    for (uint32_t j = threadIdx.x; j < H_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (flags[lo + i] & F_UP)) {
        const Hdr& x = hdr[i];
        const uint32_t me = lo + i;
        uint32_t out = 0;
        for (uint32_t k = 0; k < x.act_n; k++) {
            const uint32_t p = act[(size_t)i * PSIM_ACTIVE_CAP + k];
            if (p == me) continue;
            out++;
            if (flags[p] & F_UP) { atomicAdd(&indeg_a[p], 1u); atomicAdd(&sh[H_LINKS], 1ull); }
        }
        for (uint32_t k = 0; k < x.pas_n; k++) {
            const uint32_t p = pas[(size_t)i * PSIM_PASSIVE_CAP + k];
            if (p != me && (flags[p] & F_UP)) atomicAdd(&indeg_p[p], 1u);
        }
        atomicAdd(&sh[H_AOUT * PSIM_HIST_BINS + hbin(out)], 1ull);
        atomicAdd(&sh[H_PFILL * PSIM_HIST_BINS + hbin(x.pas_n)], 1ull);
        atomicAdd(&sh[H_NUP], 1ull);
        if (tbit && ((((uint64_t)x.aux << 32) | x.have) & tbit)) {
            atomicAdd(&sh[H_DELIV], 1ull);
            atomicAdd(&sh[H_HOP * PSIM_HIST_BINS + hbin(x.trk_hop)], 1ull);
            if (x.trk_round != PSIM_NONE) atomicMax(&sh[H_LAST], (unsigned long long)x.trk_round);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < H_N; j += blockDim.x) {
        if (!sh[j]) continue;
        if (j == H_LAST) atomicMax(&hist[j], sh[j]);
        else atomicAdd(&hist[j], sh[j]);
    }
}

__global__ void k_hist_in(const uint32_t* __restrict__ indeg_a, const uint32_t* __restrict__ indeg_p,
                          const uint8_t* __restrict__ flags, uint32_t lo, uint32_t n, unsigned long long* hist) {
    __shared__ unsigned long long sh[2 * PSIM_HIST_BINS];
    for (uint32_t j = threadIdx.x; j < 2 * PSIM_HIST_BINS; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (flags[lo + i] & F_UP)) {
        atomicAdd(&sh[hbin(indeg_a[lo + i])], 1ull);
        atomicAdd(&sh[PSIM_HIST_BINS + hbin(indeg_p[lo + i])], 1ull);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < 2 * PSIM_HIST_BINS; j += blockDim.x)
        if (sh[j]) atomicAdd(&hist[H_AIN * PSIM_HIST_BINS + j], sh[j]);
}

// the whole overlay's active rows (gathered from every shard / RCCL rank into
// gact / gan by global id): reverse-link test and label propagation over live
// active links (min label, then pointer jumping)
__global__ void k_pack_act(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ act, uint32_t n,
                           uint32_t* gact, uint8_t* gan) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = hdr[i].act_n;
    gan[i] = (uint8_t)k;
    for (uint32_t j = 0; j < PSIM_ACTIVE_CAP; j++) gact[(size_t)i * PSIM_ACTIVE_CAP + j] = act[(size_t)i * PSIM_ACTIVE_CAP + j];
}

__global__ void k_hist_sym(const uint8_t* __restrict__ gan, const uint32_t* __restrict__ act,
                           const uint8_t* __restrict__ flags, uint32_t n, unsigned long long* sym) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !(flags[i] & F_UP)) return;
    uint32_t c = 0;
    for (uint32_t k = 0; k < gan[i]; k++) {
        const uint32_t p = act[(size_t)i * PSIM_ACTIVE_CAP + k];
        if (p == i || p >= n || !(flags[p] & F_UP)) continue;
        for (uint32_t q = 0; q < gan[p]; q++)
            if (act[(size_t)p * PSIM_ACTIVE_CAP + q] == i) { c++; break; }
    }
    if (c) atomicAdd(sym, (unsigned long long)c);
}

__global__ void k_cc_init(const uint8_t* __restrict__ flags, uint32_t n, uint32_t* L) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) L[i] = (flags[i] & F_UP) ? i : PSIM_NONE;
}

// (the rows may be unfiltered: psim_get_histograms hands over the gathered active rows)
// Hooks roots, not labels: the two ends' trees are followed to their roots
// and the larger root is put under the smaller.  L[x] <= x always and a word
// only ever falls, so L stays a forest; a root another thread lowered in the
// meantime keeps the lower of the two (the link lost that way is found again:
// `changed` is set, and the loop ends only after a pass that changed nothing)
__global__ void k_cc_hook(Links ln, const uint8_t* __restrict__ flags, uint32_t n, uint32_t* L, uint32_t* changed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !(flags[i] & F_UP)) return;
    const uint32_t* row = ln.row(i);
    for (uint32_t k = 0, c = ln.cnt[i]; k < c; k++) {
        const uint32_t p = row[k];
        if (p == i || p >= n || !(flags[p] & F_UP)) continue;
        uint32_t a = L[i], b = L[p];
        if (a == b) continue;                         // (one parent: one tree)
        while (L[a] != a) a = L[a];
        while (L[b] != b) b = L[b];
        if (a == b) continue;
        const uint32_t lo = min(a, b), hi = max(a, b);
        atomicMin(&L[hi], lo);
        *changed = 1;
    }
}

// Every live node to its root.  A hook pass can leave a chain as deep as the
// overlay is long (a path whose ids fall along it: j under j - 1 for every j),
// and a thread that walked it alone would read the whole chain: n * depth
// loads a pass.  So a node publishes each ancestor it reaches as its own
// parent at once, and a walk that comes by takes the other's progress as its
// next step: threads that advance together double their reach a step, as
// pointer jumping does, without a launch a round.  A word only ever moves to
// an ancestor of its node, so any mix of old and new reads ends at the root.
// The passes of cc_run are few (logarithmic when the hooks halve the roots);
// the work of one is n log(depth) loads at best and n * depth at worst
__global__ void k_cc_jump(uint32_t n, uint32_t* L) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || L[i] == PSIM_NONE) return;
    uint32_t r = L[i];
    for (;;) {
        const uint32_t g = __atomic_load_n(&L[r], __ATOMIC_RELAXED);
        if (g == r) break;
        r = g;
        __atomic_store_n(&L[i], r, __ATOMIC_RELAXED);
    }
}

__global__ void k_cc_count(const uint32_t* __restrict__ L, uint32_t n, uint32_t* size, unsigned long long* comps) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || L[i] == PSIM_NONE) return;
    atomicAdd(&size[L[i]], 1u);
    if (L[i] == i) atomicAdd(comps, 1ull);
}

__global__ void k_cc_max(const uint32_t* __restrict__ size, uint32_t n, unsigned long long* largest) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && size[i]) atomicMax(largest, (unsigned long long)size[i]);
}

// ------------------------------------------ overlay stats, pluggable --
// psim_get_strategy_histograms.  A SCAMP row is PSIM_SVIEW_CAP ids with ~3 in
// use, so the whole overlay is packed into a CSR instead of gathering rows:
//   k_sh_rows (count)  a wave takes 64 local nodes and holds one view at a time
//                      as two 64-lane registers (only the lanes below its
//                      length load), marks
//                      first occurrences, self and live targets, counts the
//                      per-node statistics and writes the node's number of
//                      distinct live targets != self (a byte, by global id)
//   scan_excl          the counts (all-gathered across ranks) -> row offsets
//   k_sh_rows (pack)   the same wave writes those targets at its offset
//   k_sh_links / k_sh_in / k_sh_inv / k_cc_*   statistics over the CSR
// sl layout (summed over ranks; SL_VMAX: max): three histograms, then scalars
enum { SL_VFILL = 0, SL_IFILL = 1, SL_OUT = 2, SL_NUP = 3 * PSIM_HIST_BINS, SL_VSUM, SL_ISUM, SL_DANG, SL_SELF,
       SL_DUP, SL_IVL, SL_IVC, SL_VMAX, SL_N };
// sg layout (over the whole CSR, the same on every rank): the in-degree
// histogram, then scalars
enum { SG_LINKS = PSIM_HIST_BINS, SG_MUTUAL, SG_INMAX, SG_ISOL, SG_COMPS, SG_LARGEST, SG_N };
// full strategy
enum { SF_NUP = 0, SF_MIN, SF_MAX, SF_SUM, SF_AGREE, SF_N };
constexpr uint32_t SH_NPB = BLK;      // nodes a k_sh_rows / k_sh_inv block takes: 64 a wave

// a row of n <= PSIM_SVIEW_CAP ids, entry l in lane l of `a`, entry 64 + l in
// lane l of `b` (lanes past n: PSIM_NONE, never loaded)
DEV void sh_row_load(const uint32_t* __restrict__ row, uint32_t n, uint32_t& a, uint32_t& b) {
    const uint32_t l = lane_id();
    a = l < n ? row[l] : PSIM_NONE;
    b = n > 64 && 64 + l < n ? row[64 + l] : PSIM_NONE;
}
// fa / fb: the lane's entry is the first occurrence of its id in the row
DEV void sh_row_first(uint32_t a, uint32_t b, uint32_t n, bool& fa, bool& fb) {
    const uint32_t l = lane_id();
    fa = l < n; fb = 64 + l < n;
    for (uint32_t j = 0; j + 1 < n; j++) {            // (uniform: n is)
        const uint32_t v = j < 64 ? shfl(a, (int)j) : shfl(b, (int)(j - 64));
        if (l > j && a == v) fa = false;
        if (64 + l > j && b == v) fb = false;
    }
}
DEV bool sh_live(const uint8_t* __restrict__ flags, uint32_t N, uint32_t id) {
    return id < N && (flags[id] & F_UP);
}

// off == nullptr: the count pass (statistics into sl, the node's link count
// into cnt[lo + i]); else the pack pass (the links into adj at off[lo + i])
__global__ void __launch_bounds__(BLK) k_sh_rows(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ sview,
                                                 const uint8_t* __restrict__ flags, uint32_t lo, uint32_t n,
                                                 uint32_t N, uint32_t v2, uint8_t* cnt,
                                                 const uint32_t* __restrict__ off, uint32_t* adj,
                                                 unsigned long long* sl) {
    __shared__ unsigned long long sh[SL_N];
    for (uint32_t j = threadIdx.x; j < SL_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t l = lane_id();
    const uint32_t base = blockIdx.x * SH_NPB + (threadIdx.x >> 6) * 64;     // this wave's first node
    const uint32_t mine = base + l;
    uint32_t vn = 0, in_n = 0, o = 0, my_cnt = 0;
    if (mine < n && (flags[lo + mine] & F_UP)) {
        vn = min((uint32_t)hdr[mine].act_n, (uint32_t)PSIM_SVIEW_CAP);
        in_n = hdr[mine].pas_n;
        if (off) o = off[lo + mine];
    }
    const uint64_t up = ballot(mine < n && (flags[lo + mine] & F_UP));
    uint64_t todo = off ? ballot(vn != 0) : up;
    unsigned long long s_vsum = 0, s_isum = 0, s_dang = 0, s_self = 0, s_dup = 0, s_vmax = 0;
    while (todo) {                                    // (uniform)
        const int k = ffs64(todo);
        todo &= todo - 1;
        const uint32_t i = base + (uint32_t)k, me = lo + i;
        const uint32_t len = shfl(vn, k);
        uint32_t a, b;
        bool fa, fb;
        sh_row_load(sview + (size_t)i * PSIM_SVIEW_CAP, len, a, b);
        sh_row_first(a, b, len, fa, fb);
        const uint64_t oa = ballot(fa && a != me), ob = ballot(fb && b != me);
        const uint64_t la = ballot(fa && a != me && sh_live(flags, N, a));
        const uint64_t lb = ballot(fb && b != me && sh_live(flags, N, b));
        if (off) {
            const uint32_t at = shfl(o, k);
            if ((la >> l) & 1) adj[at + popc(la & lt_mask())] = a;
            if ((lb >> l) & 1) adj[at + popc(la) + popc(lb & lt_mask())] = b;
            continue;
        }
        const uint32_t links = popc(la) + popc(lb), others = popc(oa) + popc(ob);
        const uint32_t distinct = popc(ballot(fa)) + popc(ballot(fb));
        if (l == (uint32_t)k) my_cnt = links;
        s_vsum += len; s_dang += others - links; s_self += distinct - others; s_dup += len - distinct;
        s_vmax = len > s_vmax ? len : s_vmax;
        const uint32_t inn = v2 ? shfl(in_n, k) : 0;
        s_isum += inn;
        if (l == 0) {
            atomicAdd(&sh[SL_VFILL * PSIM_HIST_BINS + hbin(len)], 1ull);
            atomicAdd(&sh[SL_OUT * PSIM_HIST_BINS + hbin(others)], 1ull);
            if (v2) atomicAdd(&sh[SL_IFILL * PSIM_HIST_BINS + hbin(inn)], 1ull);
        }
    }
    if (off) return;
    if (mine < n) cnt[lo + mine] = (uint8_t)my_cnt;
    if (l == 0) {
        atomicAdd(&sh[SL_NUP], (unsigned long long)popc(up));
        atomicAdd(&sh[SL_VSUM], s_vsum); atomicAdd(&sh[SL_ISUM], s_isum); atomicAdd(&sh[SL_DANG], s_dang);
        atomicAdd(&sh[SL_SELF], s_self); atomicAdd(&sh[SL_DUP], s_dup); atomicMax(&sh[SL_VMAX], s_vmax);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < SL_N; j += blockDim.x) {
        if (!sh[j]) continue;
        if (j == SL_VMAX) atomicMax(&sl[j], sh[j]);
        else atomicAdd(&sl[j], sh[j]);
    }
}

// is `id` in node p's CSR row?
DEV bool sh_has(Links ln, uint32_t p, uint32_t id) {
    const uint32_t* row = ln.csr_row(p);
    for (uint32_t q = 0, c = ln.cnt[p]; q < c; q++)
        if (row[q] == id) return true;
    return false;
}

// scamp v2: the in_view rows of the local nodes against the CSR -- the
// distinct live (i, j != i) with j in i's in_view, and those with j -> i a link
__global__ void __launch_bounds__(BLK) k_sh_inv(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ sinv,
                                                const uint8_t* __restrict__ flags, uint32_t lo, uint32_t n,
                                                uint32_t N, Links ln, unsigned long long* sl) {
    const uint32_t l = lane_id();
    const uint32_t base = blockIdx.x * SH_NPB + (threadIdx.x >> 6) * 64;
    const uint32_t mine = base + l;
    uint32_t in_n = 0;
    if (mine < n && (flags[lo + mine] & F_UP)) in_n = min((uint32_t)hdr[mine].pas_n, (uint32_t)PSIM_SVIEW_CAP);
    uint64_t todo = ballot(in_n != 0);
    uint32_t ivl = 0, ivc = 0;                        // (per lane)
    while (todo) {                                    // (uniform)
        const int k = ffs64(todo);
        todo &= todo - 1;
        const uint32_t i = base + (uint32_t)k, me = lo + i;
        const uint32_t len = shfl(in_n, k);
        uint32_t a, b;
        bool fa, fb;
        sh_row_load(sinv + (size_t)i * PSIM_SVIEW_CAP, len, a, b);
        sh_row_first(a, b, len, fa, fb);
        if (fa && a != me && sh_live(flags, N, a)) { ivl++; ivc += sh_has(ln, a, me) ? 1u : 0u; }
        if (fb && b != me && sh_live(flags, N, b)) { ivl++; ivc += sh_has(ln, b, me) ? 1u : 0u; }
    }
    ivl = sh_wave_sum(ivl); ivc = sh_wave_sum(ivc);
    if (l == 0 && ivl) atomicAdd(&sl[SL_IVL], (unsigned long long)ivl);
    if (l == 0 && ivc) atomicAdd(&sl[SL_IVC], (unsigned long long)ivc);
}

// per rank r (one thread): its first row offset base[r] = E[r * per] and, in
// tot[0], the largest number of links a rank holds (E: the exclusive scan of
// the counts, npad + 1 entries)
__global__ void k_sh_rank_tot(const uint32_t* __restrict__ E, uint32_t per, uint32_t W, uint32_t npad,
                              uint32_t* base, unsigned long long* tot) {
    if (blockIdx.x || threadIdx.x) return;
    unsigned long long mx = 0;
    for (uint32_t r = 0; r < W; r++) {
        const uint32_t b = E[min(npad, r * per)], e = E[min(npad, (r + 1) * per)];
        base[r] = b;
        mx = max(mx, (unsigned long long)(e - b));
    }
    tot[0] = mx;
}
// rank r's rows start at r * slot: E[i] -> the row's place in the gathered CSR
__global__ void k_sh_shift(uint32_t* E, uint32_t npad, uint32_t per, uint32_t slot,
                           const uint32_t* __restrict__ base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    const uint32_t r = i / per;
    E[i] = E[i] - base[r] + r * slot;
}

// the CSR's links: in-degrees, the link count, the links whose reverse exists
__global__ void k_sh_links(Links ln, uint32_t n, uint32_t* indeg, unsigned long long* sg) {
    __shared__ unsigned long long sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = i < n ? ln.cnt[i] : 0;
    if (c) {
        const uint32_t* row = ln.csr_row(i);
        uint32_t m = 0;
        for (uint32_t k = 0; k < c; k++) {
            const uint32_t p = row[k];
            if (p >= n) continue;                     // (never: the pack pass keeps live ids < N)
            atomicAdd(&indeg[p], 1u);
            m += sh_has(ln, p, i) ? 1u : 0u;
        }
        atomicAdd(&sh[0], (unsigned long long)c);
        if (m) atomicAdd(&sh[1], (unsigned long long)m);
    }
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(&sg[SG_LINKS + threadIdx.x], sh[threadIdx.x]);
}

__global__ void k_sh_in(const uint32_t* __restrict__ indeg, const uint8_t* __restrict__ cnt,
                        const uint8_t* __restrict__ flags, uint32_t n, unsigned long long* sg) {
    __shared__ unsigned long long sh[SG_ISOL + 1];
    for (uint32_t j = threadIdx.x; j <= SG_ISOL; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (flags[i] & F_UP)) {
        const uint32_t d = indeg[i];
        atomicAdd(&sh[hbin(d)], 1ull);
        atomicMax(&sh[SG_INMAX], (unsigned long long)d);
        if (!d && !cnt[i]) atomicAdd(&sh[SG_ISOL], 1ull);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j <= SG_ISOL; j += blockDim.x) {
        if (!sh[j]) continue;                         // (the link words stay zero here: k_sh_links')
        if (j == SG_INMAX) atomicMax(&sg[j], sh[j]);
        else atomicAdd(&sg[j], sh[j]);
    }
}

// full strategy: the lowest live id (low: preset to PSIM_NONE; the flags are
// replicated, so any shard finds it), then a wave per node over its member
// row -- |add & ~remove| and its equality with the lowest live node's (ref:
// that row, wherever it lives); the remove halves are read only once a
// removal exists
__global__ void k_sh_low(const uint8_t* __restrict__ flags, uint32_t lo, uint32_t n, uint32_t* low) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (flags[lo + i] & F_UP)) atomicMin(low, i);
}
__global__ void __launch_bounds__(BLK) k_sh_full(const uint32_t* __restrict__ fbits, const uint8_t* __restrict__ flags,
                                                 uint32_t lo, uint32_t n, uint32_t fw, uint32_t tomb,
                                                 const uint32_t* __restrict__ ref, unsigned long long* sf) {
    const uint32_t i = blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);         // (uniform per wave)
    if (i >= n || !(flags[lo + i] & F_UP)) return;
    const uint32_t* row = fbits + (size_t)i * 2 * fw;
    uint32_t c = 0;
    bool differs = false;
    for (uint32_t w = lane_id(); w < fw; w += 64) {
        const uint32_t q = tomb ? row[w] & ~row[fw + w] : row[w];
        const uint32_t r = tomb ? ref[w] & ~ref[fw + w] : ref[w];
        c += (uint32_t)__popc(q);
        differs |= q != r;
    }
    c = sh_wave_sum(c);
    const bool agree = ballot(differs) == 0;
    if (lane_id() == 0) {
        atomicAdd(&sf[SF_NUP], 1ull);
        atomicMin(&sf[SF_MIN], (unsigned long long)c);
        atomicMax(&sf[SF_MAX], (unsigned long long)c);
        atomicAdd(&sf[SF_SUM], (unsigned long long)c);
        if (agree) atomicAdd(&sf[SF_AGREE], 1ull);
    }
}

// ------------------------------------- path lengths and clustering --
// psim_get_graph_metrics.  Every kernel reads the link set L as Links: the
// pluggable handles' CSR as k_sh_rows packs it (distinct, != i, live), or
// HyParView's rows after k_gm_filter (the same three properties).
//   k_gm_cluster_hv / k_gm_cluster   closed_i = sum over a in N(i) of
//                      |N(a) & N(i)| (no row holds its own node, so b != a)
//   k_gm_init / k_gm_push / k_gm_level   the bit-parallel BFS: bit j of a
//                      node's word = reached from source slot j
enum { GM_NUP = 0, GM_LINKS, GM_NODES, GM_CLOSED, GM_PAIRS, GM_Q32, GM_N };
constexpr uint32_t GM_TAB = 256;      // k_gm_cluster: hash slots a wave keeps for one N(i) (<= PSIM_SVIEW_CAP ids)

__global__ void k_gm_filter(const uint8_t* __restrict__ gan, const uint32_t* __restrict__ gact,
                            const uint8_t* __restrict__ flags, uint32_t n, uint32_t* fadj, uint8_t* fcnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0;
    if (flags[i] & F_UP) {
        const uint32_t* row = gact + (size_t)i * PSIM_ACTIVE_CAP;
        const uint32_t len = min((uint32_t)gan[i], (uint32_t)PSIM_ACTIVE_CAP);
        for (uint32_t k = 0; k < len; k++) {
            const uint32_t p = row[k];
            if (p == i || p >= n || !(flags[p] & F_UP)) continue;
            bool dup = false;
            for (uint32_t q = 0; q < k; q++) dup |= row[q] == p;
            if (!dup) fadj[(size_t)i * PSIM_ACTIVE_CAP + c++] = p;
        }
    }
    fcnt[i] = (uint8_t)c;
}

// a node's share of the clustering sums, into the block's LDS words
DEV void gm_cluster_add(unsigned long long* sh, uint32_t k, uint32_t closed) {
    atomicAdd(&sh[GM_NUP], 1ull);
    if (k) atomicAdd(&sh[GM_LINKS], (unsigned long long)k);
    if (k < 2) return;
    const unsigned long long pairs = (unsigned long long)k * (k - 1);
    atomicAdd(&sh[GM_NODES], 1ull);
    atomicAdd(&sh[GM_PAIRS], pairs);
    if (closed) {
        atomicAdd(&sh[GM_CLOSED], (unsigned long long)closed);
        atomicAdd(&sh[GM_Q32], ((unsigned long long)closed << 32) / pairs);
    }
}

// HyParView rows: 8 lanes a node, lane g takes neighbour g's row
__global__ void __launch_bounds__(BLK) k_gm_cluster_hv(Links ln, const uint8_t* __restrict__ flags, uint32_t n,
                                                       unsigned long long* gm) {
    static_assert(PSIM_ACTIVE_CAP == 8, "one 8-lane group per node");
    __shared__ unsigned long long sh[GM_N];
    if (threadIdx.x < GM_N) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / PSIM_ACTIVE_CAP, g = threadIdx.x % PSIM_ACTIVE_CAP;
    const bool up = i < n && (flags[i] & F_UP);
    const uint32_t k = up ? ln.cnt[i] : 0;
    uint32_t mine[PSIM_ACTIVE_CAP];
#pragma unroll
    for (uint32_t r = 0; r < PSIM_ACTIVE_CAP; r++) mine[r] = r < k ? ln.hv_row(i)[r] : PSIM_NONE;
    uint32_t c = 0;
    if (g < k && k >= 2) {
        const uint32_t a = ln.hv_row(i)[g];
        const uint32_t* row = ln.hv_row(a);
        for (uint32_t q = 0, ka = ln.cnt[a]; q < ka; q++) {
            const uint32_t b = row[q];
#pragma unroll
            for (uint32_t r = 0; r < PSIM_ACTIVE_CAP; r++) c += mine[r] == b ? 1u : 0u;
        }
    }
    for (int d = PSIM_ACTIVE_CAP / 2; d; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
    if (up && g == 0) gm_cluster_add(sh, k, c);
    __syncthreads();
    if (threadIdx.x < GM_N && sh[threadIdx.x]) atomicAdd(&gm[threadIdx.x], sh[threadIdx.x]);
}

DEV uint32_t gm_hash(uint32_t id) { return (id * 2654435761u) >> 24; }     // (GM_TAB = 2^8 slots)

// CSR rows (up to PSIM_SVIEW_CAP ids): a wave a node.  N(i) sits in the
// wave's LDS hash table (at most half full); each neighbour's row is read
// coalesced, two ids a lane as sh_row_load holds a view, and probed against it
__global__ void __launch_bounds__(BLK) k_gm_cluster(Links ln, const uint8_t* __restrict__ flags, uint32_t n,
                                                    unsigned long long* gm) {
    static_assert(GM_TAB == 256 && GM_TAB >= 2 * PSIM_SVIEW_CAP, "gm_hash gives 8 bits; the table stays half empty");
    __shared__ uint32_t tab_all[BLK / 64][GM_TAB];
    __shared__ unsigned long long sh[GM_N];
    const uint32_t w = threadIdx.x >> 6, l = lane_id();
    uint32_t* tab = tab_all[w];
    for (uint32_t q = l; q < GM_TAB; q += 64) tab[q] = PSIM_NONE;
    if (threadIdx.x < GM_N) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * (BLK / 64) + w;                          // (uniform per wave)
    const bool up = i < n && (flags[i] & F_UP);
    const uint32_t k = up ? min((uint32_t)ln.cnt[i], (uint32_t)PSIM_SVIEW_CAP) : 0;
    uint32_t a = PSIM_NONE, b = PSIM_NONE;
    if (k >= 2) {
        sh_row_load(ln.csr_row(i), k, a, b);
        for (int half = 0; half < 2; half++) {
            const uint32_t id = half ? b : a;
            if (id == PSIM_NONE) continue;
            uint32_t s = gm_hash(id);
            for (uint32_t t = 0; t < GM_TAB; t++, s = (s + 1) % GM_TAB)      // (ends at a free slot: <= 128 ids)
                if (atomicCAS(&tab[s], PSIM_NONE, id) == PSIM_NONE) break;
        }
    }
    __syncthreads();
    uint32_t c = 0;
    if (k >= 2) {
        for (uint32_t t = 0; t < k; t++) {                                   // (uniform)
            const uint32_t p = t < 64 ? shfl(a, (int)t) : shfl(b, (int)(t - 64));
            uint32_t x, y;
            sh_row_load(ln.csr_row(p), min((uint32_t)ln.cnt[p], (uint32_t)PSIM_SVIEW_CAP), x, y);
            for (int half = 0; half < 2; half++) {
                const uint32_t id = half ? y : x;
                if (id == PSIM_NONE) continue;
                uint32_t s = gm_hash(id);
                for (uint32_t u = 0; u < GM_TAB; u++, s = (s + 1) % GM_TAB) {
                    const uint32_t v = tab[s];
                    if (v == id) c++;
                    if (v == id || v == PSIM_NONE) break;
                }
            }
        }
        c = sh_wave_sum(c);
    }
    if (up && l == 0) gm_cluster_add(sh, k, c);
    __syncthreads();
    if (threadIdx.x < GM_N && sh[threadIdx.x]) atomicAdd(&gm[threadIdx.x], sh[threadIdx.x]);
}

// source slot j starts at sources[j] if that node is live; live: the mask of
// such slots (one block of 64 threads; the sources are distinct and < n)
__global__ void k_gm_init(const uint32_t* __restrict__ sources, uint32_t ns, const uint8_t* __restrict__ flags,
                          unsigned long long* seen, unsigned long long* front, unsigned long long* live) {
    const uint32_t j = threadIdx.x;
    const bool on = j < ns && (flags[sources[j]] & F_UP);
    if (on) { seen[sources[j]] = 1ull << j; front[sources[j]] = 1ull << j; }
    const uint64_t m = ballot(on);
    if (j == 0) *live = m;
}

// a node on the frontier ORs its word into each out-neighbour that lacks a bit of it
__global__ void k_gm_push(Links ln, uint32_t n, const unsigned long long* __restrict__ front,
                          const unsigned long long* __restrict__ seen, unsigned long long* next) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long f = front[i];
    if (!f) return;
    const uint32_t* row = ln.row(i);
    for (uint32_t k = 0, c = ln.cnt[i]; k < c; k++) {
        const uint32_t p = row[k];
        if (f & ~seen[p]) atomicOr(&next[p], f);
    }
}

// the level's new bits: into seen, the next frontier, lv[0] (their OR over
// all nodes), lv[1] (their number) and reach[j] per slot; reduced in the wave,
// then in the block's LDS, and only where a wave saw a new bit
__global__ void __launch_bounds__(BLK) k_gm_level(uint32_t n, unsigned long long* next, unsigned long long* seen,
                                                  unsigned long long* front, unsigned long long* lv,
                                                  unsigned long long* reach) {
    __shared__ unsigned long long sh_reach[PSIM_GRAPH_SOURCES], sh_lv[2];
    if (threadIdx.x < PSIM_GRAPH_SOURCES) sh_reach[threadIdx.x] = 0;
    if (threadIdx.x < 2) sh_lv[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nw = 0;
    if (i < n) {
        const unsigned long long nx = next[i];
        if (nx) {
            const unsigned long long s = seen[i];
            nw = nx & ~s;
            next[i] = 0;
            if (nw) seen[i] = s | nw;
        }
        if (front[i] != nw) front[i] = nw;
    }
    if (ballot(nw != 0)) {                            // (uniform)
        const uint64_t todo = wave_or(nw);
        const uint32_t cnt = sh_wave_sum(popc(nw));
        if (lane_id() == 0) { atomicOr(&sh_lv[0], (unsigned long long)todo); atomicAdd(&sh_lv[1], (unsigned long long)cnt); }
        tile_add(sh_reach, nw, todo);
    }
    __syncthreads();
    if (!sh_lv[0]) return;                            // (uniform per block)
    if (threadIdx.x < PSIM_GRAPH_SOURCES && sh_reach[threadIdx.x]) atomicAdd(&reach[threadIdx.x], sh_reach[threadIdx.x]);
    if (threadIdx.x == 0) { atomicOr(&lv[0], sh_lv[0]); atomicAdd(&lv[1], sh_lv[1]); }
}

// ------------------------------------------- reach under mass failure --
// psim_get_resilience (psim_resilience in the header defines every field):
// the word of the k_gm_* BFS spent on 64 failure cases, bit j of alive[v] =
// "v is in A_j".  The rows are those k_gm_push reads.
//   k_rs_live     the mask of cases whose source is up
//   k_rs_alive    alive[v], and the BFS seeded from it: seen[v] = ~alive[v]
//                 plus the bits of the cases that start at v, front[v] = those
//                 bits; a failed or down bit is never new to k_gm_level
//   k_rs_census   over every link (i, p): m = alive[i] & alive[p] counted per
//                 bit into links_alive, ORed into inw[p]; no_out from the
//                 bits of alive[i] that no link kept
//   k_rs_sweep    alive[] and no_in per bit
// The case table `par`: RS_SRC, RS_THR and RS_SALT by the host's order (cases
// of one salt side by side, so a node pays one inner mix64 per distinct salt),
// RS_SLOT the slot of each.
enum { RS_SRC = 0, RS_THR = 64, RS_SALT = 128, RS_SLOT = 192, RS_PAR = 256 };
enum { RS_ALIVE = 0, RS_LINKS = 64, RS_NOOUT = 128, RS_NOIN = 192, RS_NUP = 256, RS_L = 257, RS_LIVE = 258, RS_N = 259 };

__global__ void k_rs_live(const uint32_t* __restrict__ par, uint32_t nc, const uint8_t* __restrict__ flags,
                          unsigned long long* rs) {
    const uint32_t q = threadIdx.x;                   // (one block of 64 threads; the sources are < n)
    const bool on = q < nc && (flags[par[RS_SRC + q]] & F_UP);
    if (on) atomicOr(&rs[RS_LIVE], 1ull << par[RS_SLOT + q]);
}

__global__ void __launch_bounds__(BLK) k_rs_alive(const uint32_t* __restrict__ par, uint32_t nc, uint64_t fail_seed,
                                                  const uint8_t* __restrict__ flags, uint32_t n,
                                                  unsigned long long* rs, unsigned long long* alive,
                                                  unsigned long long* seen, unsigned long long* front) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool up = v < n && (flags[v] & F_UP);
    const unsigned long long live = rs[RS_LIVE];      // (k_rs_live ran before on the stream)
    unsigned long long a = 0, sb = 0;
    if (up) {
        uint64_t inner = 0;
        for (uint32_t q = 0; q < nc; q++) {           // (uniform)
            const uint32_t salt = par[RS_SALT + q];
            if (!q || salt != par[RS_SALT + q - 1]) inner = mix64(((uint64_t)salt << 32) | v);
            const uint32_t u = (uint32_t)(mix64(fail_seed ^ inner) >> 32);
            const unsigned long long bit = 1ull << par[RS_SLOT + q];
            const bool src = par[RS_SRC + q] == v;
            if (src || u >= par[RS_THR + q]) a |= bit;
            if (src) sb |= bit;
        }
        a &= live; sb &= live;
    }
    if (v < n) { alive[v] = a; seen[v] = ~a | sb; front[v] = sb; }
    const uint32_t c = popc(ballot(up));
    if (c && lane_id() == 0) atomicAdd(&rs[RS_NUP], (unsigned long long)c);
}

__global__ void __launch_bounds__(BLK) k_rs_census(Links ln, const uint8_t* __restrict__ flags, uint32_t n,
                                                   const unsigned long long* __restrict__ alive,
                                                   unsigned long long* inw, unsigned long long* rs) {
    static_assert(PSIM_SVIEW_CAP < 256 && PSIM_ACTIVE_CAP < 256, "a row's links per case fit the 8 counter planes");
    __shared__ unsigned long long sh_links[PSIM_FAIL_CASES], sh_noout[PSIM_FAIL_CASES], sh_l;
    if (threadIdx.x < PSIM_FAIL_CASES) { sh_links[threadIdx.x] = 0; sh_noout[threadIdx.x] = 0; }
    if (threadIdx.x == 0) sh_l = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool up = i < n && (flags[i] & F_UP);
    const uint32_t c = up ? ln.cnt[i] : 0;
    const unsigned long long a = up ? alive[i] : 0;
    // plane b holds bit b of this node's link count of every case
    unsigned long long pl[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ho = 0;
    if (a) {
        const uint32_t* row = ln.row(i);
        for (uint32_t k = 0; k < c; k++) {
            const uint32_t p = row[k];
            const unsigned long long m = a & alive[p];
            if (!m) continue;
            ho |= m;
            if (m & ~inw[p]) atomicOr(&inw[p], m);
            plane_inc(pl, m);
        }
    }
    const uint32_t lsum = sh_wave_sum(c);
    if (lsum && lane_id() == 0) atomicAdd(&sh_l, (unsigned long long)lsum);
    if (ballot(a != 0)) {                             // (uniform)
        tile_add(sh_noout, a & ~ho);
        tile_add_planes(sh_links, pl, wave_or(ho));
    }
    __syncthreads();
    if (threadIdx.x < PSIM_FAIL_CASES) {
        if (sh_links[threadIdx.x]) atomicAdd(&rs[RS_LINKS + threadIdx.x], sh_links[threadIdx.x]);
        if (sh_noout[threadIdx.x]) atomicAdd(&rs[RS_NOOUT + threadIdx.x], sh_noout[threadIdx.x]);
    }
    if (threadIdx.x == 0 && sh_l) atomicAdd(&rs[RS_L], sh_l);
}

__global__ void __launch_bounds__(BLK) k_rs_sweep(uint32_t n, const unsigned long long* __restrict__ alive,
                                                  const unsigned long long* __restrict__ inw,
                                                  unsigned long long* rs) {
    __shared__ unsigned long long sh_alive[PSIM_FAIL_CASES], sh_noin[PSIM_FAIL_CASES];
    if (threadIdx.x < PSIM_FAIL_CASES) { sh_alive[threadIdx.x] = 0; sh_noin[threadIdx.x] = 0; }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long a = i < n ? alive[i] : 0;
    if (ballot(a != 0)) {                             // (uniform)
        tile_add(sh_alive, a);
        tile_add(sh_noin, a & ~inw[i < n ? i : 0]);
    }
    __syncthreads();
    if (threadIdx.x < PSIM_FAIL_CASES) {
        if (sh_alive[threadIdx.x]) atomicAdd(&rs[RS_ALIVE + threadIdx.x], sh_alive[threadIdx.x]);
        if (sh_noin[threadIdx.x]) atomicAdd(&rs[RS_NOIN + threadIdx.x], sh_noin[threadIdx.x]);
    }
}

// ------------------------------------------------- gossip with a fanout --
// psim_get_gossip_reach (psim_gossip_reach in the header defines every field):
// k_rs_alive's survivor words and the k_gm_level BFS, with one more word per
// link slot: bit j of sel[e] = "link e = (i, p) is in S_j(i)", e the slot of
// the link in Links.adj.
//   k_go_select      rows of at most GO_SHORT links: a thread a node, the
//                    row's ids, keys and ranks in registers
//   k_go_select_long the longer rows of a CSR: GO_LN lanes a node, entry
//                    c * GO_LN + g in slot c of the group's lane g; an entry's
//                    rank = the entries of the row before it in (w, id) order,
//                    counted by broadcasting every entry across the group
//                    both walk the case table in k_rs_alive's order: h, the
//                    keys and the ranks once per distinct salt, a case is one
//                    compare of the rank against its fanout; a row no longer
//                    than the smallest fanout above 0 (fmin) is chosen whole
//                    in every case and pays none of it
//   k_go_push        k_gm_push over the chosen links: m = front[i] & sel[e]
//   k_go_tally       after the loop: the senders word of i is seen[i] &
//                    alive[i] & ~front[i] (front: only a truncated last level);
//                    over i's links m = that word & sel[e] counted per bit into
//                    sent, m & ~alive[p] into lost; alive[] per bit; |L|
// The case table `par`: k_rs_alive's, then GO_FAN, the fanouts in its order.
enum { GO_FAN = RS_PAR, GO_PAR = RS_PAR + 64 };
enum { GO_ALIVE = 0, GO_SENT = 64, GO_LOST = 128, GO_L = 192, GO_N = 193 };
constexpr uint64_t GO_GOLDEN = 0x9E3779B97F4A7C15ull;
// Row lengths (DESIGN.md "Gossip with a fanout"): every HyParView row and
// 99.3 % of SCAMP v2's (c = 5, 2^24 nodes: 69 % hold one link, the longest 54)
// have at most 8 links -- a thread; of the rest most have at most 16, and a
// v1 row can pass 100 -- 16 lanes, up to 8 entries each
constexpr uint32_t GO_SHORT = 8, GO_LN = 16, GO_C = PSIM_SVIEW_CAP / GO_LN;

// entry (ka, pa) comes before entry (kb, pb) in the order S_j(i) is cut from
DEV bool go_before(uint64_t ka, uint32_t pa, uint64_t kb, uint32_t pb) { return ka < kb || (ka == kb && pa < pb); }
DEV uint64_t go_h(uint64_t fail_seed, uint32_t salt, uint32_t i) { return mix64(fail_seed ^ mix64(((uint64_t)salt << 32) | i)); }
DEV uint64_t go_key(uint64_t h, uint32_t p) { return mix64(h + GO_GOLDEN * ((uint64_t)p + 1)); }

// all: the bits of every case; fmin: the smallest fanout above 0 (none: PSIM_NONE)
__global__ void __launch_bounds__(BLK) k_go_select(Links ln, uint32_t n, const uint32_t* __restrict__ par,
                                                   uint32_t nc, uint64_t fail_seed, unsigned long long all,
                                                   uint32_t fmin, unsigned long long* sel) {
    static_assert(PSIM_ACTIVE_CAP <= GO_SHORT, "every HyParView row is a short one");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = i < n ? ln.cnt[i] : 0;
    if (!c || c > GO_SHORT) return;                   // (the longer rows: k_go_select_long's)
    const size_t at = ln.slot(i);
    if (c <= fmin) {
        for (uint32_t r = 0; r < c; r++) sel[at + r] = all;
        return;
    }
    // (entries past c: the last of every order, and never stored)
    uint32_t p[GO_SHORT], rank[GO_SHORT];
    uint64_t key[GO_SHORT];
    unsigned long long w[GO_SHORT];
#pragma unroll
    for (uint32_t r = 0; r < GO_SHORT; r++) { p[r] = r < c ? ln.adj[at + r] : PSIM_NONE; rank[r] = 0; key[r] = 0; w[r] = 0; }
    for (uint32_t q = 0; q < nc; q++) {               // (uniform)
        const uint32_t salt = par[RS_SALT + q];
        if (!q || salt != par[RS_SALT + q - 1]) {
            const uint64_t h = go_h(fail_seed, salt, i);
#pragma unroll
            for (uint32_t r = 0; r < GO_SHORT; r++) key[r] = r < c ? go_key(h, p[r]) : ~0ull;
#pragma unroll
            for (uint32_t r = 0; r < GO_SHORT; r++) rank[r] = 0;
            // (a pair once: one of two entries comes first, a row's ids are distinct)
#pragma unroll
            for (uint32_t r = 0; r < GO_SHORT; r++)
#pragma unroll
                for (uint32_t t = r + 1; t < GO_SHORT; t++) {
                    const uint32_t tf = go_before(key[t], p[t], key[r], p[r]) ? 1u : 0u;
                    rank[r] += tf; rank[t] += 1u - tf;
                }
        }
        const uint32_t f = par[GO_FAN + q];
        const unsigned long long bit = 1ull << par[RS_SLOT + q];
#pragma unroll
        for (uint32_t r = 0; r < GO_SHORT; r++)
            if (!f || rank[r] < f) w[r] |= bit;
    }
#pragma unroll
    for (uint32_t r = 0; r < GO_SHORT; r++)
        if (r < c) sel[at + r] = w[r];
}

// (the loop bounds are the same in all lanes of a group, and a lane reads its
// own group only, as in tm_match)
__global__ void __launch_bounds__(BLK) k_go_select_long(Links ln, uint32_t n, const uint32_t* __restrict__ par,
                                                        uint32_t nc, uint64_t fail_seed, unsigned long long all,
                                                        uint32_t fmin, unsigned long long* sel) {
    static_assert(GO_LN * GO_C == PSIM_SVIEW_CAP && 64 % GO_LN == 0, "a group holds a whole row and sits in one wave");
    const uint32_t i = (uint32_t)(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / GO_LN);
    const uint32_t l = lane_id(), g = l % GO_LN, gb = l - g;
    const uint32_t c = i < n ? min((uint32_t)ln.cnt[i], (uint32_t)PSIM_SVIEW_CAP) : 0;
    if (c <= GO_SHORT) return;                        // (k_go_select's)
    const uint32_t nch = (c + GO_LN - 1) / GO_LN;     // slots in use
    const size_t at = ln.off[i];
    if (c <= fmin) {
        for (uint32_t e = g; e < c; e += GO_LN) sel[at + e] = all;
        return;
    }
    uint32_t p[GO_C], rank[GO_C];
    uint64_t key[GO_C];
    unsigned long long w[GO_C];
#pragma unroll
    for (uint32_t s = 0; s < GO_C; s++) { p[s] = s * GO_LN + g < c ? ln.adj[at + s * GO_LN + g] : PSIM_NONE; rank[s] = 0; key[s] = 0; w[s] = 0; }
    for (uint32_t q = 0; q < nc; q++) {               // (uniform)
        const uint32_t salt = par[RS_SALT + q];
        if (!q || salt != par[RS_SALT + q - 1]) {
            const uint64_t h = go_h(fail_seed, salt, i);
#pragma unroll
            for (uint32_t s = 0; s < GO_C; s++) {
                if (s < nch) key[s] = s * GO_LN + g < c ? go_key(h, p[s]) : ~0ull;
                rank[s] = 0;
            }
#pragma unroll
            for (uint32_t s2 = 0; s2 < GO_C; s2++)
                for (uint32_t y = 0; y < GO_LN && s2 * GO_LN + y < c; y++) {
                    const uint64_t kv = shfl64(key[s2], (int)(gb + y));
                    const uint32_t pv = shfl(p[s2], (int)(gb + y));
#pragma unroll
                    for (uint32_t s = 0; s < GO_C; s++)
                        if (s < nch) rank[s] += go_before(kv, pv, key[s], p[s]) ? 1u : 0u;
                }
        }
        const uint32_t f = par[GO_FAN + q];
        const unsigned long long bit = 1ull << par[RS_SLOT + q];
#pragma unroll
        for (uint32_t s = 0; s < GO_C; s++)
            if (!f || rank[s] < f) w[s] |= bit;
    }
#pragma unroll
    for (uint32_t s = 0; s < GO_C; s++)
        if (s * GO_LN + g < c) sel[at + s * GO_LN + g] = w[s];
}

// a node on the frontier ORs the bits that chose a link into its target if that lacks one of them
__global__ void k_go_push(Links ln, const unsigned long long* __restrict__ sel, uint32_t n,
                          const unsigned long long* __restrict__ front, const unsigned long long* __restrict__ seen,
                          unsigned long long* next) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long f = front[i];
    if (!f) return;
    const size_t at = ln.slot(i);
    for (uint32_t k = 0, c = ln.cnt[i]; k < c; k++) {
        const unsigned long long m = f & sel[at + k];
        if (!m) continue;
        const uint32_t p = ln.adj[at + k];
        if (m & ~seen[p]) atomicOr(&next[p], m);
    }
}

// (a node that is down holds no links and no alive bit)
__global__ void __launch_bounds__(BLK) k_go_tally(Links ln, const unsigned long long* __restrict__ sel, uint32_t n,
                                                  const unsigned long long* __restrict__ alive,
                                                  const unsigned long long* __restrict__ seen,
                                                  const unsigned long long* __restrict__ front,
                                                  unsigned long long* go) {
    static_assert(PSIM_SVIEW_CAP < 256 && PSIM_ACTIVE_CAP < 256, "a row's copies per case fit the 8 counter planes");
    __shared__ unsigned long long sh_alive[PSIM_FAIL_CASES], sh_sent[PSIM_FAIL_CASES], sh_lost[PSIM_FAIL_CASES], sh_l;
    if (threadIdx.x < PSIM_FAIL_CASES) { sh_alive[threadIdx.x] = 0; sh_sent[threadIdx.x] = 0; sh_lost[threadIdx.x] = 0; }
    if (threadIdx.x == 0) sh_l = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = i < n ? ln.cnt[i] : 0;
    const unsigned long long a = i < n ? alive[i] : 0;
    const unsigned long long sw = a ? a & seen[i] & ~front[i] : 0;
    unsigned long long ps[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pl[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hs = 0, hl = 0;
    if (sw) {
        const size_t at = ln.slot(i);
        for (uint32_t k = 0; k < c; k++) {
            const unsigned long long m = sw & sel[at + k];
            if (!m) continue;
            hs |= m;
            plane_inc(ps, m);
            const unsigned long long ml = m & ~alive[ln.adj[at + k]];
            if (!ml) continue;
            hl |= ml;
            plane_inc(pl, ml);
        }
    }
    const uint32_t lsum = sh_wave_sum(c);
    if (lsum && lane_id() == 0) atomicAdd(&sh_l, (unsigned long long)lsum);
    if (ballot(a != 0)) {                             // (uniform)
        tile_add(sh_alive, a);
        tile_add_planes(sh_sent, ps, wave_or(hs));
        tile_add_planes(sh_lost, pl, wave_or(hl));
    }
    __syncthreads();
    if (threadIdx.x < PSIM_FAIL_CASES) {
        if (sh_alive[threadIdx.x]) atomicAdd(&go[GO_ALIVE + threadIdx.x], sh_alive[threadIdx.x]);
        if (sh_sent[threadIdx.x]) atomicAdd(&go[GO_SENT + threadIdx.x], sh_sent[threadIdx.x]);
        if (sh_lost[threadIdx.x]) atomicAdd(&go[GO_LOST + threadIdx.x], sh_lost[threadIdx.x]);
    }
    if (threadIdx.x == 0 && sh_l) atomicAdd(&go[GO_L], sh_l);
}

// ------------------------------------------------------ broadcast tree --
// psim_get_tree_metrics: root R's eager / lazy sets of every live node
// (psim_tree_metrics in the header defines every field).
//   k_tm_rows (count)  LN lanes a node; finds R's slot in the root row, holds
//                      the eager and the lazy run RT_SET / LN entries a lane,
//                      decodes, drops self, tests liveness, marks the first
//                      occurrence of a peer over both identity forms by a
//                      compare against every lane of the group, tests the
//                      active view, counts the entry-level fields and writes
//                      |E_i| (a byte, by global id)
//   scan_excl          the counts (all-gathered across ranks) -> row offsets
//   k_tm_rows (pack)   the same group writes E_i at its offset and adds the
//                      in-degrees
//   k_tm_sym           (i, p) in T: is i in p's row?
//   k_tm_bfs           one level of a single-source BFS over CSR or
//                      HyParView rows, depths in an N-word array
//   k_tm_final         the in-degree histogram and the two depth arrays
// tm layout (summed over ranks): two histograms, then scalars
enum { TM_EOUT = 0, TM_LOUT = 1, TM_NUP = 2 * PSIM_HIST_BINS, TM_SLOT, TM_EENT, TM_LENT, TM_ELINKS, TM_LLINKS,
       TM_BOTH, TM_FORMS, TM_SELF, TM_EDEAD, TM_LDEAD, TM_ENM, TM_LNM, TM_N };
constexpr uint32_t TM_SCALARS = TM_N - TM_NUP;
// tf layout (over the whole CSR, the same on every rank): the in-degree histogram, then scalars
enum { TF_LFR = PSIM_HIST_BINS, TF_OREACH, TF_BOTH, TF_DSUM, TF_LSUM, TF_DEEPER, TF_SHALLOWER, TF_N };

// a run of at most RT_SET entries held by a group of LN lanes: entry
// c * LN + g in e[c] of the group's lane g
template <uint32_t LN>
struct TmRun {
    static constexpr uint32_t C = RT_SET / LN;
    uint32_t e[C], p[C];
    bool keep[C];                         // the entry names a live node other than the owner
    uint32_t n;
};

// loads the run; counts the lane's entries that name the owner / a dead node
template <uint32_t LN>
DEV void tm_load(TmRun<LN>& r, const uint32_t* __restrict__ src, uint32_t n, uint32_t me,
                 const uint8_t* __restrict__ flags, uint32_t N, uint32_t& self, uint32_t& dead) {
    const uint32_t g = lane_id() % LN;
    r.n = n;
#pragma unroll
    for (uint32_t c = 0; c < TmRun<LN>::C; c++) {
        const bool v = c * LN + g < n;
        r.e[c] = v ? src[c * LN + g] : PSIM_NONE;
        r.p[c] = r.e[c] & ~PSIM_MAP_BIT;
        const bool own = v && r.p[c] == me, live = v && sh_live(flags, N, r.p[c]);
        r.keep[c] = live && !own;
        self += own ? 1u : 0u;
        dead += v && !own && !live ? 1u : 0u;
    }
}

// every entry of run b, in order, against the lane's entries of run a:
// dup[c]: an entry of b before position c * LN + g names the same node (a == b:
// the entry is no first occurrence); hit[c]: some entry of b names it;
// atom[c] / map[c]: b holds the node's plain / PSIM_MAP_BIT form.  The loop
// bounds are the same in all lanes of a group, and a lane reads its own group only
template <uint32_t LN>
DEV void tm_match(const TmRun<LN>& a, const TmRun<LN>& b, bool* dup, bool* hit, bool* atom, bool* map) {
    constexpr uint32_t C = TmRun<LN>::C;
    const uint32_t l = lane_id(), g = l % LN, gb = l - g;
#pragma unroll
    for (uint32_t c = 0; c < C; c++) dup[c] = hit[c] = atom[c] = map[c] = false;
#pragma unroll
    for (uint32_t c2 = 0; c2 < C; c2++)
        for (uint32_t y = 0; y < LN && c2 * LN + y < b.n; y++) {
            const uint32_t ev = shfl(b.e[c2], (int)(gb + y)), pv = ev & ~PSIM_MAP_BIT;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                const bool same = pv == a.p[c];
                dup[c] |= same && c2 * LN + y < c * LN + g;
                hit[c] |= same;
                atom[c] |= ev == a.p[c];
                map[c] |= ev == (a.p[c] | PSIM_MAP_BIT);
            }
        }
}

// off == nullptr: the count pass (statistics into tm, |E_i| into
// cnt[lo + i]); else the pack pass (E_i into adj at off[lo + i], indeg)
template <uint32_t LN>
__global__ void __launch_bounds__(BLK) k_tm_rows(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ act,
                                                 const uint32_t* __restrict__ pt_rt,
                                                 const uint32_t* __restrict__ pt_eag,
                                                 const uint32_t* __restrict__ pt_laz,
                                                 const uint32_t* __restrict__ pt_com,
                                                 const uint8_t* __restrict__ flags, uint32_t lo, uint32_t n,
                                                 uint32_t N, uint32_t root, uint8_t* cnt,
                                                 const uint32_t* __restrict__ off, uint32_t* adj, uint32_t* indeg,
                                                 unsigned long long* tm) {
    static_assert(LN == 16 || LN == 64, "a DPP row or a wave a node");
    static_assert(PSIM_PT_ROOTS == 4 && RT_SET == 64, "the counts of a pool: one byte a slot, 64 entries");
    constexpr uint32_t C = TmRun<LN>::C;
    constexpr uint64_t GROUP = LN == 64 ? ~0ull : (1ull << (LN % 64)) - 1ull;     // a group's lanes of a ballot
    __shared__ unsigned long long sh[TM_N];
    for (uint32_t j = threadIdx.x; j < TM_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t l = lane_id(), g = l % LN, gb = l - g;
    const uint32_t i = (blockIdx.x * BLK + threadIdx.x) / LN, me = lo + i;
    const bool up = i < n && (flags[me] & F_UP);
    uint32_t s[TM_SCALARS] = {0};                     // the lane's share of the scalars
    if (up) {                                         // (the same in all lanes of a group)
        // R's slot, or the common set
        const uint32_t* rt = pt_rt + (size_t)i * RT_WORDS;
        int k = -1;
        for (int q = PSIM_PT_ROOTS - 1; q >= 0; q--) k = rt[q] == (root | PSIM_MAP_BIT) ? q : k;
        uint32_t en, ln = 0, eo = 0, zo = 0;
        if (k >= 0) {
            const uint32_t ce = rt[RT_EN], cl = rt[RT_LN];
            for (int q = 0; q < k; q++) { eo += (ce >> (8 * q)) & 0xFFu; zo += (cl >> (8 * q)) & 0xFFu; }
            eo = min(eo, RT_SET); zo = min(zo, RT_SET);
            en = min((ce >> (8 * k)) & 0xFFu, RT_SET - eo);
            ln = min((cl >> (8 * k)) & 0xFFu, RT_SET - zo);
        } else {
            en = min((uint32_t)hdr[i].com_n, (uint32_t)PSIM_PT_MEMBERS_CAP);
        }
        const uint32_t* er = k >= 0 ? pt_eag + (size_t)i * RT_SET + eo : pt_com + (size_t)i * PSIM_PT_MEMBERS_CAP;
        TmRun<LN> E;
        bool dup[C], hit[C], atom[C], map[C];
        tm_load(E, er, en, me, flags, N, s[TM_SELF - TM_NUP], s[TM_EDEAD - TM_NUP]);
        tm_match(E, E, dup, hit, atom, map);
        // E_i: the first occurrences among the kept entries, packed in entry order
        uint32_t ne = 0;
        bool first[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            first[c] = E.keep[c] && !dup[c];
            const uint64_t b = (ballot(first[c]) >> gb) & GROUP;
            if (off && first[c]) {
                adj[off[me] + ne + popc(b & ((1ull << g) - 1ull))] = E.p[c];
                atomicAdd(&indeg[E.p[c]], 1u);
            }
            ne += popc(b);
        }
        if (!off) {
            const uint32_t an = min((uint32_t)hdr[i].act_n, (uint32_t)PSIM_ACTIVE_CAP);
            uint32_t av[PSIM_ACTIVE_CAP];
#pragma unroll
            for (uint32_t q = 0; q < PSIM_ACTIVE_CAP; q++) av[q] = q < an ? act[(size_t)i * PSIM_ACTIVE_CAP + q] : PSIM_NONE;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                if (!first[c]) continue;
                bool mem = false;
#pragma unroll
                for (uint32_t q = 0; q < PSIM_ACTIVE_CAP; q++) mem |= av[q] == E.p[c];
                s[TM_ENM - TM_NUP] += mem ? 0u : 1u;
                s[TM_FORMS - TM_NUP] += atom[c] && map[c] ? 1u : 0u;
            }
            uint32_t nz = 0;
            if (ln) {                                 // (the same in all lanes of a group)
                TmRun<LN> Z;
                bool zdup[C], inE[C];
                tm_load(Z, pt_laz + (size_t)i * RT_SET + zo, ln, me, flags, N, s[TM_SELF - TM_NUP],
                        s[TM_LDEAD - TM_NUP]);
                tm_match(Z, Z, zdup, hit, atom, map);
                tm_match(Z, E, dup, inE, atom, map);
#pragma unroll
                for (uint32_t c = 0; c < C; c++) {
                    if (!Z.keep[c] || zdup[c]) continue;
                    bool mem = false;
#pragma unroll
                    for (uint32_t q = 0; q < PSIM_ACTIVE_CAP; q++) mem |= av[q] == Z.p[c];
                    nz++;
                    s[TM_LNM - TM_NUP] += mem ? 0u : 1u;
                    s[TM_BOTH - TM_NUP] += inE[c] ? 1u : 0u;
                }
                s[TM_LLINKS - TM_NUP] += nz;
                for (int d = LN / 2; d; d >>= 1) nz += (uint32_t)__shfl_xor((int)nz, d);
            }
            if (g == 0) {
                cnt[me] = (uint8_t)ne;
                s[TM_NUP - TM_NUP] = 1; s[TM_SLOT - TM_NUP] = k >= 0 ? 1u : 0u;
                s[TM_EENT - TM_NUP] = en; s[TM_LENT - TM_NUP] = ln; s[TM_ELINKS - TM_NUP] = ne;
                atomicAdd(&sh[TM_EOUT * PSIM_HIST_BINS + hbin(ne)], 1ull);
                atomicAdd(&sh[TM_LOUT * PSIM_HIST_BINS + hbin(nz)], 1ull);
            }
        }
    }
    if (off) return;
#pragma unroll
    for (uint32_t j = 0; j < TM_SCALARS; j++) {
        const uint32_t v = sh_wave_sum(s[j]);
        if (l == 0 && v) atomicAdd(&sh[TM_NUP + j], (unsigned long long)v);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < TM_N; j += blockDim.x)
        if (sh[j]) atomicAdd(&tm[j], sh[j]);
}

// the links of T whose reverse is a link of T (every process over the whole CSR)
__global__ void k_tm_sym(Links ln, uint32_t n, unsigned long long* sym) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (i < n) {
        const uint32_t* row = ln.csr_row(i);
        for (uint32_t k = 0, ci = ln.cnt[i]; k < ci; k++) c += sh_has(ln, row[k], i) ? 1u : 0u;
    }
    c = sh_wave_sum(c);
    if (lane_id() == 0 && c) atomicAdd(sym, (unsigned long long)c);
}

// level d of a single-source BFS (rows as k_gm_push reads them): a node at
// depth d - 1 claims each out-neighbour that has no depth yet; found: the
// nodes claimed
__global__ void k_tm_bfs(Links ln, uint32_t n, uint32_t d, uint32_t* depth, unsigned long long* found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (i < n && depth[i] == d - 1) {
        const uint32_t* row = ln.row(i);
        for (uint32_t k = 0, ci = ln.cnt[i]; k < ci; k++) {
            const uint32_t p = row[k];
            if (p < n && depth[p] == PSIM_NONE && atomicCAS(&depth[p], PSIM_NONE, d) == PSIM_NONE) c++;
        }
    }
    c = sh_wave_sum(c);
    if (lane_id() == 0 && c) atomicAdd(found, (unsigned long long)c);
}

// per live node: its in-degree in T; dt / dl (nullptr: R is not live): its
// depth over T and its distance over L (PSIM_NONE: none)
__global__ void __launch_bounds__(BLK) k_tm_final(const uint32_t* __restrict__ indeg,
                                                  const uint8_t* __restrict__ cnt,
                                                  const uint8_t* __restrict__ flags, uint32_t n, uint32_t root,
                                                  const uint32_t* __restrict__ dt,
                                                  const uint32_t* __restrict__ dl, unsigned long long* tf) {
    __shared__ unsigned long long sh[TF_N];
    for (uint32_t j = threadIdx.x; j < TF_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s[TF_N - TF_LFR] = {0};
    if (i < n && (flags[i] & F_UP)) {
        atomicAdd(&sh[hbin(indeg[i])], 1ull);
        const uint32_t a = dt ? dt[i] : PSIM_NONE, b = dl ? dl[i] : PSIM_NONE;
        if (a != PSIM_NONE) s[TF_LFR - TF_LFR] = cnt[i];
        if (i != root) {
            if (b != PSIM_NONE) s[TF_OREACH - TF_LFR] = 1;
            if (a != PSIM_NONE && b != PSIM_NONE) {
                s[TF_BOTH - TF_LFR] = 1; s[TF_DSUM - TF_LFR] = a; s[TF_LSUM - TF_LFR] = b;
                s[TF_DEEPER - TF_LFR] = a > b ? 1u : 0u; s[TF_SHALLOWER - TF_LFR] = a < b ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < TF_N - TF_LFR; j++) {
        const uint32_t v = sh_wave_sum(s[j]);         // (a wave's depths: 64 * 4096 at the most)
        if (lane_id() == 0 && v) atomicAdd(&sh[TF_LFR + j], (unsigned long long)v);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < TF_N; j += blockDim.x)
        if (sh[j]) atomicAdd(&tf[j], sh[j]);
}

// -------------------------------------------------- transitive unicast --
// psim_get_relay_reach (psim_relay_reach in the header defines every field):
// the relay_message flood counts walks, so its frontier is a sparse list of
// (case, ttl, node) -> count entries instead of a word per node.
//   k_rl_pack     virtual shards and ranks: a node's three rows and their
//                 lengths by global id (one shard reads its rows in place)
//   k_rl_census   16 lanes a node: the out entries in lanes 0-7, the active
//                 view in lanes 8-15, the connection table in both halves;
//                 every entry meets every other by a shuffle in its group
//   k_rl_expand   a level's entries: LN = 1, a lane an entry, the rows in
//                 registers, or LN = 8 lanes an entry, lane g out-link g and
//                 entry g of each row (PSIM_RELAY_LANES=8, for A/B: the
//                 slower of the two); per-case tallies into the
//                 block's LDS tile, the children at a block-wide offset
//   k_rl_merge    the children into an open-addressing table: the key claimed
//                 by a 64-bit atomicCAS, the count added by a 64-bit atomicAdd
//   k_rl_compact  the table's used slots -> the next level's entries, their
//                 number and count sum per case
// A key: case << 32 | ttl << 27 | node.  The case table `par`: RP_DST, RP_TTL.
enum { RC_NUP = 0, RC_ENT, RC_USE, RC_NONMEM, RC_DOWN, RC_DEG, RC_N = RC_DEG + PSIM_HIST_BINS };
enum { RF_DELIV = 0, RF_HOPS, RF_RELAY, RF_REFUSED, RF_EXPIRED, RF_RESTART, RF_FIRST, RF_FIELDS,
       RF_LIVE = RF_FIELDS * PSIM_RELAY_CASES, RF_DIRECT, RF_N };
enum { RP_DST = 0, RP_TTL = PSIM_RELAY_CASES, RP_N = 2 * PSIM_RELAY_CASES };
enum { RV_CHILD = 0, RV_NEXT, RV_DISTINCT, RV_SUM = RV_DISTINCT + PSIM_RELAY_CASES, RV_N = RV_SUM + PSIM_RELAY_CASES };
enum : uint32_t { RL_NONE = 0, RL_CONN = 1, RL_DOWN = 2 };
constexpr unsigned long long RL_EMPTY = ~0ull;
constexpr uint32_t RL_ROW = 8;
static_assert(PSIM_ACTIVE_CAP == RL_ROW && PSIM_PT_MEMBERS_CAP == RL_ROW && PSIM_CONN_CAP == RL_ROW,
              "three rows of 8 words: one 8-lane group holds each");
static_assert(PSIM_RELAY_MAX_TTL < 32 && KEY_DST_BITS == 27, "a key: 6 bits of case, 5 of ttl, 27 of node");

struct RlRows {
    const Hdr* hdr;            // one shard: the lengths in place; else nullptr and cnt
    const uint32_t* cnt;       // act_n | com_n << 8 | conn_n << 16 by global id
    const uint32_t *act, *com, *conn;
    // the three lengths, each at most RL_ROW
    DEV void counts(uint32_t i, uint32_t& an, uint32_t& en, uint32_t& kn) const {
        if (hdr) { an = hdr[i].act_n; en = hdr[i].com_n; kn = hdr[i].conn_n; }
        else { const uint32_t c = cnt[i]; an = c & 0xFFu; en = (c >> 8) & 0xFFu; kn = (c >> 16) & 0xFFu; }
        an = min(an, RL_ROW); en = min(en, RL_ROW); kn = min(kn, RL_ROW);
    }
};

DEV unsigned long long rl_key(uint32_t j, uint32_t ttl, uint32_t node) {
    return ((unsigned long long)j << 32) | ((unsigned long long)ttl << KEY_DST_BITS) | node;
}
// state(i, p) of a live p != i from what the rows of i hold
DEV uint32_t rl_state(bool live, bool in_act, bool down, bool plain) {
    return !live ? RL_NONE : down ? (in_act ? RL_DOWN : RL_NONE) : (plain || in_act ? RL_CONN : RL_NONE);
}
DEV bool rl_live(const uint8_t* __restrict__ flags, uint32_t N, uint32_t i, uint32_t p) {
    return p != i && p < N && (flags[p] & F_UP);
}

__global__ void k_rl_pack(const Hdr* __restrict__ hdr, const uint32_t* __restrict__ act,
                          const uint32_t* __restrict__ com, const uint32_t* __restrict__ conn, uint32_t n,
                          uint32_t* gact, uint32_t* gcom, uint32_t* gconn, uint32_t* gcnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gcnt[i] = (uint32_t)hdr[i].act_n | (uint32_t)hdr[i].com_n << 8 | (uint32_t)hdr[i].conn_n << 16;
    for (uint32_t q = 0; q < RL_ROW; q++) {
        gact[(size_t)i * RL_ROW + q] = act[(size_t)i * RL_ROW + q];
        gcom[(size_t)i * RL_ROW + q] = com[(size_t)i * RL_ROW + q];
        gconn[(size_t)i * RL_ROW + q] = conn[(size_t)i * RL_ROW + q];
    }
}

// (over the whole overlay's rows, the same on every rank: nothing to reduce)
__global__ void __launch_bounds__(BLK) k_rl_census(RlRows R, const uint8_t* __restrict__ flags, uint32_t N,
                                                   unsigned long long* cs) {
    constexpr uint32_t LN = 16;
    __shared__ unsigned long long sh[RC_N];
    for (uint32_t j = threadIdx.x; j < RC_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t l = lane_id(), g = l % LN, gb = l - g, q8 = g % RL_ROW;
    const uint32_t i = (blockIdx.x * BLK + threadIdx.x) / LN;
    const bool up = i < N && (flags[i] & F_UP), is_out = g < RL_ROW;
    uint32_t x = PSIM_NONE, cn = PSIM_NONE;            // the lane's out or active entry; its connection entry
    bool valid = false;
    if (up) {
        uint32_t an, en, kn;
        R.counts(i, an, en, kn);
        valid = q8 < (is_out ? en : an);
        if (valid) x = (is_out ? R.com : R.act)[(size_t)i * RL_ROW + q8];
        if (q8 < kn) cn = R.conn[(size_t)i * RL_ROW + q8];
    }
    const uint32_t p = is_out ? x & ~PSIM_MAP_BIT : x;
    bool in_act = false, dn = false, pl = false, dup = false;
#pragma unroll
    for (uint32_t q = 0; q < RL_ROW; q++) {            // (every lane of the wave: no branch around a shuffle)
        const uint32_t aq = shfl(x, (int)(gb + RL_ROW + q)), cq = shfl(cn, (int)(gb + q));
        in_act |= aq == p; dn |= cq == (p | PSIM_CONN_DOWN); pl |= cq == p;
        dup |= q < q8 && aq == p;                      // (read by the active lanes only)
    }
    const uint32_t st = rl_state(valid && rl_live(flags, N, i, p), in_act, dn, pl);
    const bool ent = valid && is_out && x != i;
    const uint64_t b_ent = ballot(ent), b_use = ballot(ent && st == RL_CONN), b_non = ballot(ent && !in_act);
    const uint64_t b_dn = ballot(valid && !is_out && !dup && st == RL_DOWN), b_up = ballot(up && g == 0);
    if (up && g == 0) atomicAdd(&sh[RC_DEG + hbin(popc((b_use >> gb) & 0xFFFFull))], 1ull);
    if (l == 0) {
        if (b_up) atomicAdd(&sh[RC_NUP], (unsigned long long)popc(b_up));
        if (b_ent) atomicAdd(&sh[RC_ENT], (unsigned long long)popc(b_ent));
        if (b_use) atomicAdd(&sh[RC_USE], (unsigned long long)popc(b_use));
        if (b_non) atomicAdd(&sh[RC_NONMEM], (unsigned long long)popc(b_non));
        if (b_dn) atomicAdd(&sh[RC_DOWN], (unsigned long long)popc(b_dn));
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < RC_N; j += blockDim.x)
        if (sh[j]) atomicAdd(&cs[j], sh[j]);
}

// what an entry (case j, ttl tt, node v) -> c does at level lvl (0: the origin)
// once its node's rows are known: d_act / d_conn: the target is an active
// member of v / state(v, d) is connected.  Returns whether v forwards, and
// with which ttl; the entry's own tallies go into the block's tile
DEV bool rl_decide(unsigned long long* sh, unsigned long long* tl, uint32_t j, uint32_t tt, uint32_t T,
                   unsigned long long c, uint32_t lvl, bool d_act, bool d_conn, uint32_t& ft) {
    ft = tt;
    if (lvl == 0) {
        atomicOr(&tl[RF_LIVE], 1ull << j);
        if (d_conn) atomicOr(&tl[RF_DIRECT], 1ull << j);
    }
    if (lvl == 0 ? d_conn : d_act && d_conn) {
        atomicAdd(&sh[RF_DELIV * PSIM_RELAY_CASES + j], c);
        atomicAdd(&sh[RF_HOPS * PSIM_RELAY_CASES + j], c * (lvl + 1));
        atomicMin(&sh[RF_FIRST * PSIM_RELAY_CASES + j], (unsigned long long)(lvl + 1));
        return false;
    }
    if (lvl == 0) return true;
    if (d_act) {
        atomicAdd(&sh[RF_RESTART * PSIM_RELAY_CASES + j], c);
        ft = T;
        return true;
    }
    if (tt == 0) {
        atomicAdd(&sh[RF_EXPIRED * PSIM_RELAY_CASES + j], c);
        return false;
    }
    return true;
}

template <uint32_t LN>
__global__ void __launch_bounds__(BLK) k_rl_expand(RlRows R, const uint8_t* __restrict__ flags, uint32_t N,
                                                   const uint32_t* __restrict__ par,
                                                   const unsigned long long* __restrict__ fkey,
                                                   const unsigned long long* __restrict__ fcnt, uint64_t nf,
                                                   uint32_t lvl, unsigned long long* ckey,
                                                   unsigned long long* ccnt, unsigned long long* rv,
                                                   unsigned long long* tl) {
    static_assert(LN == RL_ROW || LN == 1, "a group a row, or a lane an entry");
    __shared__ unsigned long long sh[RF_FIELDS * PSIM_RELAY_CASES];
    __shared__ unsigned long long sh_base;
    for (uint32_t q = threadIdx.x; q < RF_FIELDS * PSIM_RELAY_CASES; q += blockDim.x)
        sh[q] = q / PSIM_RELAY_CASES == RF_FIRST ? RL_EMPTY : 0ull;
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * BLK + threadIdx.x, ei = t / LN;
    const uint32_t l = lane_id(), g = (uint32_t)(t % LN), gb = l - g;
    bool on = ei < nf;
    const unsigned long long key = on ? fkey[ei] : 0ull, c = on ? fcnt[ei] : 0ull;
    const uint32_t j = (uint32_t)(key >> 32), tt = (uint32_t)(key >> KEY_DST_BITS) & 31u, v = (uint32_t)key & KEY_DST_MASK;
    const uint32_t d = par[RP_DST + j], T = par[RP_TTL + j];
    // (the origin: a case whose source or target is not live is skipped)
    if (lvl == 0) on = on && (flags[v] & F_UP) && (flags[d] & F_UP);
    uint32_t an = 0, en = 0, kn = 0;
    if (on) R.counts(v, an, en, kn);
    uint32_t emit = 0, ft = 0;
    uint32_t child[LN == 1 ? RL_ROW : 1];
    if constexpr (LN == RL_ROW) {
        // entry g of each row in lane g
        const uint32_t e = g < en ? R.com[(size_t)v * RL_ROW + g] : PSIM_NONE;
        const uint32_t a = g < an ? R.act[(size_t)v * RL_ROW + g] : PSIM_NONE;
        const uint32_t k = g < kn ? R.conn[(size_t)v * RL_ROW + g] : PSIM_NONE;
        const uint32_t p = e & ~PSIM_MAP_BIT;
        bool in_act = false, dn = false, pl = false, d_act = false, d_dn = false, d_pl = false;
#pragma unroll
        for (uint32_t q = 0; q < RL_ROW; q++) {        // (every lane of the wave: no branch around a shuffle)
            const uint32_t aq = shfl(a, (int)(gb + q)), kq = shfl(k, (int)(gb + q));
            in_act |= aq == p; dn |= kq == (p | PSIM_CONN_DOWN); pl |= kq == p;
            d_act |= aq == d; d_dn |= kq == (d | PSIM_CONN_DOWN); d_pl |= kq == d;
        }
        const bool d_conn = rl_state(v != d, d_act, d_dn, d_pl) == RL_CONN;      // (d is live: the case is)
        bool fwd = false;
        if (on && g == 0) fwd = rl_decide(sh, tl, j, tt, T, c, lvl, d_act, d_conn, ft);
        fwd = shfl(fwd ? 1u : 0u, (int)gb) != 0; ft = shfl(ft, (int)gb);
        const bool oe = fwd && g < en && e != v;
        const bool usable = oe && rl_state(rl_live(flags, N, v, p), in_act, dn, pl) == RL_CONN;
        const uint32_t nrel = popc((ballot(usable) >> gb) & 0xFFull), nref = popc((ballot(oe && !usable) >> gb) & 0xFFull);
        if (g == 0 && nrel) atomicAdd(&sh[RF_RELAY * PSIM_RELAY_CASES + j], c * nrel);
        if (g == 0 && nref) atomicAdd(&sh[RF_REFUSED * PSIM_RELAY_CASES + j], c * nref);
        if (usable) { emit = 1; child[0] = p; }
    } else {
        if (on) {
            uint32_t e[RL_ROW], a[RL_ROW], k[RL_ROW];
            const uint4* re = reinterpret_cast<const uint4*>(R.com + (size_t)v * RL_ROW);
            const uint4* ra = reinterpret_cast<const uint4*>(R.act + (size_t)v * RL_ROW);
            const uint4* rk = reinterpret_cast<const uint4*>(R.conn + (size_t)v * RL_ROW);
            const uint4 e0 = re[0], e1 = re[1], a0 = ra[0], a1 = ra[1], k0 = rk[0], k1 = rk[1];
            e[0] = e0.x; e[1] = e0.y; e[2] = e0.z; e[3] = e0.w; e[4] = e1.x; e[5] = e1.y; e[6] = e1.z; e[7] = e1.w;
            a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
            k[0] = k0.x; k[1] = k0.y; k[2] = k0.z; k[3] = k0.w; k[4] = k1.x; k[5] = k1.y; k[6] = k1.z; k[7] = k1.w;
#pragma unroll
            for (uint32_t q = 0; q < RL_ROW; q++) {
                if (q >= an) a[q] = PSIM_NONE;
                if (q >= kn) k[q] = PSIM_NONE;
            }
            bool d_act = false, d_dn = false, d_pl = false;
#pragma unroll
            for (uint32_t q = 0; q < RL_ROW; q++) { d_act |= a[q] == d; d_dn |= k[q] == (d | PSIM_CONN_DOWN); d_pl |= k[q] == d; }
            const bool d_conn = rl_state(v != d, d_act, d_dn, d_pl) == RL_CONN;
            if (rl_decide(sh, tl, j, tt, T, c, lvl, d_act, d_conn, ft)) {
                uint32_t nref = 0;
#pragma unroll
                for (uint32_t r = 0; r < RL_ROW; r++) {
                    if (r >= en || e[r] == v) continue;
                    const uint32_t p = e[r] & ~PSIM_MAP_BIT;
                    bool in_act = false, dn = false, pl = false;
#pragma unroll
                    for (uint32_t q = 0; q < RL_ROW; q++) { in_act |= a[q] == p; dn |= k[q] == (p | PSIM_CONN_DOWN); pl |= k[q] == p; }
                    if (rl_state(rl_live(flags, N, v, p), in_act, dn, pl) == RL_CONN) child[emit++] = p;
                    else nref++;
                }
                if (emit) atomicAdd(&sh[RF_RELAY * PSIM_RELAY_CASES + j], c * emit);
                if (nref) atomicAdd(&sh[RF_REFUSED * PSIM_RELAY_CASES + j], c * nref);
            }
        }
    }
    // the block's children side by side: one returning global add a block
    uint32_t tot;
    const uint32_t at = block_excl<uint32_t>(emit, &tot);
    if (threadIdx.x == 0) sh_base = tot ? atomicAdd(&rv[RV_CHILD], (unsigned long long)tot) : 0ull;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < (LN == 1 ? RL_ROW : 1); r++)
        if (r < emit) { ckey[sh_base + at + r] = rl_key(j, ft - 1, child[r]); ccnt[sh_base + at + r] = c; }
    for (uint32_t q = threadIdx.x; q < RF_FIELDS * PSIM_RELAY_CASES; q += blockDim.x) {
        if (q / PSIM_RELAY_CASES == RF_FIRST) { if (sh[q] != RL_EMPTY) atomicMin(&tl[q], sh[q]); }
        else if (sh[q]) atomicAdd(&tl[q], sh[q]);
    }
}

// tkey: RL_EMPTY in every free slot; mask: the slots - 1 (a power of two, at
// least twice the children, so a probe ends at a free slot)
__global__ void __launch_bounds__(BLK) k_rl_merge(const unsigned long long* __restrict__ ckey,
                                                  const unsigned long long* __restrict__ ccnt, uint64_t m,
                                                  unsigned long long* tkey, unsigned long long* tcnt, uint64_t mask) {
    const uint64_t t = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (t >= m) return;
    const unsigned long long key = ckey[t], c = ccnt[t];
    uint64_t s = mix64(key) & mask;
    for (uint64_t it = 0; it <= mask; it++, s = (s + 1) & mask) {
        // (a slot goes from free to one key once: a key read here is final, a free slot is tried)
        unsigned long long old = __hip_atomic_load(&tkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == RL_EMPTY) old = atomicCAS(&tkey[s], RL_EMPTY, key);
        if (old == RL_EMPTY || old == key) { atomicAdd(&tcnt[s], c); return; }
    }
}

__global__ void __launch_bounds__(BLK) k_rl_compact(const unsigned long long* __restrict__ tkey,
                                                    const unsigned long long* __restrict__ tcnt, uint64_t slots,
                                                    unsigned long long* fkey, unsigned long long* fcnt,
                                                    unsigned long long* rv) {
    __shared__ unsigned long long sh[2 * PSIM_RELAY_CASES];
    __shared__ unsigned long long sh_base;
    if (threadIdx.x < 2 * PSIM_RELAY_CASES) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    const unsigned long long key = s < slots ? tkey[s] : RL_EMPTY;
    const bool used = key != RL_EMPTY;
    const unsigned long long c = used ? tcnt[s] : 0ull;
    if (used) {
        atomicAdd(&sh[key >> 32], 1ull);
        atomicAdd(&sh[PSIM_RELAY_CASES + (key >> 32)], c);
    }
    uint32_t tot;
    const uint32_t at = block_excl<uint32_t>(used ? 1u : 0u, &tot);
    if (threadIdx.x == 0) sh_base = tot ? atomicAdd(&rv[RV_NEXT], (unsigned long long)tot) : 0ull;
    __syncthreads();
    if (used) { fkey[sh_base + at] = key; fcnt[sh_base + at] = c; }
    if (threadIdx.x < 2 * PSIM_RELAY_CASES && sh[threadIdx.x]) atomicAdd(&rv[RV_DISTINCT + threadIdx.x], sh[threadIdx.x]);
}

// ---------------------------------------------- latency-weighted paths --
// psim_get_latency_metrics (psim_latency_metrics in the header defines every
// field).  A node's state is a row of LT_W distances, lane = source slot,
// 256 B: a wave reads or relaxes a whole row in one coalesced access.  Two rows
// a node: `cur` takes the atomicMins of a sweep, `prev` is the row as of the
// end of the sweep before, and the only thing a push reads -- so sweep r
// computes exactly D_r whatever the order of the atomics.  The frontier words
// are WordBfs' shape: bit j of front[i] = "slot j of node i fell last sweep".
//   k_lt_cell     a node's torus cell (20 bits), one mix64 a node (the A/B form of the weights)
//   k_lt_census   a thread a node over its row of L (or T): the link costs
//   k_lt_init     the rows' zeros at the live sources, their frontier bits
//   k_lt_push     a wave takes 64 nodes' frontier words and relaxes the rows
//                 of the nodes on the frontier, one after the other
//   k_lt_push_list  a wave a node of the compacted frontier list
//   k_lt_level    the fallen lanes cur -> prev, front = next, next = 0, the
//                 frontier list, the sweep's OR word and node count
//   k_lt_final    one pass over the rows: per slot reach, sum, max; the histogram
//   k_lt_column / k_lt_tree   slot 0 of every row; the tree half's comparison
constexpr uint32_t LT_W = PSIM_LAT_SOURCES;
constexpr uint32_t LT_INF = 0xFFFFFFFFu;
enum { LC_NUP = 0, LC_LINKS, LC_COST, LC_NODES, LC_WORST, LC_BEST, LC_HIST, LC_N = LC_HIST + PSIM_HIST_BINS };
enum { LF_REACH = 0, LF_SUM = LT_W, LF_HIST = 2 * LT_W, LF_ECC = 2 * LT_W + PSIM_HIST_BINS, LF_N = LF_ECC + LT_W };
enum { LR_TREACH = 0, LR_TSUM, LR_OREACH, LR_BOTH, LR_TSUMB, LR_OSUMB, LR_SLOWER, LR_FASTER, LR_TMAX, LR_N };

DEV uint32_t lt_cell_of(uint64_t seed, uint32_t i) {
    return (uint32_t)mix64(seed ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull)) & 0xFFFFFu;
}
// w(i, p), i != p: from the cells (cell != nullptr), or xbot_latency itself
DEV uint32_t lt_weight(const uint32_t* __restrict__ cell, uint64_t seed, uint32_t i, uint32_t p) {
    if (!cell) return xbot_latency(seed, i, p);
    const uint32_t a = cell[i], b = cell[p];
    return xbot_axis(a & 1023u, b & 1023u) + xbot_axis(a >> 10, b >> 10);
}

__global__ void k_lt_cell(uint64_t seed, uint32_t n, uint32_t* cell) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cell[i] = lt_cell_of(seed, i);
}

__global__ void __launch_bounds__(BLK) k_lt_census(Links ln, const uint8_t* __restrict__ flags, uint32_t n,
                                                   const uint32_t* __restrict__ cell, uint64_t seed,
                                                   unsigned long long* lc) {
    __shared__ unsigned long long sh[LC_N];
    for (uint32_t j = threadIdx.x; j < LC_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool up = i < n && (flags[i] & F_UP);
    const uint32_t c = up ? ln.cnt[i] : 0;
    uint32_t sum = 0, hi = 0, lo = LT_INF;
    if (c) {
        const uint32_t* row = ln.row(i);
        for (uint32_t k = 0; k < c; k++) {
            const uint32_t w = lt_weight(cell, seed, i, row[k]);
            sum += w; hi = max(hi, w); lo = min(lo, w);
            atomicAdd(&sh[LC_HIST + hbin(w >> 4)], 1ull);
        }
    }
    const uint32_t nup = popc(ballot(up)), nodes = popc(ballot(c != 0));
    const uint32_t links = sh_wave_sum(c), cost = sh_wave_sum(sum);          // (a wave: 64 * 128 * 1024 at the most)
    const uint32_t worst = sh_wave_sum(hi), best = sh_wave_sum(c ? lo : 0u);
    if (lane_id() == 0 && nup) {
        atomicAdd(&sh[LC_NUP], (unsigned long long)nup);
        if (nodes) {
            atomicAdd(&sh[LC_LINKS], (unsigned long long)links); atomicAdd(&sh[LC_COST], (unsigned long long)cost);
            atomicAdd(&sh[LC_NODES], (unsigned long long)nodes);
            atomicAdd(&sh[LC_WORST], (unsigned long long)worst); atomicAdd(&sh[LC_BEST], (unsigned long long)best);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < LC_N; j += blockDim.x)
        if (sh[j]) atomicAdd(&lc[j], sh[j]);
}

// slot j starts at sources[j] if that node is live: distance 0 in both rows
// (all others LT_INF), its frontier bit, its place in the frontier list; lv[0]:
// the mask of such slots, lv[1]: their number (one block of 64 threads; the
// sources are distinct and < n)
__global__ void k_lt_init(const uint32_t* __restrict__ sources, uint32_t ns, const uint8_t* __restrict__ flags,
                          uint32_t* cur, uint32_t* prev, unsigned long long* front, uint32_t* list,
                          unsigned long long* lv) {
    const uint32_t j = threadIdx.x;
    const bool on = j < ns && (flags[sources[j]] & F_UP);
    const uint64_t m = ballot(on);
    if (on) {
        const uint32_t s = sources[j];
        cur[(size_t)s * LT_W + j] = 0; prev[(size_t)s * LT_W + j] = 0;
        front[s] = 1ull << j;
        list[popc(m & lt_mask())] = s;
    }
    if (j == 0) { lv[0] = m; lv[1] = popc(m); }
}

// the wave relaxes the out-links of frontier node i: lane j holds prev[i][j];
// the row's ids and weights sit one link a lane (two for a long CSR row), so a
// weight is computed once per link; per link the lanes of f do the atomicMin,
// and the ballot of those that lowered the target is one atomicOr into next
DEV void lt_relax(Links ln, const uint32_t* __restrict__ cell, uint64_t seed, uint32_t i, uint64_t f,
                  const uint32_t* __restrict__ prev, uint32_t* cur, unsigned long long* next) {
    const uint32_t l = lane_id();
    const uint32_t c = min((uint32_t)ln.cnt[i], (uint32_t)PSIM_SVIEW_CAP);
    if (!c) return;                                   // (uniform)
    const uint32_t d = prev[(size_t)i * LT_W + l];
    const bool mine = ((f >> l) & 1) && d != LT_INF;
    uint32_t a, b, wa = 0, wb = 0;
    sh_row_load(ln.row(i), c, a, b);
    if (l < c) wa = lt_weight(cell, seed, i, a);
    if (64 + l < c) wb = lt_weight(cell, seed, i, b);
    for (uint32_t t = 0; t < c; t++) {                // (uniform)
        const uint32_t p = t < 64 ? shfl(a, (int)t) : shfl(b, (int)(t - 64));
        const uint32_t w = t < 64 ? shfl(wa, (int)t) : shfl(wb, (int)(t - 64));
        const uint32_t nd = d + w;
        uint32_t* at = cur + (size_t)p * LT_W + l;
        // (a stale read can only be too large: a distance never rises)
        const bool fell = mine && nd < *at && atomicMin(at, nd) > nd;
        const uint64_t m = ballot(fell);
        if (m && l == 0) atomicOr(&next[p], (unsigned long long)m);
    }
}

__global__ void __launch_bounds__(BLK) k_lt_push(Links ln, uint32_t n, const uint32_t* __restrict__ cell,
                                                 uint64_t seed, const unsigned long long* __restrict__ front,
                                                 const uint32_t* __restrict__ prev, uint32_t* cur,
                                                 unsigned long long* next) {
    const uint32_t base = (blockIdx.x * (BLK / 64) + (threadIdx.x >> 6)) * 64;     // this wave's first node
    const uint32_t mine = base + lane_id();
    const uint64_t f = mine < n ? front[mine] : 0;
    uint64_t todo = ballot(f != 0);
    while (todo) {                                    // (uniform)
        const int k = ffs64(todo);
        todo &= todo - 1;
        lt_relax(ln, cell, seed, base + (uint32_t)k, shfl64(f, k), prev, cur, next);
    }
}

__global__ void __launch_bounds__(BLK) k_lt_push_list(Links ln, const uint32_t* __restrict__ list, uint32_t nf,
                                                      const uint32_t* __restrict__ cell, uint64_t seed,
                                                      const unsigned long long* __restrict__ front,
                                                      const uint32_t* __restrict__ prev, uint32_t* cur,
                                                      unsigned long long* next) {
    const uint32_t q = blockIdx.x * (BLK / 64) + (threadIdx.x >> 6);               // (uniform per wave)
    if (q >= nf) return;
    const uint32_t i = list[q];
    lt_relax(ln, cell, seed, i, front[i], prev, cur, next);
}

// a wave takes 64 nodes: where next[i] != 0 its lanes of cur go to prev;
// front = next, next = 0; the nodes go into the frontier list at lv[1]'s
// count (list == nullptr: no list); lv[0]: the OR of the sweep's words
__global__ void __launch_bounds__(BLK) k_lt_level(uint32_t n, unsigned long long* next, unsigned long long* front,
                                                  const uint32_t* __restrict__ cur, uint32_t* prev, uint32_t* list,
                                                  unsigned long long* lv) {
    __shared__ unsigned long long sh_or;
    if (threadIdx.x == 0) sh_or = 0;
    __syncthreads();
    const uint32_t l = lane_id();
    const uint32_t base = (blockIdx.x * (BLK / 64) + (threadIdx.x >> 6)) * 64;
    const uint32_t mine = base + l;
    unsigned long long nx = 0;
    if (mine < n) {
        nx = next[mine];
        if (nx) next[mine] = 0;
        if (front[mine] != nx) front[mine] = nx;
    }
    const uint64_t some = ballot(nx != 0);
    if (some) {                                       // (uniform)
        uint64_t todo = some;
        while (todo) {
            const int k = ffs64(todo);
            todo &= todo - 1;
            const size_t at = (size_t)(base + (uint32_t)k) * LT_W + l;
            if ((shfl64(nx, k) >> l) & 1) prev[at] = cur[at];
        }
        const uint64_t w = wave_or(nx);
        uint32_t pos = 0;
        if (l == 0) {
            atomicOr(&sh_or, (unsigned long long)w);
            pos = (uint32_t)atomicAdd(&lv[1], (unsigned long long)popc(some));
        }
        pos = shfl(pos, 0);
        if (list && nx) list[pos + popc(some & lt_mask())] = mine;
    }
    __syncthreads();
    if (threadIdx.x == 0 && sh_or) atomicOr(&lv[0], sh_or);
}

// one pass over the rows after the last sweep: a wave a node at a time, lane =
// slot; the per-slot counts stay in the lane's registers, then the block's LDS
// tile, then one global add per block and word
__global__ void __launch_bounds__(BLK) k_lt_final(const uint32_t* __restrict__ cur,
                                                  const uint32_t* __restrict__ sources,
                                                  const uint8_t* __restrict__ flags, uint32_t n, uint32_t per_wave,
                                                  unsigned long long* lf) {
    __shared__ unsigned long long sh[LF_N];
    for (uint32_t j = threadIdx.x; j < LF_N; j += blockDim.x) sh[j] = 0;
    __syncthreads();
    const uint32_t l = lane_id();
    const uint32_t src = sources[l];                  // (slots past the sources: never finite)
    const uint32_t lo = (blockIdx.x * (BLK / 64) + (threadIdx.x >> 6)) * per_wave;
    const uint32_t hi = min(n, lo + per_wave);
    uint32_t reach = 0, ecc = 0;
    unsigned long long sum = 0;
    for (uint32_t v = lo; v < hi; v++) {              // (uniform)
        if (!(flags[v] & F_UP)) continue;
        const uint32_t d = cur[(size_t)v * LT_W + l];
        if (d == LT_INF || v == src) continue;
        reach++; sum += d; ecc = max(ecc, d);
        atomicAdd(&sh[LF_HIST + hbin(d >> 8)], 1ull);
    }
    if (reach) {
        atomicAdd(&sh[LF_REACH + l], (unsigned long long)reach);
        atomicAdd(&sh[LF_SUM + l], sum);
        atomicMax(&sh[LF_ECC + l], (unsigned long long)ecc);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < LF_N; j += blockDim.x) {
        if (!sh[j]) continue;
        if (j >= LF_ECC) atomicMax(&lf[j], sh[j]);
        else atomicAdd(&lf[j], sh[j]);
    }
}

// slot 0 of every row
__global__ void k_lt_column(const uint32_t* __restrict__ cur, uint32_t n, uint32_t* col) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) col[i] = cur[(size_t)i * LT_W];
}

// per live node v != root: its latency over T (dt) against that over L (dl)
__global__ void __launch_bounds__(BLK) k_lt_tree(const uint32_t* __restrict__ dt, const uint32_t* __restrict__ dl,
                                                 const uint8_t* __restrict__ flags, uint32_t n, uint32_t root,
                                                 unsigned long long* lr) {
    __shared__ unsigned long long sh[LR_N];
    if (threadIdx.x < LR_N) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s[LR_TMAX] = {0}, mx = 0;
    if (i < n && i != root && (flags[i] & F_UP)) {
        const uint32_t a = dt[i], b = dl[i];
        if (a != LT_INF) { s[LR_TREACH] = 1; s[LR_TSUM] = a; mx = a; }
        if (b != LT_INF) s[LR_OREACH] = 1;
        if (a != LT_INF && b != LT_INF) {
            s[LR_BOTH] = 1; s[LR_TSUMB] = a; s[LR_OSUMB] = b;
            s[LR_SLOWER] = a > b ? 1u : 0u; s[LR_FASTER] = a < b ? 1u : 0u;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < LR_TMAX; j++) {
        const uint32_t v = sh_wave_sum(s[j]);         // (a wave's latencies: 64 * 2^22 at the most)
        if (lane_id() == 0 && v) atomicAdd(&sh[j], (unsigned long long)v);
    }
    if (ballot(mx != 0)) {                            // (uniform)
        for (int d = 32; d; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
        if (lane_id() == 0) atomicMax(&sh[LR_TMAX], (unsigned long long)mx);
    }
    __syncthreads();
    if (threadIdx.x < LR_N && sh[threadIdx.x]) {
        if (threadIdx.x == LR_TMAX) atomicMax(&lr[threadIdx.x], sh[threadIdx.x]);
        else atomicAdd(&lr[threadIdx.x], sh[threadIdx.x]);
    }
}

}  // namespace

// ---------------------------------------------------------------- host --
// A getter's start, after its argument and state checks: the device set, the
// result zeroed, every shard's stream idle.  st: the stream the getter works
// on; fl: the flags (replicated: every shard holds all N)
static int getter_begin(psim_handle* h, void* out, size_t bytes, hipStream_t& st, const uint8_t*& fl) {
    if (hipSetDevice(h->device) != hipSuccess) return PSIM_EDEVICE;
    memset(out, 0, bytes);
    for (Shard* s : h->shards) HIP_TRY(hipStreamSynchronize(s->stream));
    st = h->shards[0]->stream; fl = h->shards[0]->flags.p;
    return PSIM_OK;
}

// the level cap of a BFS getter (m = 0: the largest)
static uint32_t level_cap(uint32_t m) { return !m || m > PSIM_GRAPH_MAX_LEVELS ? PSIM_GRAPH_MAX_LEVELS : m; }

// n device words to the host, waited for
template <typename T>
static int read_back(hipStream_t st, T* dst, const T* src, size_t n = 1) {
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSIM_OK;
}

// weakly connected components of the live nodes over the rows k_cc_hook
// reads: root hooking and pointer jumping to a fixed point, then the component
// count and the largest (comps, largest: zeroed device words; L, size: n
// words, size zeroed).  A pass that hooks nothing ends the loop: every link
// then joins two nodes of one tree, and a tree never leaves its component.
// Every other pass takes at least one root away (the larger root of a link
// between two trees gets a parent, and no node ever becomes a root again), so
// n passes are the most there can be.  Running out of the bound is an error,
// never a count (the getter's time on a path of 12 500 nodes whose ids run
// against it: profiles/synthetic_overlays/cc_before.txt)
static int cc_run(Links ln, const uint8_t* fl, uint32_t n, uint32_t* L, uint32_t* size, uint32_t* flag,
                  unsigned long long* comps, unsigned long long* largest, hipStream_t st) {
    k_cc_init<<<grid_for(n), BLK, 0, st>>>(fl, n, L);
    uint32_t changed = 1;
    for (uint64_t it = 0; changed && it < (uint64_t)n + 2; it++) {
        HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
        k_cc_hook<<<grid_for(n), BLK, 0, st>>>(ln, fl, n, L, flag);
        k_cc_jump<<<grid_for(n), BLK, 0, st>>>(n, L);
        TRY(read_back(st, &changed, flag));
    }
    // (unreachable: the bound above cannot run out.  Were it to, on a ranked
    // handle this return would come before the caller's next collective and
    // leave the other ranks waiting in it)
    if (changed) return PSIM_ESTATE;
    k_cc_count<<<grid_for(n), BLK, 0, st>>>(L, n, size, comps);
    k_cc_max<<<grid_for(n), BLK, 0, st>>>(size, n, largest);
    HIP_TRY(hipGetLastError());
    return PSIM_OK;
}

// the whole overlay's active rows by global id, gact (PSIM_ACTIVE_CAP ids a
// row) and gan (their lengths), of per * G rows: the shards' rows are gathered
// (device copies for virtual shards, an in-place ncclAllGather of equal
// per-rank slots for RCCL ranks; 33 B per node), and every process then runs
// the same kernels over the whole overlay
static int gather_active_rows(psim_handle* h, hipStream_t st, TmpBuf<uint32_t>& gact, TmpBuf<uint8_t>& gan) {
    const uint32_t per = h->per;
    const size_t npad = (size_t)per * h->G;
    TRY(gact.alloc_on(npad * PSIM_ACTIVE_CAP, st)); TRY(gan.alloc_on(npad, st));
    for (Shard* s : h->shards)
        if (s->n)
            k_pack_act<<<grid_for(s->n), BLK, 0, st>>>(s->hdr.p, s->act.p, s->n,
                                                       gact.p + (size_t)s->lo * PSIM_ACTIVE_CAP, gan.p + s->lo);
    if (h->ranked) {
        const size_t off = (size_t)h->rank * per;
        TRY(h->comm->all_gather(gact.p + off * PSIM_ACTIVE_CAP, gact.p, (size_t)per * PSIM_ACTIVE_CAP * 4, st));
        TRY(h->comm->all_gather(gan.p + off, gan.p, per, st));
    }
    return PSIM_OK;
}

extern "C" int psim_get_histograms(psim_handle* h, psim_histograms* out) {
    if (!h || !out) return PSIM_EINVAL;
    if (h->cfg.manager == PSIM_MANAGER_PLUGGABLE || h->hosted) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    const size_t N = h->N;
    TmpBuf<uint32_t> ind;                        // in-degrees, active then passive, by global id
    TmpBuf<unsigned long long> hist;
    TRY(ind.alloc_on(2 * N, st)); TRY(hist.alloc_on(H_N + 4, st));
    const uint64_t tbit = h->tracked_msg == PSIM_NONE ? 0ull : 1ull << (h->tracked_msg % PSIM_MSG_SLOTS);
    for (Shard* s : h->shards)
        k_hist_out<<<grid_for(s->n), BLK, 0, st>>>(s->hdr.p, s->act.p, s->pas.p, s->flags.p, s->lo, s->n, tbit,
                                                   ind.p, ind.p + N, hist.p);
    if (h->ranked) TRY(h->comm->all_reduce(ind.p, 2 * N, CType::U32, COp::SUM, st));
    for (Shard* s : h->shards)
        k_hist_in<<<grid_for(s->n), BLK, 0, st>>>(ind.p, ind.p + N, s->flags.p, s->lo, s->n, hist.p);
    std::vector<unsigned long long> hv(H_N + 4, 0);
    TRY(read_back(st, hv.data(), hist.p, H_N + 4));
    if (h->ranked) {                             // sums over ranks; the latest round: max
        hv[H_N] = hv[H_LAST];
        TRY(h->comm_cnt.ensure(H_N + 4));
        HIP_TRY(hipMemcpyAsync(h->comm_cnt.p, hv.data(), (H_N + 4) * 8, hipMemcpyHostToDevice, st));
        TRY(h->comm->all_reduce(h->comm_cnt.p, H_N, CType::U64, COp::SUM, st));
        TRY(h->comm->all_reduce(h->comm_cnt.p + H_N, 1, CType::U64, COp::MAX, st));
        TRY(read_back(st, hv.data(), (const unsigned long long*)h->comm_cnt.p, H_N + 4));
        hv[H_LAST] = hv[H_N];
    }
    for (int k = 0; k < PSIM_HIST_BINS; k++) {
        out->active_in[k] = hv[H_AIN * PSIM_HIST_BINS + k];
        out->passive_in[k] = hv[H_PIN * PSIM_HIST_BINS + k];
        out->active_out[k] = hv[H_AOUT * PSIM_HIST_BINS + k];
        out->passive_fill[k] = hv[H_PFILL * PSIM_HIST_BINS + k];
        out->hop[k] = hv[H_HOP * PSIM_HIST_BINS + k];
    }
    out->n_up = hv[H_NUP]; out->delivered = hv[H_DELIV]; out->last_round = hv[H_LAST];
    out->active_links = hv[H_LINKS];
    // symmetry and components need every node's active row
    const uint32_t n = h->N;
    TmpBuf<uint32_t> gact, L, sz, flag;
    TmpBuf<uint8_t> gan;
    TmpBuf<unsigned long long> r;
    TRY(gather_active_rows(h, st, gact, gan));
    TRY(L.alloc_on(n, st)); TRY(sz.alloc_on(n, st)); TRY(flag.alloc_on(1, st)); TRY(r.alloc_on(3, st));
    k_hist_sym<<<grid_for(n), BLK, 0, st>>>(gan.p, gact.p, fl, n, r.p);
    TRY(cc_run(Links{nullptr, gan.p, gact.p}, fl, n, L.p, sz.p, flag.p, r.p + 1, r.p + 2, st));
    unsigned long long rv[3];
    TRY(read_back(st, rv, r.p, 3));
    out->symmetric_links = rv[0]; out->components = rv[1]; out->largest_component = rv[2];
    return PSIM_OK;
}

// the full strategy's statistics, over every shard of this process and, on
// ranks, as a collective (every rank gets the same struct).  The flags are
// replicated, so every shard finds the lowest live id itself; its row belongs
// to one shard or rank -- a device pointer serves virtual shards, ranks
// all-reduce the row (its owner's words, zeros elsewhere: the sum is the row).
// The ranks' minimum is the maximum of the complement (Comm reduces SUM and MAX)
static int strategy_hist_full(psim_handle* h, hipStream_t st, const uint8_t* fl, psim_strategy_histograms* out) {
    TmpBuf<unsigned long long> sf;
    TmpBuf<uint32_t> low, ref;
    TRY(sf.alloc_on(SF_N, st)); TRY(low.alloc_on(1, st));
    HIP_TRY(hipMemsetAsync(sf.p + SF_MIN, 0xFF, 8, st));
    HIP_TRY(hipMemsetAsync(low.p, 0xFF, 4, st));
    k_sh_low<<<grid_for(h->N), BLK, 0, st>>>(fl, 0, h->N, low.p);
    HIP_TRY(hipGetLastError());
    uint32_t lowest = PSIM_NONE;
    TRY(read_back(st, &lowest, low.p));
    if (lowest != PSIM_NONE) {
        Shard* o = owner_of(h, lowest);
        const uint32_t* rp = o ? o->fbits.p + (size_t)(lowest - o->lo) * 2 * h->fw : nullptr;
        if (h->ranked && h->world > 1) {
            TRY(ref.alloc_on(2 * h->fw, st));
            if (rp) HIP_TRY(hipMemcpyAsync(ref.p, rp, 2 * h->fw * 4, hipMemcpyDeviceToDevice, st));
            TRY(h->comm->all_reduce(ref.p, 2 * h->fw, CType::U32, COp::SUM, st));
            rp = ref.p;
        }
        if (!rp) return PSIM_ESTATE;
        for (Shard* s : h->shards)
            if (s->n)
                k_sh_full<<<grid_for((uint64_t)s->n * 64), BLK, 0, st>>>(s->fbits.p, s->flags.p, s->lo, s->n, h->fw,
                                                                       h->tomb ? 1u : 0u, rp, sf.p);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long v[SF_N];
    TRY(read_back(st, v, sf.p, SF_N));
    if (h->ranked && h->world > 1) {
        // (a rank without live nodes: SF_MIN is still all ones, its complement 0)
        uint64_t w[SF_N] = {v[SF_NUP], v[SF_SUM], v[SF_AGREE], v[SF_MAX], ~(uint64_t)v[SF_MIN]};
        TRY(h->comm_cnt.ensure(SF_N));
        HIP_TRY(hipMemcpyAsync(h->comm_cnt.p, w, sizeof w, hipMemcpyHostToDevice, st));
        TRY(h->comm->all_reduce(h->comm_cnt.p, 3, CType::U64, COp::SUM, st));
        TRY(h->comm->all_reduce(h->comm_cnt.p + 3, 2, CType::U64, COp::MAX, st));
        HIP_TRY(hipMemcpyAsync(w, h->comm_cnt.p, sizeof w, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        v[SF_NUP] = w[0]; v[SF_SUM] = w[1]; v[SF_AGREE] = w[2]; v[SF_MAX] = w[3]; v[SF_MIN] = ~w[4];
    }
    out->n_up = v[SF_NUP];
    if (v[SF_NUP]) {
        out->members_min = v[SF_MIN]; out->members_max = v[SF_MAX]; out->members_sum = v[SF_SUM];
        out->agreeing = v[SF_AGREE];
    }
    return PSIM_OK;
}

// the compact CSR of a SCAMP handle's overlay, the same on every rank: node
// i's cnt[i] links at adj + off[i] (ids by equal per-shard slots, per * G of
// them; the pad ids hold no links)
struct ShCsr {
    TmpBuf<uint8_t> cnt;
    TmpBuf<uint32_t> off, base, adj;
    TmpBuf<unsigned long long> tot;
    Links links() const { return Links{off.p, cnt.p, adj.p}; }
};
// the counts and offsets of a CSR, zeroed, before its count pass
static int csr_alloc(psim_handle* h, hipStream_t st, ShCsr& c) {
    const size_t npad = (size_t)h->per * h->G;
    TRY(c.tot.alloc_on(1, st));
    TRY(c.cnt.alloc_on(npad + 1, st)); TRY(c.off.alloc_on(npad + 1, st));
    TRY(c.base.alloc_on(h->ranked ? (uint32_t)h->world : 1u, st));
    return PSIM_OK;
}
// after the count pass wrote this process's counts: every rank's counts, the
// row offsets and the (empty) links.  slot: the links of a rank's share
static int csr_place(psim_handle* h, hipStream_t st, ShCsr& c, uint32_t& slot) {
    const uint32_t per = h->per, npad = per * h->G;
    const uint32_t W = h->ranked ? (uint32_t)h->world : 1u, rper = h->ranked ? per : npad;
    if (h->ranked) TRY(h->comm->all_gather(c.cnt.p + (size_t)h->rank * per, c.cnt.p, per, st));
    // row offsets: a scan of all counts (entry npad: the total); a rank's
    // rows are packed from the start of its slot, every slot as long as the
    // largest rank's links, so the gathered CSR is the same everywhere
    TRY(scan_excl(h->shards[0], c.cnt.p, c.off.p, npad + 1));
    k_sh_rank_tot<<<1, 64, 0, st>>>(c.off.p, rper, W, npad, c.base.p, c.tot.p);
    unsigned long long slot64 = 0;
    TRY(read_back(st, &slot64, c.tot.p));
    if (slot64 * W > 0xFFFFFFFFull) return PSIM_ENOMEM;       // (row offsets are 32-bit)
    slot = (uint32_t)slot64;
    if (W > 1) k_sh_shift<<<grid_for(npad), BLK, 0, st>>>(c.off.p, npad, rper, slot, c.base.p);
    TRY(c.adj.alloc_on((size_t)slot * W, st));
    return PSIM_OK;
}
// after the pack pass wrote this process's links: every rank's
static int csr_gather(psim_handle* h, hipStream_t st, ShCsr& c, uint32_t slot) {
    if (h->ranked && slot) TRY(h->comm->all_gather(c.adj.p + (size_t)h->rank * slot, c.adj.p, (size_t)slot * 4, st));
    return PSIM_OK;
}

static uint32_t rows_grid(uint32_t n) { return (n + SH_NPB - 1) / SH_NPB; }   // k_sh_rows, k_sh_inv: blocks
// sl: the SL_N words the count pass adds its per-node statistics to
static int sh_build_csr(psim_handle* h, hipStream_t st, unsigned long long* sl, ShCsr& c) {
    const uint8_t* fl = h->shards[0]->flags.p;   // replicated: every shard holds all N
    const uint32_t N = h->N, v2 = h->cfg.strategy == PSIM_STRATEGY_SCAMP_V2 ? 1u : 0u;
    auto rows = [&](const uint32_t* off, uint32_t* adj) {
        for (Shard* s : h->shards)
            if (s->n)
                k_sh_rows<<<rows_grid(s->n), BLK, 0, st>>>(s->hdr.p, s->sview.p, fl, s->lo, s->n, N, v2, c.cnt.p, off,
                                                           adj, sl);
    };
    TRY(csr_alloc(h, st, c));
    // 1. the row pass: per-node statistics, and the link count of every node
    rows(nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    // 2. row offsets, then the pack pass
    uint32_t slot = 0;
    TRY(csr_place(h, st, c, slot));
    rows(c.off.p, c.adj.p);
    HIP_TRY(hipGetLastError());
    return csr_gather(h, st, c, slot);
}

// The overlay's link set L as rows, the same on every rank: the SCAMP CSR, or
// HyParView's gathered rows filtered once (p != i, p live, distinct), so that
// every reader sees the same L.  LinkSet owns the buffers behind its Links
struct LinkSet {
    Links ln;
    size_t slots = 0;                            // link slots behind ln.adj
    ShCsr csr;
    TmpBuf<unsigned long long> sl;               // (the count pass's statistics: not reported)
    TmpBuf<uint32_t> gact, fadj;
    TmpBuf<uint8_t> gan, fcnt;
};
static int link_set(psim_handle* h, hipStream_t st, const uint8_t* fl, LinkSet& s) {
    if (h->cfg.manager == PSIM_MANAGER_PLUGGABLE) {
        TRY(s.sl.alloc_on(SL_N, st));
        TRY(sh_build_csr(h, st, s.sl.p, s.csr));
        s.ln = s.csr.links();
        s.slots = s.csr.adj.n;
    } else {
        const uint32_t N = h->N;
        TRY(gather_active_rows(h, st, s.gact, s.gan));
        TRY(s.fadj.alloc_on((size_t)N * PSIM_ACTIVE_CAP, st)); TRY(s.fcnt.alloc_on(N, st));
        k_gm_filter<<<grid_for(N), BLK, 0, st>>>(s.gan.p, s.gact.p, fl, N, s.fadj.p, s.fcnt.p);
        s.ln = Links{nullptr, s.fcnt.p, s.fadj.p};
        s.slots = (size_t)N * PSIM_ACTIVE_CAP;
    }
    return PSIM_OK;
}

// The word BFS (a push kernel, k_gm_level): bit j of a node's word = reached
// in slot j.  seen, front: seeded by the caller; next: zero; lv: 2 (cap + 1)
// zeroed words, a pair a level; reach: a count per slot
struct WordBfs { TmpBuf<unsigned long long> seen, front, next, lv, reach; };
// Its level loop: push() launches the kernel that ORs the frontier's words
// into next (k_gm_push over every link, k_go_push over the chosen ones), then
// the level kernel; the level's two words -- w[0] the OR of its new bits, w[1]
// their number -- are read back after each, and reach[] with them into `cur`
// where the caller wants it per level (nullptr: not).  Zero new bits end it,
// at most `cap` levels; f(d, w) for every level that found something; out:
// levels, ecc_max, truncated
template <class Out, class Push, class F>
static int bfs_levels(hipStream_t st, uint32_t N, uint32_t cap, WordBfs& b, unsigned long long* cur, Out* out,
                      Push push, F f) {
    for (uint32_t d = 1; d <= cap; d++) {
        unsigned long long w[2] = {0, 0};
        unsigned long long* lv = b.lv.p + 2 * (size_t)d;
        push();
        k_gm_level<<<grid_for(N), BLK, 0, st>>>(N, b.next.p, b.seen.p, b.front.p, lv, b.reach.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(w, lv, sizeof w, hipMemcpyDeviceToHost, st));
#ifndef PSIM_RS_NO_REACH_COPY                    // (timing only, `make mvariant`: what this copy costs a level)
        if (cur) HIP_TRY(hipMemcpyAsync(cur, b.reach.p, PSIM_GRAPH_SOURCES * 8, hipMemcpyDeviceToHost, st));
#endif
        HIP_TRY(hipStreamSynchronize(st));
        out->levels = d;
        if (!w[0]) break;
        f(d, w);
        out->ecc_max = d;
        if (d == cap) out->truncated = 1;
    }
    return PSIM_OK;
}

// bfs_levels' f of a getter with a case per slot: cur is reach[] as read back
// with level d, its growth since prev times d is the level's share of the hop sum
template <class Out>
static auto case_levels(Out* out, const unsigned long long* cur, unsigned long long* prev) {
    return [=](uint32_t d, const unsigned long long* w) {
        for (uint32_t j = 0; j < PSIM_FAIL_CASES; j++) {
            if (!((w[0] >> j) & 1)) continue;
            out->hop_sum[j] += (uint64_t)d * (cur[j] - prev[j]);
            out->reached[j] = prev[j] = cur[j];
            out->ecc[j] = d;
        }
    };
}

extern "C" int psim_get_strategy_histograms(psim_handle* h, psim_strategy_histograms* out) {
    if (!h || !out) return PSIM_EINVAL;
    if (h->cfg.manager != PSIM_MANAGER_PLUGGABLE || h->hosted) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    if (h->cfg.strategy == PSIM_STRATEGY_FULL) return strategy_hist_full(h, st, fl, out);
    const uint32_t N = h->N, v2 = h->cfg.strategy == PSIM_STRATEGY_SCAMP_V2 ? 1u : 0u;
    // temporaries: O(N) bytes and words, and the links
    TmpBuf<unsigned long long> sl, sg;
    TmpBuf<uint32_t> indeg, L, sz, flag;
    ShCsr csr;
    TRY(sl.alloc_on(SL_N, st)); TRY(sg.alloc_on(SG_N, st));
    // 1., 2. the row pass and the CSR
    TRY(sh_build_csr(h, st, sl.p, csr));
    const Links ln = csr.links();
    // 3. over the whole CSR (every rank the same): in-degrees, reciprocity,
    // components; the in_view rows are local and probe it
    TRY(indeg.alloc_on(N, st)); TRY(L.alloc_on(N, st)); TRY(sz.alloc_on(N, st)); TRY(flag.alloc_on(1, st));
    k_sh_links<<<grid_for(N), BLK, 0, st>>>(ln, N, indeg.p, sg.p);
    k_sh_in<<<grid_for(N), BLK, 0, st>>>(indeg.p, ln.cnt, fl, N, sg.p);
    if (v2)
        for (Shard* s : h->shards)
            if (s->n)
                k_sh_inv<<<rows_grid(s->n), BLK, 0, st>>>(s->hdr.p, s->sinv.p, fl, s->lo, s->n, N, ln, sl.p);
    HIP_TRY(hipGetLastError());
    TRY(cc_run(ln, fl, N, L.p, sz.p, flag.p, sg.p + SG_COMPS, sg.p + SG_LARGEST, st));
    if (h->ranked) {                             // the local sums over ranks; the longest view: max
        TRY(h->comm->all_reduce(sl.p, SL_VMAX, CType::U64, COp::SUM, st));
        TRY(h->comm->all_reduce(sl.p + SL_VMAX, 1, CType::U64, COp::MAX, st));
    }
    unsigned long long lv[SL_N], gv[SG_N];
    HIP_TRY(hipMemcpyAsync(lv, sl.p, sizeof lv, hipMemcpyDeviceToHost, st));
    TRY(read_back(st, gv, sg.p, SG_N));
    for (int k = 0; k < PSIM_HIST_BINS; k++) {
        out->view_fill[k] = lv[SL_VFILL * PSIM_HIST_BINS + k];
        out->in_fill[k] = lv[SL_IFILL * PSIM_HIST_BINS + k];
        out->out_degree[k] = lv[SL_OUT * PSIM_HIST_BINS + k];
        out->in_degree[k] = gv[k];
    }
    out->n_up = lv[SL_NUP]; out->view_sum = lv[SL_VSUM]; out->in_sum = lv[SL_ISUM]; out->view_max = lv[SL_VMAX];
    out->dangling_links = lv[SL_DANG]; out->self_entries = lv[SL_SELF]; out->duplicate_entries = lv[SL_DUP];
    out->in_view_links = lv[SL_IVL]; out->in_view_confirmed = lv[SL_IVC];
    out->links = gv[SG_LINKS]; out->mutual_links = gv[SG_MUTUAL]; out->in_degree_max = gv[SG_INMAX];
    out->isolated = gv[SG_ISOL]; out->components = gv[SG_COMPS]; out->largest_component = gv[SG_LARGEST];
    return PSIM_OK;
}

extern "C" int psim_get_graph_metrics(psim_handle* h, const uint32_t* sources, size_t n_sources, uint32_t max_levels,
                                      psim_graph_metrics* out) {
    static_assert(PSIM_GRAPH_SOURCES == 64, "one bit of a 64-bit word per source slot");
    if (!h || !out || (n_sources && !sources) || n_sources > PSIM_GRAPH_SOURCES) return PSIM_EINVAL;
    const bool pl = h->cfg.manager == PSIM_MANAGER_PLUGGABLE;
    if (h->hosted || (pl && h->cfg.strategy == PSIM_STRATEGY_FULL)) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    if (h->round_open) return PSIM_ESTATE;
    const uint32_t N = h->N, ns = (uint32_t)n_sources;
    uint32_t src[PSIM_GRAPH_SOURCES] = {0};
    for (uint32_t j = 0; j < ns; j++) {
        if (sources[j] >= N) return PSIM_ERANGE;
        src[j] = sources[j];
    }
    for (uint32_t j = 0; j < ns; j++)
        for (uint32_t q = 0; q < j; q++)
            if (src[q] == src[j]) return PSIM_EINVAL;
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    // 1. the link set as rows: both halves read the same L
    LinkSet ls;
    TmpBuf<unsigned long long> gm;
    TRY(gm.alloc_on(GM_N, st));
    TRY(link_set(h, st, fl, ls));
    // 2. clustering
    if (pl) k_gm_cluster<<<(N + BLK / 64 - 1) / (BLK / 64), BLK, 0, st>>>(ls.ln, fl, N, gm.p);
    else k_gm_cluster_hv<<<grid_for((uint64_t)N * PSIM_ACTIVE_CAP), BLK, 0, st>>>(ls.ln, fl, N, gm.p);
    HIP_TRY(hipGetLastError());
    unsigned long long gv[GM_N];
    TRY(read_back(st, gv, gm.p, GM_N));
    out->n_up = gv[GM_NUP]; out->links = gv[GM_LINKS]; out->cl_nodes = gv[GM_NODES];
    out->cl_closed = gv[GM_CLOSED]; out->cl_pairs = gv[GM_PAIRS]; out->cl_sum_q32 = gv[GM_Q32];
    if (!ns) return PSIM_OK;
    // 3. the BFS, reach[] read once at its end
    const uint32_t cap = level_cap(max_levels);
    TmpBuf<uint32_t> dsrc;
    WordBfs b;
    TRY(dsrc.alloc_on(PSIM_GRAPH_SOURCES, st));
    TRY(b.seen.alloc_on(N, st)); TRY(b.front.alloc_on(N, st)); TRY(b.next.alloc_on(N, st));
    TRY(b.lv.alloc_on(2 * ((size_t)cap + 1), st)); TRY(b.reach.alloc_on(PSIM_GRAPH_SOURCES, st));
    HIP_TRY(hipMemcpyAsync(dsrc.p, src, sizeof src, hipMemcpyHostToDevice, st));
    k_gm_init<<<1, 64, 0, st>>>(dsrc.p, ns, fl, b.seen.p, b.front.p, b.lv.p);      // (lv[0]: the live slots)
    unsigned long long live = 0;
    TRY(read_back(st, &live, b.lv.p));
    out->sources_live = (uint64_t)__builtin_popcountll(live);
    if (!live) return PSIM_OK;
    const auto push = [&] { k_gm_push<<<grid_for(N), BLK, 0, st>>>(ls.ln, N, b.front.p, b.seen.p, b.next.p); };
    TRY(bfs_levels(st, N, cap, b, nullptr, out, push, [&](uint32_t d, const unsigned long long* w) {
        out->dist[d < PSIM_HIST_BINS ? d : PSIM_HIST_BINS - 1] += w[1];
        out->dist_sum += (uint64_t)d * w[1];
        out->pairs_reached += w[1];
        for (uint32_t j = 0; j < PSIM_GRAPH_SOURCES; j++)
            if ((w[0] >> j) & 1) out->ecc[j] = d;
    }));
    unsigned long long rv[PSIM_GRAPH_SOURCES];
    TRY(read_back(st, rv, b.reach.p, PSIM_GRAPH_SOURCES));
    for (uint32_t j = 0; j < PSIM_GRAPH_SOURCES; j++) out->reach[j] = rv[j];
    out->pairs_unreached = out->sources_live * (out->n_up - 1) - out->pairs_reached;
    return PSIM_OK;
}

extern "C" int psim_get_resilience(psim_handle* h, const psim_failure_case* cases, size_t n_cases, uint64_t fail_seed,
                                   uint32_t max_levels, psim_resilience* out) {
    static_assert(PSIM_FAIL_CASES == 64 && PSIM_FAIL_CASES == PSIM_GRAPH_SOURCES,
                  "one bit of k_gm_level's 64-bit word per case");
    if (!h || !out || (n_cases && !cases) || n_cases > PSIM_FAIL_CASES) return PSIM_EINVAL;
    const uint32_t nc = (uint32_t)n_cases;
    for (uint32_t j = 0; j < nc; j++)
        if (cases[j].reserved) return PSIM_EINVAL;
    const bool pl = h->cfg.manager == PSIM_MANAGER_PLUGGABLE;
    if (h->hosted || (pl && h->cfg.strategy == PSIM_STRATEGY_FULL)) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    if (h->round_open) return PSIM_ESTATE;
    const uint32_t N = h->N;
    for (uint32_t j = 0; j < nc; j++)
        if (cases[j].source >= N) return PSIM_ERANGE;
    // the case table: cases of one salt side by side (k_rs_alive)
    uint32_t ord[PSIM_FAIL_CASES], par[RS_PAR] = {0};
    for (uint32_t j = 0; j < nc; j++) ord[j] = j;
    std::stable_sort(ord, ord + nc, [&](uint32_t a, uint32_t b) { return cases[a].salt < cases[b].salt; });
    for (uint32_t q = 0; q < nc; q++) {
        const psim_failure_case& c = cases[ord[q]];
        par[RS_SRC + q] = c.source; par[RS_THR + q] = c.threshold; par[RS_SALT + q] = c.salt; par[RS_SLOT + q] = ord[q];
    }
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    // 1. the link set as rows, as psim_get_graph_metrics reads it
    LinkSet ls;
    TmpBuf<unsigned long long> rs, alive;
    TmpBuf<uint32_t> dpar;
    WordBfs b;
    TRY(link_set(h, st, fl, ls));
    // 2. the survivor words (they seed the BFS) and the census
    const uint32_t cap = level_cap(max_levels);
    TRY(rs.alloc_on(RS_N, st)); TRY(dpar.alloc_on(RS_PAR, st));
    TRY(alive.alloc_on(N, st)); TRY(b.seen.alloc_on(N, st)); TRY(b.front.alloc_on(N, st)); TRY(b.next.alloc_on(N, st));
    HIP_TRY(hipMemcpyAsync(dpar.p, par, sizeof par, hipMemcpyHostToDevice, st));
    k_rs_live<<<1, 64, 0, st>>>(dpar.p, nc, fl, rs.p);
    k_rs_alive<<<grid_for(N), BLK, 0, st>>>(dpar.p, nc, fail_seed, fl, N, rs.p, alive.p, b.seen.p, b.front.p);
    // (next: the in-link words until the BFS needs it zeroed again)
    k_rs_census<<<grid_for(N), BLK, 0, st>>>(ls.ln, fl, N, alive.p, b.next.p, rs.p);
    if (nc) k_rs_sweep<<<grid_for(N), BLK, 0, st>>>(N, alive.p, b.next.p, rs.p);
    HIP_TRY(hipGetLastError());
    unsigned long long rv[RS_N];
    TRY(read_back(st, rv, rs.p, RS_N));
    out->n_up = rv[RS_NUP]; out->links = rv[RS_L];
    const unsigned long long live = rv[RS_LIVE];
    out->live_mask = live; out->cases_live = (uint64_t)__builtin_popcountll(live);
    for (uint32_t j = 0; j < PSIM_FAIL_CASES; j++) {
        out->alive[j] = rv[RS_ALIVE + j]; out->links_alive[j] = rv[RS_LINKS + j];
        out->no_out[j] = rv[RS_NOOUT + j]; out->no_in[j] = rv[RS_NOIN + j];
    }
    if (!live) return PSIM_OK;
    // 3. the BFS of psim_get_graph_metrics over the seeded words: reach[]
    // comes back with each level's words, its growth times d is the hop sum
    TRY(b.lv.alloc_on(2 * ((size_t)cap + 1), st)); TRY(b.reach.alloc_on(PSIM_GRAPH_SOURCES, st));
    HIP_TRY(hipMemsetAsync(b.next.p, 0, (size_t)N * 8, st));
    unsigned long long prev[PSIM_FAIL_CASES] = {0}, cur[PSIM_FAIL_CASES] = {0};
    const auto push = [&] { k_gm_push<<<grid_for(N), BLK, 0, st>>>(ls.ln, N, b.front.p, b.seen.p, b.next.p); };
    return bfs_levels(st, N, cap, b, cur, out, push, case_levels(out, cur, prev));
}

extern "C" int psim_get_gossip_reach(psim_handle* h, const psim_gossip_case* cases, size_t n_cases, uint64_t fail_seed,
                                     uint32_t max_levels, psim_gossip_reach* out) {
    if (!h || !out || (n_cases && !cases) || n_cases > PSIM_FAIL_CASES) return PSIM_EINVAL;
    const uint32_t nc = (uint32_t)n_cases;
    const bool pl = h->cfg.manager == PSIM_MANAGER_PLUGGABLE;
    if (h->hosted || (pl && h->cfg.strategy == PSIM_STRATEGY_FULL)) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    if (h->round_open) return PSIM_ESTATE;
    const uint32_t N = h->N;
    for (uint32_t j = 0; j < nc; j++)
        if (cases[j].source >= N) return PSIM_ERANGE;
    // the case table: k_rs_alive's, and the fanouts in its order
    uint32_t ord[PSIM_FAIL_CASES], par[GO_PAR] = {0};
    for (uint32_t j = 0; j < nc; j++) ord[j] = j;
    std::stable_sort(ord, ord + nc, [&](uint32_t a, uint32_t b) { return cases[a].salt < cases[b].salt; });
    for (uint32_t q = 0; q < nc; q++) {
        const psim_gossip_case& c = cases[ord[q]];
        par[RS_SRC + q] = c.source; par[RS_THR + q] = c.threshold; par[RS_SALT + q] = c.salt; par[RS_SLOT + q] = ord[q];
        par[GO_FAN + q] = c.fanout;
    }
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    // 1. the link set as rows, as psim_get_resilience reads it
    LinkSet ls;
    TmpBuf<unsigned long long> rs, go, alive, sel;
    TmpBuf<uint32_t> dpar;
    WordBfs b;
    TRY(link_set(h, st, fl, ls));
    // 2. the survivor words (they seed the BFS) and the chosen links
    const uint32_t cap = level_cap(max_levels);
    TRY(rs.alloc_on(RS_N, st)); TRY(go.alloc_on(GO_N, st)); TRY(dpar.alloc_on(GO_PAR, st));
    TRY(alive.alloc_on(N, st)); TRY(b.seen.alloc_on(N, st)); TRY(b.front.alloc_on(N, st)); TRY(b.next.alloc_on(N, st));
    TRY(sel.alloc_on(nc ? ls.slots : 0, st));
    HIP_TRY(hipMemcpyAsync(dpar.p, par, sizeof par, hipMemcpyHostToDevice, st));
    k_rs_live<<<1, 64, 0, st>>>(dpar.p, nc, fl, rs.p);
    k_rs_alive<<<grid_for(N), BLK, 0, st>>>(dpar.p, nc, fail_seed, fl, N, rs.p, alive.p, b.seen.p, b.front.p);
    if (nc) {
        const unsigned long long all = nc == PSIM_FAIL_CASES ? ~0ull : (1ull << nc) - 1;
        uint32_t fmin = PSIM_NONE;
        for (uint32_t j = 0; j < nc; j++)
            if (cases[j].fanout) fmin = std::min(fmin, cases[j].fanout);
        k_go_select<<<grid_for(N), BLK, 0, st>>>(ls.ln, N, dpar.p, nc, fail_seed, all, fmin, sel.p);
        if (pl)
            k_go_select_long<<<grid_for((uint64_t)N * GO_LN), BLK, 0, st>>>(ls.ln, N, dpar.p, nc, fail_seed, all, fmin,
                                                                          sel.p);
    }
    HIP_TRY(hipGetLastError());
    unsigned long long rv[RS_N];
    TRY(read_back(st, rv, rs.p, RS_N));
    out->n_up = rv[RS_NUP];
    const unsigned long long live = rv[RS_LIVE];
    out->live_mask = live; out->cases_live = (uint64_t)__builtin_popcountll(live);
    // 3. the BFS of psim_get_resilience, pushed over the chosen links only
    if (live) {
        TRY(b.lv.alloc_on(2 * ((size_t)cap + 1), st)); TRY(b.reach.alloc_on(PSIM_GRAPH_SOURCES, st));
        unsigned long long prev[PSIM_FAIL_CASES] = {0}, cur[PSIM_FAIL_CASES] = {0};
        const auto push = [&] {
            k_go_push<<<grid_for(N), BLK, 0, st>>>(ls.ln, sel.p, N, b.front.p, b.seen.p, b.next.p);
        };
        TRY(bfs_levels(st, N, cap, b, cur, out, push, case_levels(out, cur, prev)));
    }
    // 4. the copies the senders pushed; with no live case only |L|
    k_go_tally<<<grid_for(N), BLK, 0, st>>>(ls.ln, sel.p, N, alive.p, b.seen.p, b.front.p, go.p);
    HIP_TRY(hipGetLastError());
    unsigned long long gv[GO_N];
    TRY(read_back(st, gv, go.p, GO_N));
    out->links = gv[GO_L];
    for (uint32_t j = 0; j < PSIM_FAIL_CASES; j++) {
        out->alive[j] = gv[GO_ALIVE + j]; out->sent[j] = gv[GO_SENT + j]; out->lost[j] = gv[GO_LOST + j];
    }
    return PSIM_OK;
}

// a single-source BFS from the live node `root` over the rows k_tm_bfs reads,
// a kernel per level, the level's count read back after each (zero ends it),
// at most `cap` levels.  depth: N words; lv: cap + 1 zeroed words; per[d]: the
// nodes first found at level d; levels, truncated: as psim_graph_metrics' are
static int tm_bfs(hipStream_t st, Links ln, uint32_t N, uint32_t root, uint32_t cap, uint32_t* depth,
                  unsigned long long* lv, std::vector<uint64_t>& per, uint64_t& levels, bool& truncated) {
    HIP_TRY(hipMemsetAsync(depth, 0xFF, (size_t)N * 4, st));
    HIP_TRY(hipMemsetAsync(depth + root, 0, 4, st));
    per.assign(1, 0);
    levels = 0;
    for (uint32_t d = 1; d <= cap; d++) {
        unsigned long long w = 0;
        k_tm_bfs<<<grid_for(N), BLK, 0, st>>>(ln, N, d, depth, lv + d);
        HIP_TRY(hipGetLastError());
        TRY(read_back(st, &w, lv + d));
        levels = d;
        if (!w) break;
        per.push_back(w);
        if (d == cap) truncated = true;
    }
    return PSIM_OK;
}

// PSIM_TREE_LANES=64: a wave a node in k_tm_rows, for A/B (DESIGN.md
// "Broadcast tree"); anything else: the 16-lane row
static uint32_t tm_lanes() {
    const char* e = getenv("PSIM_TREE_LANES");
    return e && atoi(e) == 64 ? 64u : 16u;
}

// A root's eager link set T (psim_tree_metrics defines it) as a CSR, the same
// on every rank, with what its row pass counts: tm (TM_N words, summed over
// ranks) and the in-degrees in T.  TreeSet owns the buffers
struct TreeSet {
    ShCsr csr;
    TmpBuf<unsigned long long> tm;
    TmpBuf<uint32_t> indeg;
};
static int tree_set(psim_handle* h, hipStream_t st, const uint8_t* fl, uint32_t root, TreeSet& t) {
    const uint32_t N = h->N, lanes = tm_lanes();
    ShCsr& csr = t.csr;
    TmpBuf<unsigned long long>& tm = t.tm;
    TmpBuf<uint32_t>& indeg = t.indeg;
    TRY(tm.alloc_on(TM_N, st)); TRY(indeg.alloc_on(N, st));
    TRY(csr_alloc(h, st, csr));
    const auto k_rows = lanes == 64 ? k_tm_rows<64> : k_tm_rows<16>;
    auto rows = [&](const uint32_t* off, uint32_t* adj) {
        for (Shard* s : h->shards) {
            if (!s->n) continue;
            const uint32_t grid = (uint32_t)(((uint64_t)s->n * lanes + BLK - 1) / BLK);
            k_rows<<<grid, BLK, 0, st>>>(s->hdr.p, s->act.p, s->pt_rt.p, s->pt_eag.p, s->pt_laz.p, s->pt_com.p, fl,
                                         s->lo, s->n, N, root, csr.cnt.p, off, adj, indeg.p, tm.p);
        }
    };
    rows(nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    uint32_t slot = 0;
    TRY(csr_place(h, st, csr, slot));
    rows(csr.off.p, csr.adj.p);
    HIP_TRY(hipGetLastError());
    TRY(csr_gather(h, st, csr, slot));
    if (h->ranked) {
        TRY(h->comm->all_reduce(tm.p, TM_N, CType::U64, COp::SUM, st));
        TRY(h->comm->all_reduce(indeg.p, N, CType::U32, COp::SUM, st));
    }
    return PSIM_OK;
}

extern "C" int psim_get_tree_metrics(psim_handle* h, uint32_t root, uint32_t max_levels, psim_tree_metrics* out) {
    if (!h || !out) return PSIM_EINVAL;
    if (h->cfg.manager == PSIM_MANAGER_PLUGGABLE || h->hosted || !h->cfg.plumtree)
        return PSIM_EUNSUPPORTED;                // (hosted: a collective)
    if (h->round_open) return PSIM_ESTATE;
    if (root >= h->N) return PSIM_ERANGE;
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    const uint32_t N = h->N;
    // 1. T as a CSR, the same on every rank, and the entry-level counts
    TreeSet ts;
    TmpBuf<unsigned long long> tf, sym;
    TRY(tf.alloc_on(TF_N, st)); TRY(sym.alloc_on(1, st));
    TRY(tree_set(h, st, fl, root, ts));
    const ShCsr& csr = ts.csr;
    const TmpBuf<unsigned long long>& tm = ts.tm;
    const TmpBuf<uint32_t>& indeg = ts.indeg;
    const Links tree = csr.links();
    k_tm_sym<<<grid_for(N), BLK, 0, st>>>(tree, N, sym.p);
    HIP_TRY(hipGetLastError());
    unsigned long long tv[TM_N], sv = 0;
    uint8_t rf = 0;
    HIP_TRY(hipMemcpyAsync(tv, tm.p, sizeof tv, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&sv, sym.p, 8, hipMemcpyDeviceToHost, st));
    TRY(read_back(st, &rf, fl + root));
    for (int k = 0; k < PSIM_HIST_BINS; k++) {
        out->eager_out[k] = tv[TM_EOUT * PSIM_HIST_BINS + k];
        out->lazy_out[k] = tv[TM_LOUT * PSIM_HIST_BINS + k];
    }
    out->n_up = tv[TM_NUP]; out->slot_nodes = tv[TM_SLOT];
    out->eager_entries = tv[TM_EENT]; out->lazy_entries = tv[TM_LENT];
    out->eager_links = tv[TM_ELINKS]; out->lazy_links = tv[TM_LLINKS]; out->both_links = tv[TM_BOTH];
    out->eager_both_forms = tv[TM_FORMS]; out->self_entries = tv[TM_SELF];
    out->eager_dead = tv[TM_EDEAD]; out->lazy_dead = tv[TM_LDEAD];
    out->eager_nonmember = tv[TM_ENM]; out->lazy_nonmember = tv[TM_LNM];
    out->eager_symmetric = sv;
    out->root_live = (rf & F_UP) ? 1 : 0;
    // 2. the two BFS passes from a live root: over T, then over the overlay's
    // L (as psim_get_graph_metrics reads it)
    TmpBuf<uint32_t> dt, dl;
    LinkSet ls;
    TmpBuf<unsigned long long> lv;
    if (out->root_live) {
        const uint32_t cap = level_cap(max_levels);
        std::vector<uint64_t> per;
        uint64_t levels = 0;
        bool trunc = false;
        TRY(dt.alloc_on(N, st)); TRY(dl.alloc_on(N, st)); TRY(lv.alloc_on(2 * ((size_t)cap + 1), st));
        TRY(tm_bfs(st, tree, N, root, cap, dt.p, lv.p, per, levels, trunc));
        out->levels = levels;
        for (uint32_t d = 1; d < per.size(); d++) {
            out->depth[d < PSIM_HIST_BINS ? d : PSIM_HIST_BINS - 1] += per[d];
            out->depth_sum += (uint64_t)d * per[d];
            out->reached += per[d];
            out->depth_max = d;
        }
        TRY(link_set(h, st, fl, ls));
        TRY(tm_bfs(st, ls.ln, N, root, cap, dl.p, lv.p + cap + 1, per, levels, trunc));
        out->truncated = trunc ? 1 : 0;
        out->unreached = out->n_up - 1 - out->reached;
    }
    // 3. per node: the in-degree histogram, the two depths side by side
    k_tm_final<<<grid_for(N), BLK, 0, st>>>(indeg.p, tree.cnt, fl, N, root, dt.p, dl.p, tf.p);
    HIP_TRY(hipGetLastError());
    unsigned long long fv[TF_N];
    TRY(read_back(st, fv, tf.p, TF_N));
    for (int k = 0; k < PSIM_HIST_BINS; k++) out->eager_in[k] = fv[k];
    out->links_from_reached = fv[TF_LFR]; out->overlay_reached = fv[TF_OREACH]; out->both_reached = fv[TF_BOTH];
    out->depth_sum_both = fv[TF_DSUM]; out->dist_sum_both = fv[TF_LSUM];
    out->deeper = fv[TF_DEEPER]; out->shallower = fv[TF_SHALLOWER];
    return PSIM_OK;
}

// PSIM_RELAY_LANES=8: an 8-lane group an entry in k_rl_expand, for A/B
// (DESIGN.md "Transitive unicast": 2.4 times the kernel time of the default);
// anything else: a lane an entry
static uint32_t rl_lanes() {
    const char* e = getenv("PSIM_RELAY_LANES");
    return e && atoi(e) == (int)RL_ROW ? RL_ROW : 1u;
}
// the merge table's first size, a power of two (PSIM_RELAY_SLOTS, a test
// hook: a small one makes a small run wrap its probes and regrow)
static uint64_t rl_slots() {
    const char* e = getenv("PSIM_RELAY_SLOTS");
    const uint64_t want = e ? strtoull(e, nullptr, 10) : 0;
    uint64_t s = 16;
    while (s < (want ? std::min<uint64_t>(want, 1ull << 30) : 1ull << 16)) s <<= 1;
    return s;
}

// The rows k_rl_census and k_rl_expand read: one shard's in place; virtual
// shards and ranks gather them by global id as gather_active_rows does (100 B
// a node), and every process then runs the same kernels over the whole overlay
struct RlGather { TmpBuf<uint32_t> act, com, conn, cnt; };
static int rl_rows(psim_handle* h, hipStream_t st, RlGather& b, RlRows& R) {
    if (!h->ranked && h->shards.size() == 1) {
        Shard* s = h->shards[0];
        R = RlRows{s->hdr.p, nullptr, s->act.p, s->pt_com.p, s->conn.p};
        return PSIM_OK;
    }
    const uint32_t per = h->per;
    const size_t npad = (size_t)per * h->G;
    TRY(b.act.alloc_on(npad * RL_ROW, st)); TRY(b.com.alloc_on(npad * RL_ROW, st));
    TRY(b.conn.alloc_on(npad * RL_ROW, st)); TRY(b.cnt.alloc_on(npad, st));
    for (Shard* s : h->shards)
        if (s->n)
            k_rl_pack<<<grid_for(s->n), BLK, 0, st>>>(s->hdr.p, s->act.p, s->pt_com.p, s->conn.p, s->n,
                                                      b.act.p + (size_t)s->lo * RL_ROW, b.com.p + (size_t)s->lo * RL_ROW,
                                                      b.conn.p + (size_t)s->lo * RL_ROW, b.cnt.p + s->lo);
    HIP_TRY(hipGetLastError());
    if (h->ranked) {
        const size_t off = (size_t)h->rank * per;
        TRY(h->comm->all_gather(b.act.p + off * RL_ROW, b.act.p, (size_t)per * RL_ROW * 4, st));
        TRY(h->comm->all_gather(b.com.p + off * RL_ROW, b.com.p, (size_t)per * RL_ROW * 4, st));
        TRY(h->comm->all_gather(b.conn.p + off * RL_ROW, b.conn.p, (size_t)per * RL_ROW * 4, st));
        TRY(h->comm->all_gather(b.cnt.p + off, b.cnt.p, (size_t)per * 4, st));
    }
    R = RlRows{nullptr, b.cnt.p, b.act.p, b.com.p, b.conn.p};
    return PSIM_OK;
}

extern "C" int psim_get_relay_reach(psim_handle* h, const psim_relay_case* cases, size_t n_cases, uint32_t max_levels,
                                    psim_relay_reach* out) {
    if (!h || !out || (n_cases && !cases) || n_cases > PSIM_RELAY_CASES) return PSIM_EINVAL;
    const uint32_t nc = (uint32_t)n_cases;
    for (uint32_t j = 0; j < nc; j++)
        if (cases[j].reserved || !cases[j].ttl || cases[j].ttl > PSIM_RELAY_MAX_TTL || cases[j].source == cases[j].target)
            return PSIM_EINVAL;
    if (h->cfg.manager != PSIM_MANAGER_HYPARVIEW || h->hosted || !h->cfg.plumtree)
        return PSIM_EUNSUPPORTED;                // (hosted: a collective)
    if (h->round_open) return PSIM_ESTATE;
    const uint32_t N = h->N;
    for (uint32_t j = 0; j < nc; j++)
        if (cases[j].source >= N || cases[j].target >= N) return PSIM_ERANGE;
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    // 1. the rows, and the census over them
    RlGather gb;
    RlRows R;
    TmpBuf<unsigned long long> cs, tl, rv;
    TRY(rl_rows(h, st, gb, R));
    TRY(cs.alloc_on(RC_N, st));
    k_rl_census<<<grid_for((uint64_t)N * 16), BLK, 0, st>>>(R, fl, N, cs.p);
    HIP_TRY(hipGetLastError());
    unsigned long long cv[RC_N];
    TRY(read_back(st, cv, cs.p, RC_N));
    out->n_up = cv[RC_NUP]; out->out_entries = cv[RC_ENT]; out->out_usable = cv[RC_USE];
    out->out_nonmember = cv[RC_NONMEM]; out->members_down = cv[RC_DOWN];
    for (int k = 0; k < PSIM_HIST_BINS; k++) out->out_degree[k] = cv[RC_DEG + k];
    if (!nc) return PSIM_OK;
    // 2. the flood, a level at a time: expand, merge by key, compact
    const uint32_t cap = !max_levels || max_levels > PSIM_RELAY_MAX_TTL ? PSIM_RELAY_MAX_TTL : max_levels;
    const uint32_t lanes = rl_lanes();
    const auto expand = lanes == 1 ? k_rl_expand<1> : k_rl_expand<RL_ROW>;
    TmpBuf<unsigned long long> fkey, fcnt, ckey, ccnt, tkey, tcnt;
    TmpBuf<uint32_t> dpar;
    uint32_t par[RP_N] = {0};
    unsigned long long k0[PSIM_RELAY_CASES], c0[PSIM_RELAY_CASES];
    for (uint32_t j = 0; j < nc; j++) {
        par[RP_DST + j] = cases[j].target; par[RP_TTL + j] = cases[j].ttl;
        k0[j] = ((unsigned long long)j << 32) | ((unsigned long long)cases[j].ttl << KEY_DST_BITS) | cases[j].source;
        c0[j] = 1;
    }
    TRY(tl.alloc_on(RF_N, st)); TRY(rv.alloc_on(RV_N, st)); TRY(dpar.alloc_on(RP_N, st));
    TRY(fkey.ensure(nc)); TRY(fcnt.ensure(nc));
    HIP_TRY(hipMemsetAsync(tl.p + RF_FIRST * PSIM_RELAY_CASES, 0xFF, PSIM_RELAY_CASES * 8, st));
    HIP_TRY(hipMemcpyAsync(dpar.p, par, sizeof par, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(fkey.p, k0, nc * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(fcnt.p, c0, nc * 8, hipMemcpyHostToDevice, st));
    uint64_t nf = nc, slots = rl_slots();
    for (uint32_t lvl = 0; nf && lvl <= cap; lvl++) {
        if (nf > (1ull << 31)) return PSIM_ENOMEM;   // (the children of more entries: past any device's memory)
        TRY(ckey.ensure(nf * RL_ROW)); TRY(ccnt.ensure(nf * RL_ROW));
        HIP_TRY(hipMemsetAsync(rv.p, 0, RV_N * 8, st));
        expand<<<grid_for(nf * lanes), BLK, 0, st>>>(R, fl, N, dpar.p, fkey.p, fcnt.p, nf, lvl, ckey.p, ccnt.p, rv.p, tl.p);
        HIP_TRY(hipGetLastError());
        unsigned long long m = 0;
        TRY(read_back(st, &m, rv.p + RV_CHILD));
        if (!m) break;
        while (slots < 2 * m) slots <<= 1;
        TRY(tkey.ensure(slots)); TRY(tcnt.ensure(slots)); TRY(fkey.ensure(m)); TRY(fcnt.ensure(m));
        HIP_TRY(hipMemsetAsync(tkey.p, 0xFF, slots * 8, st));
        HIP_TRY(hipMemsetAsync(tcnt.p, 0, slots * 8, st));
        k_rl_merge<<<grid_for(m), BLK, 0, st>>>(ckey.p, ccnt.p, m, tkey.p, tcnt.p, slots - 1);
        k_rl_compact<<<grid_for(slots), BLK, 0, st>>>(tkey.p, tcnt.p, slots, fkey.p, fcnt.p, rv.p);
        HIP_TRY(hipGetLastError());
        unsigned long long lv[RV_N];
        TRY(read_back(st, lv, rv.p, RV_N));
        nf = lv[RV_NEXT];
        for (uint32_t j = 0; j < PSIM_RELAY_CASES; j++) {
            if (!lv[RV_DISTINCT + j]) continue;
            if (lvl + 1 <= cap) {
                out->levels[j] = lvl + 1;
                out->peak[j] = std::max<uint64_t>(out->peak[j], lv[RV_DISTINCT + j]);
                out->levels_max = std::max<uint64_t>(out->levels_max, lvl + 1);
            } else {
                out->truncated_mask |= 1ull << j;
                out->in_flight[j] = lv[RV_SUM + j];
            }
        }
    }
    unsigned long long tv[RF_N];
    TRY(read_back(st, tv, tl.p, RF_N));
    out->live_mask = tv[RF_LIVE]; out->direct_mask = tv[RF_DIRECT];
    out->cases_live = (uint64_t)__builtin_popcountll(tv[RF_LIVE]);
    for (uint32_t j = 0; j < PSIM_RELAY_CASES; j++) {
        out->delivered[j] = tv[RF_DELIV * PSIM_RELAY_CASES + j]; out->hop_sum[j] = tv[RF_HOPS * PSIM_RELAY_CASES + j];
        out->relays[j] = tv[RF_RELAY * PSIM_RELAY_CASES + j]; out->refused[j] = tv[RF_REFUSED * PSIM_RELAY_CASES + j];
        out->expired[j] = tv[RF_EXPIRED * PSIM_RELAY_CASES + j]; out->restarts[j] = tv[RF_RESTART * PSIM_RELAY_CASES + j];
        const unsigned long long f = tv[RF_FIRST * PSIM_RELAY_CASES + j];
        out->first_hop[j] = f == RL_EMPTY ? 0 : f;
    }
    return PSIM_OK;
}

// PSIM_LAT_PUSH=list: k_lt_push_list over the compacted frontier, and
// PSIM_LAT_CELL=cell: the cell array instead of xbot_latency per link, for A/B
// (DESIGN.md "Latency-weighted paths": both measured slower); anything else:
// the walk over all nodes, the weights per link
static bool lt_env(const char* name, const char* value) {
    const char* e = getenv(name);
    return e && !strcmp(e, value);
}

// The rows and frontier words of the sweeps, allocated once a call and seeded
// again for every pass
struct LatRows {
    TmpBuf<uint32_t> cur, prev, list, dsrc;
    TmpBuf<unsigned long long> front, next, lv;
    uint32_t cap = 0;
    bool use_list = false;
};
static int lt_alloc(hipStream_t st, uint32_t N, uint32_t cap, LatRows& b) {
    b.cap = cap;
    b.use_list = lt_env("PSIM_LAT_PUSH", "list");
    TRY(b.cur.ensure((size_t)N * LT_W, -1)); TRY(b.prev.ensure((size_t)N * LT_W, -1));
    TRY(b.list.ensure(std::max<size_t>(N, LT_W), -1)); TRY(b.dsrc.ensure(LT_W, -1));
    TRY(b.front.ensure(N, -1)); TRY(b.next.ensure(N, -1)); TRY(b.lv.ensure(2 * ((size_t)cap + 1), -1));
    return PSIM_OK;
}

// The sweeps from the live nodes among src[0 .. ns) over `ln`: on return
// b.cur holds D_R.  live: the mask of live slots; sweeps: R; trunc: the word
// of sweep `cap` if that still lowered a distance; last[j] (nullptr: not
// wanted): the last sweep that lowered one of slot j; front_sum: the frontier
// nodes over all sweeps
static int lt_run(hipStream_t st, Links ln, uint32_t N, const uint8_t* fl, const uint32_t* cell, uint64_t seed,
                  LatRows& b, const uint32_t* src, uint32_t ns, uint64_t& live, uint64_t& sweeps, uint64_t& trunc,
                  uint64_t* last) {
    uint32_t s64[LT_W];
    for (uint32_t j = 0; j < LT_W; j++) s64[j] = j < ns ? src[j] : PSIM_NONE;
    live = sweeps = trunc = 0;
    HIP_TRY(hipMemsetAsync(b.cur.p, 0xFF, (size_t)N * LT_W * 4, st));
    HIP_TRY(hipMemsetAsync(b.prev.p, 0xFF, (size_t)N * LT_W * 4, st));
    HIP_TRY(hipMemsetAsync(b.front.p, 0, (size_t)N * 8, st));
    HIP_TRY(hipMemsetAsync(b.next.p, 0, (size_t)N * 8, st));
    HIP_TRY(hipMemsetAsync(b.lv.p, 0, 2 * ((size_t)b.cap + 1) * 8, st));
    HIP_TRY(hipMemcpyAsync(b.dsrc.p, s64, sizeof s64, hipMemcpyHostToDevice, st));
    k_lt_init<<<1, 64, 0, st>>>(b.dsrc.p, ns, fl, b.cur.p, b.prev.p, b.front.p, b.list.p, b.lv.p);
    HIP_TRY(hipGetLastError());
    unsigned long long w[2] = {0, 0};
    TRY(read_back(st, w, b.lv.p, 2));
    live = w[0];
    uint64_t nf = w[1];
    if (!live) return PSIM_OK;
    constexpr uint32_t WPB = BLK / 64;                // waves a block
    for (uint32_t d = 1; d <= b.cap; d++) {
        unsigned long long* lv = b.lv.p + 2 * (size_t)d;
        if (b.use_list)
            k_lt_push_list<<<(uint32_t)((nf + WPB - 1) / WPB), BLK, 0, st>>>(ln, b.list.p, (uint32_t)nf, cell, seed,
                                                                             b.front.p, b.prev.p, b.cur.p, b.next.p);
        else
            k_lt_push<<<grid_for(N), BLK, 0, st>>>(ln, N, cell, seed, b.front.p, b.prev.p, b.cur.p, b.next.p);
        k_lt_level<<<grid_for(N), BLK, 0, st>>>(N, b.next.p, b.front.p, b.cur.p, b.prev.p,
                                                b.use_list ? b.list.p : nullptr, lv);
        HIP_TRY(hipGetLastError());
        TRY(read_back(st, w, lv, 2));
        sweeps = d;
        if (!w[0]) break;
        nf = w[1];
        if (last)
            for (uint32_t j = 0; j < LT_W; j++)
                if ((w[0] >> j) & 1) last[j] = d;
        if (d == b.cap) trunc = w[0];
    }
    return PSIM_OK;
}

// the link costs of `ln` (L or T) into lc, LC_N words
static int lt_census(hipStream_t st, Links ln, uint32_t N, const uint8_t* fl, const uint32_t* cell, uint64_t seed,
                     unsigned long long* lc, unsigned long long* v) {
    HIP_TRY(hipMemsetAsync(lc, 0, LC_N * 8, st));
    k_lt_census<<<grid_for(N), BLK, 0, st>>>(ln, fl, N, cell, seed, lc);
    HIP_TRY(hipGetLastError());
    return read_back(st, v, lc, LC_N);
}

extern "C" int psim_get_latency_metrics(psim_handle* h, const uint32_t* sources, size_t n_sources, uint32_t tree_root,
                                        uint32_t max_sweeps, psim_latency_metrics* out) {
    static_assert(PSIM_LAT_SOURCES == 64, "a lane of a wave and a bit of a frontier word per source slot");
    if (!h || !out || (n_sources && !sources) || n_sources > PSIM_LAT_SOURCES) return PSIM_EINVAL;
    const bool pl = h->cfg.manager == PSIM_MANAGER_PLUGGABLE, tree = tree_root != PSIM_NONE;
    if (h->hosted || (pl && h->cfg.strategy == PSIM_STRATEGY_FULL)) return PSIM_EUNSUPPORTED;   // (hosted: a collective)
    if (tree && (pl || !h->cfg.plumtree)) return PSIM_EUNSUPPORTED;
    if (h->round_open) return PSIM_ESTATE;
    const uint32_t N = h->N, ns = (uint32_t)n_sources;
    uint32_t src[PSIM_LAT_SOURCES] = {0};
    for (uint32_t j = 0; j < ns; j++) {
        if (sources[j] >= N) return PSIM_ERANGE;
        src[j] = sources[j];
    }
    if (tree && tree_root >= N) return PSIM_ERANGE;
    for (uint32_t j = 0; j < ns; j++)
        for (uint32_t q = 0; q < j; q++)
            if (src[q] == src[j]) return PSIM_EINVAL;
    hipStream_t st; const uint8_t* fl;
    TRY(getter_begin(h, out, sizeof *out, st, fl));
    const uint64_t seed = h->cfg.seed;
    // 1. L as rows, the link census
    LinkSet ls;
    TmpBuf<uint32_t> cell;
    TmpBuf<unsigned long long> lc;
    unsigned long long cv[LC_N];
    TRY(link_set(h, st, fl, ls));
    if (lt_env("PSIM_LAT_CELL", "cell")) {
        TRY(cell.ensure(N, -1));
        k_lt_cell<<<grid_for(N), BLK, 0, st>>>(seed, N, cell.p);
    }
    TRY(lc.alloc_on(LC_N, st));
    TRY(lt_census(st, ls.ln, N, fl, cell.p, seed, lc.p, cv));
    out->n_up = cv[LC_NUP]; out->links = cv[LC_LINKS]; out->link_cost_sum = cv[LC_COST];
    out->link_nodes = cv[LC_NODES]; out->worst_sum = cv[LC_WORST]; out->best_sum = cv[LC_BEST];
    for (int k = 0; k < PSIM_HIST_BINS; k++) out->link_cost[k] = cv[LC_HIST + k];
    uint8_t rf = 0;
    if (tree) TRY(read_back(st, &rf, fl + tree_root));
    out->tree_root_live = (rf & F_UP) ? 1 : 0;
    if (!ns && !out->tree_root_live) return PSIM_OK;
    // 2. the sweeps from the sources, and one pass over the rows
    const uint32_t cap = level_cap(max_sweeps);
    LatRows b;
    TRY(lt_alloc(st, N, cap, b));
    if (ns) {
        uint64_t live = 0;
        TRY(lt_run(st, ls.ln, N, fl, cell.p, seed, b, src, ns, live, out->sweeps, out->truncated_mask,
                   out->last_sweep));
        out->live_mask = live;
        out->sources_live = (uint64_t)__builtin_popcountll(live);
        if (live) {
            constexpr uint32_t PER_WAVE = 16;
            TmpBuf<unsigned long long> lf;
            unsigned long long fv[LF_N];
            TRY(lf.alloc_on(LF_N, st));
            k_lt_final<<<grid_for(((uint64_t)N + PER_WAVE - 1) / PER_WAVE * 64), BLK, 0, st>>>(b.cur.p, b.dsrc.p, fl, N,
                                                                                               PER_WAVE, lf.p);
            HIP_TRY(hipGetLastError());
            TRY(read_back(st, fv, lf.p, LF_N));
            for (uint32_t j = 0; j < PSIM_LAT_SOURCES; j++) {
                out->reach[j] = fv[LF_REACH + j]; out->lat_sum[j] = fv[LF_SUM + j]; out->lat_ecc[j] = fv[LF_ECC + j];
                out->pairs_reached += fv[LF_REACH + j]; out->lat_sum_all += fv[LF_SUM + j];
                out->lat_max = std::max<uint64_t>(out->lat_max, fv[LF_ECC + j]);
            }
            for (int k = 0; k < PSIM_HIST_BINS; k++) out->lat[k] = fv[LF_HIST + k];
            out->pairs_unreached = out->sources_live * (out->n_up - 1) - out->pairs_reached;
        }
    }
    if (!out->tree_root_live) return PSIM_OK;
    // 3. the tree half: T, its link costs, the one-slot sweeps over T and over L
    TreeSet ts;
    TmpBuf<uint32_t> dt, dl;
    TmpBuf<unsigned long long> lr;
    unsigned long long rv[LR_N];
    uint64_t live = 0, sweeps = 0, trunc_t = 0, trunc_l = 0;
    TRY(tree_set(h, st, fl, tree_root, ts));
    const Links T = ts.csr.links();
    TRY(lt_census(st, T, N, fl, cell.p, seed, lc.p, cv));
    out->tree_links = cv[LC_LINKS]; out->tree_link_cost_sum = cv[LC_COST];
    TRY(dt.ensure(N, -1)); TRY(dl.ensure(N, -1)); TRY(lr.alloc_on(LR_N, st));
    TRY(lt_run(st, T, N, fl, cell.p, seed, b, &tree_root, 1, live, out->tree_sweeps, trunc_t, nullptr));
    k_lt_column<<<grid_for(N), BLK, 0, st>>>(b.cur.p, N, dt.p);
    TRY(lt_run(st, ls.ln, N, fl, cell.p, seed, b, &tree_root, 1, live, sweeps, trunc_l, nullptr));
    k_lt_column<<<grid_for(N), BLK, 0, st>>>(b.cur.p, N, dl.p);
    k_lt_tree<<<grid_for(N), BLK, 0, st>>>(dt.p, dl.p, fl, N, tree_root, lr.p);
    HIP_TRY(hipGetLastError());
    TRY(read_back(st, rv, lr.p, LR_N));
    out->tree_reached = rv[LR_TREACH]; out->tree_lat_sum = rv[LR_TSUM]; out->tree_lat_max = rv[LR_TMAX];
    out->overlay_reached = rv[LR_OREACH]; out->both_reached = rv[LR_BOTH];
    out->tree_lat_sum_both = rv[LR_TSUMB]; out->overlay_lat_sum_both = rv[LR_OSUMB];
    out->slower = rv[LR_SLOWER]; out->faster = rv[LR_FASTER];
    out->tree_truncated = trunc_t || trunc_l ? 1 : 0;
    return PSIM_OK;
}
