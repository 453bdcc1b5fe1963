// psim_host.h -- what psim_engine.hip (the round) and psim_metrics.hip (the
// overlay getters) share of the host side: the error macros, device buffers,
// a shard's and a handle's state, and the device-wide exclusive prefix sum.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "psim_comm.h"
#include "psim_device.h"
#include "psim_kernels.h"

namespace psim {

constexpr int BLK = 256;
// blocks of the route's two passes over the sources (RB_MAX_BLOCKS at the
// most) by default: one resident generation (two 1024-thread blocks a CU) --
// 1024 blocks were two generations of latency-bound steps at 2^20 (step
// 0.619 -> 0.615 ms, profiles/r05/ab_log.txt r6n)
constexpr uint32_t RB_BLOCKS = 512;
#ifndef PSIM_RR_REG
#define PSIM_RR_REG 6
#endif
constexpr uint32_t RR_REG = PSIM_RR_REG;   // k_bucket_route: pairs a thread holds in registers

#define HIP_TRY(x)                                                       \
    do {                                                                 \
        hipError_t e_ = (x);                                             \
        if (e_ != hipSuccess) {                                          \
            std::fprintf(stderr, "psim: %s failed: %s (%s:%d)\n", #x,    \
                         hipGetErrorString(e_), __FILE__, __LINE__);     \
            return PSIM_EDEVICE;                                         \
        }                                                                \
    } while (0)

#define TRY(x)                   \
    do {                         \
        int rc_ = (x);           \
        if (rc_) return rc_;     \
    } while (0)

// a unit of the exchange's wire format (psim_engine.hip, above wire_long)
struct __attribute__((aligned(16))) Wire {
    uint4 q[2];
};
static_assert(sizeof(Wire) == 32, "a wire unit is half a record");

// ------------------------------------------------------------- buffers --
template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    // grow to the next power of two (per-round sizes peak on broadcast
    // rounds; a 25 % step re-allocated -- 1 ms each -- for many rounds),
    // contents not kept
    // headroom: grow to the power of two at or above want * (1 + headroom / 4);
    // headroom < 0: exactly want, rounded up to 64 MiB past 1 GiB (an
    // up-front reservation sized against the free device memory)
    int ensure(size_t want, int headroom = 0) {
        if (want <= n) return PSIM_OK;
        static const bool trace = getenv("PSIM_TRACE_GROW") != nullptr;
        if (trace && want >= (1u << 20))
            std::fprintf(stderr, "psim: grow %zu -> %zu (want) x %zu B\n", n, want, sizeof(T));
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        const size_t goal = want + want / 4 * (size_t)(headroom > 0 ? headroom : 0);
        size_t cap = 1024;
        while (cap < goal) cap <<= 1;
        // past 1 GiB a power of two (or the caller's headroom) may waste up
        // to half: 1/8 headroom in 64 MiB steps instead (at 2^26 nodes the
        // message buffers are tens of GB)
        if (headroom < 0) cap = want;
        if (cap * sizeof(T) > (1ull << 30)) {
            const size_t step = (64ull << 20) / sizeof(T);
            cap = (want + (headroom < 0 ? 0 : want / 8) + step - 1) / step * step;
        }
        if (hipMalloc(&p, cap * sizeof(T)) != hipSuccess) {
            size_t fr = 0, tot = 0;
            (void)hipGetLastError();
            if (hipMemGetInfo(&fr, &tot) == hipSuccess)
                std::fprintf(stderr, "psim: device allocation of %.2f GB failed (%.2f of %.2f GB free)\n",
                             cap * sizeof(T) / 1e9, fr / 1e9, tot / 1e9);
            p = nullptr;
            return PSIM_ENOMEM;
        }
        n = cap;
        return PSIM_OK;
    }
    // grow like ensure(), keeping the first `keep` elements (copied on `st`)
    int ensure_keep(size_t want, size_t keep, hipStream_t st) {
        if (want <= n) return PSIM_OK;
        if (!p || !keep) return ensure(want);
        DBuf<T> nb;
        TRY(nb.ensure(want));
        if (hipMemcpyAsync(nb.p, p, std::min(keep, n) * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            nb.release();
            return PSIM_EDEVICE;
        }
        release();
        p = nb.p; n = nb.n;
        return PSIM_OK;
    }
    int alloc(size_t want) {    // exact, zeroed
        static const bool trace = getenv("PSIM_TRACE_GROW") != nullptr;
        if (trace && want >= (1u << 20)) std::fprintf(stderr, "psim: alloc %zu x %zu B\n", want, sizeof(T));
        if (hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(T)) != hipSuccess) return PSIM_ENOMEM;
        n = want;
        if (hipMemset(p, 0, std::max<size_t>(want, 1) * sizeof(T)) != hipSuccess) return PSIM_EDEVICE;
        return PSIM_OK;
    }
    // exact, zeroed on `st` (ordered before the stream's later kernels; the
    // null-stream fill of alloc() is not ordered with a non-blocking stream)
    int alloc_on(size_t want, hipStream_t st) {
        if (hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(T)) != hipSuccess) return PSIM_ENOMEM;
        n = want;
        if (hipMemsetAsync(p, 0, std::max<size_t>(want, 1) * sizeof(T), st) != hipSuccess) return PSIM_EDEVICE;
        return PSIM_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// a temporary device buffer, released on every return path
template <typename T>
struct TmpBuf : DBuf<T> {
    TmpBuf() = default;
    TmpBuf(const TmpBuf&) = delete;
    TmpBuf& operator=(const TmpBuf&) = delete;
    ~TmpBuf() { this->release(); }
};

enum Kern { KT_EVENTS, KT_PREPARE, KT_CONSUME, KT_SCAN, KT_COMPACT, KT_SORT, KT_EXCHANGE, KT_GATHER,
            KT_STATS, KT_HOST_EXPORT, KT_HOST_IMPORT, KT_PACK, KT_TRACE_COUNT, KT_TRACE_COPY, KT_N };

inline uint32_t grid_for(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, (n + BLK - 1) / BLK); }

struct Shard {
    uint32_t idx = 0, lo = 0, n = 0;    // global shard index, owned [lo, lo + n)
    hipStream_t stream = nullptr;
    // replicated (global id)
    DBuf<uint8_t> flags, part;
    DBuf<upart_t> upart;                // k_node_prep's up-and-partition pairs (RoundArgs::upart)
    DBuf<uint16_t> lite_cm;             // k_relay's connection bits and emitted counts of lite-list nodes (RoundArgs::lite_cm)
    DBuf<uint32_t> crash_bits;   // RoundArgs::crash_bits
    DBuf<uint8_t> btab;          // RoundArgs::btab (psim_set_bucket_table), global id
    // local rows
    DBuf<Hdr> hdr;
    DBuf<uint32_t> act, pas, pt_all, pt_com, pt_eag, pt_laz, pt_rt, start;
    DBuf<uint64_t> sentm, recvm, mapx;  // id maps (id << 32 | peer): own rows, extension rows (pool)
    DBuf<uint32_t> mapx_top;
    DBuf<uint32_t> origin;              // per local node: msg id + 1 it originates this round
    DBuf<uint32_t> slots;               // the message slots (msg ids, then roots), a copy of the host's
    DBuf<uint32_t> bc_roots, bc_msgs;   // this round's broadcasts
    DBuf<uint64_t> pt_out, outx;        // outstanding: own rows, extension rows (pool)
    DBuf<uint32_t> conn;                // connection tables (PSIM_CONN_CAP per node; HyParView)
    DBuf<uint32_t> outx_top;
    // inbox of the next round: sorted (local dst | bound, record index) pairs
    DBuf<uint32_t> ikeys, ivals;
    uint32_t m_in = 0;
    DBuf<Msg> outbox;                   // this round's emissions (holes between node regions)
    // G > 1: the received records in the wire format, in source-shard order:
    // their heads, the long ones' tails, and per source its first head and
    // first tail (wseg, 2 (G + 1) words; its host copy until the next round)
    DBuf<Wire> recvh, recvt;
    DBuf<uint32_t> wseg;
    std::vector<uint32_t> wseg_host;
    // records by node run, in inbox order: read by this round's node-round
    // kernels, then (same stream) overwritten by the route with the next
    // round's -- one buffer, nothing reads a round's inbox after its consume
    DBuf<Msg> inbox;
    // per-round scratch
    DBuf<uint32_t> okey, ocnt, in_beg,
        d_nact, n_slow, n_pt, n_shuf, n_lite, n_ptl, rank, tmp, hist, hoff;
    DBuf<uint32_t> rtot, rbase;         // route: per bucket its record count, and its first pair
    DBuf<uint32_t> gcnt;                // fused route: per bucket its record count (k_bucket_fill's atomics)
    DBuf<unsigned long long> bmask;     // per local node: message slots of its BROADCAST records
    DBuf<uint2> pairs;                  // route: (destination in bucket | class, source index)
    DBuf<unsigned long long> cb;        // per local node: inbox count | bound sum << 32 (n + 1)
    DBuf<unsigned long long> btot;      // this round's outbox total (k_node_prep)
    DBuf<uint4> desc, desc_slow, desc_pt, desc_shuf, desc_lite, desc_ptl;   // work descriptors; those k_relay leaves to k_consume / k_pt / k_shuf
    DBuf<uint64_t> bound, pscan, obase, stat_part, stat_out, stat_tile, d_off;   // bound: packed (bound << 32 | work)
    DBuf<uint8_t> cub_tmp;              // the scan's tile totals
    DBuf<uint32_t> ev_ids, ev_contacts, stop_ids, n_stop;
    bool tomb_live = false;             // full: snapshots carry their remove rows
    DBuf<Wire> sendbuf;                 // G > 1: the outbox in the wire format, by owner (k_owner_part)
    // pluggable manager
    DBuf<uint32_t> sview, sinv, fbits, pay[2], pay_top;
    int pay_cur = 0;
    // full, G > 1 (the payload exchange): the (owner, slot) bitmap and its
    // popcount scan, the per-owner row counts (device, then host), the slot
    // of every row sent and the rows packed by owner, and the rows other
    // shards shipped for the next round's
    // records -- imp_rows of them in source-shard order, fw words each, 2 fw
    // once tomb_live
    DBuf<uint32_t> pbits, prank, plist, paysend, pay_imp;
    DBuf<uint64_t> pcnt_d;
    std::vector<uint64_t> pcnt;
    uint32_t pbw = 0, imp_rows = 0;
    DBuf<uint8_t> faulted;              // omission faults: generally omitting nodes (global id)
    DBuf<uint64_t> omit;                // ... sorted send-omission pairs, then receive-omission pairs
    // per destination shard: the send buffer's offsets (2 G + 1: heads of
    // each owner, tails of each owner, the end), heads and tails sent
    std::vector<uint64_t> soff, scnt, lcnt;
    uint32_t pper = BLK;               // k_node_prep / k_desc: nodes per block (a multiple of BLK)
    uint32_t pgrid = 0, cgrid = 0, rgrid = 0, tgrid = 0, sgrid = 0, lgrid = 0, qgrid = 0, egrid = 0;   // stats rows: prepare,
                                   // consume, relay, plumtree, shuffle-start, lite, Plumtree-lane blocks
    // pinned host words: NST stats and the consume span (stat_out), then the
    // outbox total and the routed record count: the round's two read-backs
    uint64_t* pin = nullptr;
    uint64_t* pin_dev = nullptr;        // the same words, as the kernels store them
    // phase timers: event pairs recorded on the stream and read back once per
    // round, after the round's final synchronisation (no sync per phase)
    static constexpr int MAXT = 32;
    hipEvent_t ev[MAXT][2];
    int tk[MAXT];
    int tn = 0;
    hipEvent_t wait_ev = nullptr;
    // the three HyParView kernels after k_relay take disjoint node lists and
    // run concurrently: k_shuf and k_consume on two side streams forked from
    // and joined back into `stream` (fork_ev, join_ev)
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, join_ev[2] = {nullptr, nullptr};
    bool ev_live = false;
    bool reserved = false;              // first-round capacity reservation done
    bool upart_valid = false;           // upart holds this state's pairs (RoundArgs::upart_dirty)
    uint64_t rcap = 0;                  // records the route's buffers hold (G == 1: checked on the device)
    // batches of rounds without host waits (run_batch): the abort word
    // (code, round) in device memory; while a batch is enqueued, k_desc
    // checks the outbox against desc_cap and the route flags its overflow
    // for round batch_round1 - 1; round j's stats go to pinned slot j + 1
    DBuf<uint32_t> ctl;
    uint64_t desc_cap = 0;
    uint32_t batch_round1 = 0;
    uint32_t stat_slot = 0;
    // a batch's route prepares the next round (RoutePrep, PSIM_PREP_FUSED):
    // prep_next = that round + 1 while its route is enqueued (0: no), and
    // prepared = the round being enqueued was prepared by the last route
    uint32_t prep_next = 0;
    bool prepared = false;
    bool outx_short = false;            // the outstanding pool failed to grow (reported once per shard)
    // the rank path's batches (run_batch_ranked): the fixed per-owner
    // capacities of the exchange (heads, tails; 0 = not known yet: no batch),
    // identical on every rank (set from all-reduced counts), and the next
    // batch's length (1 after an abort, doubling up to BATCH_MAX)
    uint32_t xcap_h = 0, xcap_t = 0;
    uint32_t xbatch = 1;
    uint64_t trace_tmax = 0, trace_mmax = 0;   // PSIM_TRACE_BOUND's high-water marks
    // the message trace (psim_trace_watch; none of it allocated on an unarmed
    // handle): the watch bitmap (global ids; none when every node is
    // watched), the kept records with their rounds, the shard's matches since
    // the last read (two words, swapped every captured round: tr_cur names
    // the current one; the first `capacity` of them are kept), and a round's
    // scratch (block counts, group ballots)
    DBuf<uint32_t> tr_bits, tr_round, tr_cnt;
    DBuf<Msg> tr_rec;
    DBuf<unsigned long long> tr_tot, tr_ballot;
    int tr_cur = 0;
};

// the events a handle holds for its next round (psim_handle's pend_* members)
struct PendingEvents {
    std::vector<uint32_t> crash, join, contact, lv_a, lv_t, b_root, b_msg;
    std::vector<uint8_t> join_mark, part;
    bool part_set = false, part_clear = false, faults_dirty = false;
};

}  // namespace psim

struct psim_handle {
    psim_config cfg;
    uint32_t N = 0, G = 1, per = 0;
    int device = 0;
    uint32_t consume_blocks = 1024;     // resident k_consume blocks on the device
    uint32_t pt_blocks = 1024;          // ... and k_pt blocks
    uint32_t lite_blocks = 1024;        // the cap of the lite kernel's grid
    // the lite list's kernel, chosen in psim_create: k_lite_quarter, four
    // nodes per wave (psim_lite.hip); PSIM_LITE_HALF=1 keeps k_lite_half
    // (two), PSIM_LITE_WAVE=1 the wave-per-node k_consume_lite (A/B)
    psim::LiteKernel lite = {};
    uint32_t ptl_blocks = 1024;         // ... and k_ptl blocks
    uint64_t round = 0;
    // a round failed half-way (psim_step returned an error from inside a
    // round or batch): the state is not a round boundary any more, so every
    // later psim_step answers PSIM_ESTATE instead of running on it
    bool failed = false;
    std::vector<psim::Shard*> shards;   // shards owned by this process
    int rank = 0, world = 1;
    // the rank path (one shard per rank, the owner partition, the exchange
    // and the collectives of psim_comm.h): world > 1, or a one-rank world
    // whose cfg.comm_id was given (the 1-GPU diagnostic of the RCCL path:
    // every collective, the self send/recv included, runs through the library)
    bool ranked = false;
    psim::Comm* comm = nullptr;         // ranked: RCCL (or the loopback test vehicle), psim_comm.h
    psim::DBuf<uint64_t> comm_cnt;      // RCCL: [send counts | recv counts]
    // a host-exchange handle (cfg.comm_id from psim_host_comm_id): one shard,
    // the range [lo, hi) of the id space; the host speaks for every other id.
    // G = 3 owner classes (below, owned, at or above), the shard is class 1;
    // a round is psim_round_emit .. psim_round_absorb (round_open between)
    bool hosted = false, round_open = false;
    std::vector<psim::Msg> host_out, host_in; // the open round's outbound records; the absorbed ones, sorted
    std::vector<uint32_t> host_wbase;   // k_host_import: the long records before each wave's
    psim::DBuf<psim::Msg> hx_rec;       // the dense records on the device (export, then import)
    psim::DBuf<uint32_t> hx_wbase;
    psim::PendingEvents open_ev;        // the events queued while the round is open (pending_swap)
    // the exchange since creation (psim_get_exchange_stats): records sent to
    // another shard, and their wire bytes (heads + tails)
    uint64_t x_records = 0, x_bytes = 0;
    // pending events
    std::vector<uint32_t> pend_crash, pend_join, pend_contact;
    std::vector<uint8_t> pend_join_mark;   // ids in pend_join (a node starts at most once per round)
    std::vector<uint32_t> pend_lv_a, pend_lv_t;     // leave/1 calls: actor, target
    std::vector<uint8_t> pend_part;
    bool pend_part_set = false, pend_part_clear = false;
    std::vector<uint32_t> pend_b_root, pend_b_msg;    // broadcasts of the next round, in call order
    uint32_t slot_tab[2 * PSIM_MSG_SLOTS];            // slot k: msg id [k], root [PSIM_MSG_SLOTS + k]
    uint32_t tracked_msg = PSIM_NONE;
    bool btab = false;                  // psim_set_bucket_table: the shards' btab rows are in use
    uint32_t btab_hash = 0;             // ... their FNV-1a | 1 (0 = the default table), in snapshots
    uint32_t fw = 0;                    // full strategy: words per member row (adds; removes beside)
    bool tomb = false;                  // full: an ORSet remove exists (leave/1): kernels read remove rows
    std::vector<uint8_t> started;       // full strategy: ids ever started (no restarts)
    // omission faults (pluggable): the next round's installed funs, edited by
    // psim_set_omission / psim_set_faulted and uploaded when changed; the
    // counts of the ones in force
    std::set<uint64_t> nx_omit_s, nx_omit_r;
    std::vector<uint8_t> nx_faulted;
    size_t nx_nfaulted = 0;
    bool faults_dirty = false;
    uint32_t faults = 0, n_omit_s = 0, n_omit_r = 0;
    double kt_ms[psim::KT_N] = {0};
    uint64_t kt_n[psim::KT_N] = {0};
    // per-phase event timers (PSIM_PHASE_TIMERS=1): each event pair puts a
    // ~10 us bubble between kernels, so by default only k_consume is timed,
    // from its in-kernel span (RoundArgs::ktime)
    bool phase_timers = false;
    // blocks of the route / owner-partition passes (RB_MAX_BLOCKS; a test
    // hook, PSIM_ROUTE_BLOCKS, lowers it so small runs take several steps per block)
    uint32_t rb_blocks = psim::RB_BLOCKS;
    uint32_t rr_reg = psim::RR_REG;     // k_bucket_route: pairs a thread may hold (PSIM_ROUTE_REG=0: the array path)
    // one shard's own outbox routed by the fused pass (k_bucket_fill) instead
    // of k_bucket_hist + k_bucket_offsets + k_bucket_scatter
    // (PSIM_ROUTE_FUSED=0: the four passes, for A/B; reroutes take them too)
    bool route_fused = true;
    // the message trace: a watch is armed (psim_step then runs single rounds
    // and captures after each), every node watched, PSIM_TRACE_* directions,
    // the type mask, records kept between two reads (per shard, and in all)
    bool trace_on = false, trace_all = false;
    uint32_t trace_dir = 0, trace_mask = 0;
    size_t trace_cap = 0;
};

namespace psim {

// the shard of this process that owns node `id`
inline Shard* owner_of(psim_handle* h, uint32_t id) {
    for (Shard* c : h->shards)
        if (id >= c->lo && id < c->lo + c->n) return c;
    return nullptr;
}

// ------------------------------------------------ exclusive prefix sum --
// Reduce-then-scan over tiles of SCAN_TILE elements (256 threads x 8
// consecutive elements each): tile totals, one block scans the totals, each
// tile scans itself from its total's prefix.  Three launches, the input read
// twice (at 2^20 nodes: 8 MB per read, a few microseconds); a count that
// fits one tile is one launch.
constexpr uint32_t SCAN_ITEMS = 8, SCAN_TILE = BLK * SCAN_ITEMS;

// exclusive scan of one value per thread across the block; returns the
// block total in *total (every thread)
template <typename T, uint32_t NT = BLK>
__device__ T block_excl(T v, T* total) {
    __shared__ T wsum[NT / 64];
    const uint32_t l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T x = v;                                          // inclusive scan within the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (l >= (uint32_t)d) x += y;
    }
    if (l == 63) wsum[wv] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < NT / 64; k++) {
        base += k < wv ? wsum[k] : T(0);
        tot += wsum[k];
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

template <typename T, typename TI>
__global__ void __launch_bounds__(BLK) k_scan_tiles(const TI* __restrict__ in, uint32_t n, T* __restrict__ sums) {
    const size_t b0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    T v = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_ITEMS; k++) v += b0 + k < n ? in[b0 + k] : T(0);
    T tot;
    (void)block_excl(v, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one block: exclusive scan of the nt tile totals in place -- each thread a
// contiguous run of ceil(nt / BLK) of them, one block scan of the run sums
// (a block scan per BLK chunk took 12.7 us for 4097 totals: 17 serial
// barrier pairs).  Up to SUMS_LDS totals go through LDS, loaded and stored
// coalesced (the runs read straight from memory were ceil(nt / BLK)
// dependent strided loads a thread: 8.6 us for 4097 totals)
constexpr uint32_t SUMS_LDS = 4096 + 2 * BLK;
template <typename T>
__global__ void __launch_bounds__(BLK) k_scan_sums(T* sums, uint32_t nt) {
    __shared__ T buf[SUMS_LDS];
    const bool lds = nt <= SUMS_LDS;                  // (uniform)
    T* p = lds ? buf : sums;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < nt; i += BLK) buf[i] = sums[i];
        __syncthreads();
    }
    const uint32_t per = (nt + BLK - 1) / BLK, i0 = threadIdx.x * per, i1 = min(nt, i0 + per);
    T v = 0;
    for (uint32_t i = i0; i < i1; i++) v += p[i];
    T tot;
    T run = block_excl(v, &tot);
    for (uint32_t i = i0; i < i1; i++) {
        const T x = p[i];
        p[i] = run;
        run += x;
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nt; i += BLK) sums[i] = buf[i];
    }
}

template <typename T, typename TI>
__global__ void __launch_bounds__(BLK) k_scan_apply(const TI* __restrict__ in, T* __restrict__ out, uint32_t n,
                                                   const T* __restrict__ sums) {
    const size_t b0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    T x[SCAN_ITEMS], v = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
        x[k] = b0 + k < n ? in[b0 + k] : T(0);
        v += x[k];
    }
    T tot;
    T run = block_excl(v, &tot) + (sums ? sums[blockIdx.x] : T(0));
#pragma unroll
    for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
        if (b0 + k < n) out[b0 + k] = run;
        run += x[k];
    }
}

// (TI: the input's type where it is narrower than the sums', e.g. byte counts)
template <typename T, typename TI>
int scan_excl(Shard* s, const TI* in, T* out, uint32_t n) {
    // (a single-pass decoupled look-back measured 1.5 % slower a step at
    // 2^20, profiles/r03/p25: its device-coherent status loads cost more than
    // the two launches it saves; removed in round 4)
    const uint32_t nt = (uint32_t)(((uint64_t)n + SCAN_TILE - 1) / SCAN_TILE);
    if (nt <= 1) {
        k_scan_apply<T, TI><<<1, BLK, 0, s->stream>>>(in, out, n, nullptr);
    } else {
        TRY(s->cub_tmp.ensure((size_t)nt * sizeof(T)));
        T* sums = reinterpret_cast<T*>(s->cub_tmp.p);
        k_scan_tiles<T, TI><<<nt, BLK, 0, s->stream>>>(in, n, sums);
        k_scan_sums<T><<<1, BLK, 0, s->stream>>>(sums, nt);
        k_scan_apply<T, TI><<<nt, BLK, 0, s->stream>>>(in, out, n, sums);
    }
    HIP_TRY(hipGetLastError());
    return PSIM_OK;
}

}  // namespace psim
