/*
 * partisan_gpu_sim.h -- C ABI of the MI355X overlay simulator.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json
 * `north_star`: partisan's HyParView membership manager and Plumtree
 * broadcast, simulated one BSP round at a time with all node state resident
 * in HBM.  The Erlang host keeps partisan's callback surfaces and drives this
 * library through a NIF shim (erlang/c_src/partisan_gpu_sim_nif.c); Python
 * drives it through ctypes (partisan_amd/_lib.py).
 *
 * Each entry point replaces one reference interface (cited as file:line under
 * /root/reference, read-only):
 *
 *   psim_create / psim_destroy
 *       partisan_hyparview_peer_service_manager:init/1          (:289-354)
 *       partisan_plumtree_broadcast:init/1                      (:251-264)
 *       config keys of partisan_config:init/0                   (partisan_config.erl:102-145)
 *   psim_join
 *       partisan_peer_service:join/1 -> hyparview join/1,
 *       handle_cast({join, Peer})                               (hyparview:225-226, :500-515)
 *   psim_crash
 *       connection death -> handle_info({'EXIT', ...})          (hyparview:609-654)
 *   psim_revive
 *       a restarted manager: init/1 without a join              (hyparview:289-354)
 *   psim_leave
 *       leave/0 under the pluggable manager                     (pluggable:283-284, :502-515)
 *   psim_set_partition / psim_clear_partition
 *       inject_partition/2, resolve_partition/1                 (hyparview:244-250, :1731-1797)
 *       (modelled as a network partition)
 *   psim_broadcast
 *       partisan_plumtree_broadcast:broadcast/2 with the default
 *       partisan_plumtree_backend handler, any number of roots  (plumtree:176-178, backend:179-200)
 *   psim_step
 *       one BSP round of every node's timers and inbox:
 *       hyparview handle_message/2 (:693-1166), handle_info timers (:542-607),
 *       plumtree handle_cast/2 (:282-336), lazy_tick (:341-345)
 *   psim_set_bucket_table
 *       the sets v1 order of every view: sets:to_list/1 yields bucket
 *       erlang:phash(NodeSpec, 16) 1..16, oldest first   (hyparview:1230-1231, :1346-1361)
 *   psim_get_nodes
 *       debug getters active/0, passive/0 (hyparview:261-281),
 *       plumtree debug_get_peers/2,3 (:222-231), broadcast_members/0 (:188-195)
 *
 * With cfg.manager = PSIM_MANAGER_PLUGGABLE a handle simulates
 * partisan_pluggable_peer_service_manager driving one membership strategy
 * (partisan_membership_strategy.erl:32-36) instead:
 *   psim_join    internal_join/3 + the hello/state handshake + Strategy:join/3
 *                (pluggable:1423-1458, :986-1044; server:125-148)
 *   psim_step    Strategy:handle_message/2 per inbox message (pluggable:1153-1195)
 *                and Strategy:periodic/1 (pluggable:881-903)
 *   psim_get_strategy_nodes / psim_get_member_bits
 *                get_local_state/0 (pluggable:625-626), members/0 (:618-620)
 *
 * Conventions: every function returns 0 on success or a negative PSIM_E*
 * code; psim_strerror() names it.  No exceptions or aborts cross the ABI.
 * A handle is thread-compatible (not thread-safe): the NIF shim serialises
 * calls per handle and runs psim_step on a dirty CPU scheduler.
 * The library owns all device memory; the caller owns every host buffer.
 */
#ifndef PARTISAN_GPU_SIM_H
#define PARTISAN_GPU_SIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSIM_ABI_VERSION 12

/* error codes */
#define PSIM_OK 0
#define PSIM_EINVAL -1      /* bad argument / config                 */
#define PSIM_ENOMEM -2      /* device or host allocation failed       */
#define PSIM_EDEVICE -3     /* HIP runtime error                      */
#define PSIM_ESTATE -4      /* call not valid in the current state    */
#define PSIM_ERANGE -5      /* node id out of range                   */
#define PSIM_ECOMM -6       /* RCCL / transport error                 */
#define PSIM_EUNSUPPORTED -7
#define PSIM_ECAPACITY -8   /* cfg.strict: a fixed table overflowed this round */

/* message types (the record `type` field; also stats indices) */
enum psim_msg_type {
    PSIM_MSG_JOIN = 0,              /* {join, Peer, Tag, Epoch}                  hyparview:703  */
    PSIM_MSG_FORWARD_JOIN = 1,      /* {forward_join, Peer, Tag, Epoch, TTL, S}  hyparview:808  */
    PSIM_MSG_NEIGHBOR = 2,          /* {neighbor, Peer, Tag, DisconnectId, _}    hyparview:774  */
    PSIM_MSG_DISCONNECT = 3,        /* {disconnect, Peer, DisconnectId}          hyparview:926  */
    PSIM_MSG_NEIGHBOR_REQUEST = 4,  /* {neighbor_request, Peer, high, ...}       hyparview:975  */
    PSIM_MSG_NEIGHBOR_ACCEPTED = 5, /* {neighbor_accepted, Peer, Tag, Id, Ex}    hyparview:1070 */
    PSIM_MSG_NEIGHBOR_REJECTED = 6, /* {neighbor_rejected, Peer, Ex}             hyparview:1056 */
    PSIM_MSG_SHUFFLE = 7,           /* {shuffle, Exchange, TTL, Sender}          hyparview:1095 */
    PSIM_MSG_SHUFFLE_REPLY = 8,     /* {shuffle_reply, Exchange, Sender}         hyparview:1091 */
    PSIM_MSG_PT_BROADCAST = 9,      /* {broadcast, Id, M, Mod, Round, Root, From} plumtree:288 */
    PSIM_MSG_PT_PRUNE = 10,         /* {prune, Root, From}                       plumtree:294  */
    PSIM_MSG_PT_IHAVE = 11,         /* {i_have, Id, Mod, Round, Root, From}      plumtree:299  */
    PSIM_MSG_PT_IGNORED_IHAVE = 12, /* {ignored_i_have, ...}                     plumtree:304  */
    PSIM_MSG_PT_GRAFT = 13,         /* {graft, Id, Mod, Round, Root, From}       plumtree:308  */
    /* X-BOT (cfg.manager = PSIM_MANAGER_XBOT): the record carries
     * a0 = OldNode, a1 = InitiatorNode, a2 = CandidateNode, word 7 (a3) =
     * DisconnectNode (PSIM_NONE = undefined), ttl = the reply's answer (1 true,
     * 0 false); xbot = src/partisan_hyparview_xbot_peer_service_manager.erl */
    PSIM_MSG_XBOT_OPTIMIZATION = 16,       /* {optimization, _, Old, I, C, undefined}       xbot:1205 */
    PSIM_MSG_XBOT_OPTIMIZATION_REPLY = 17, /* {optimization_reply, Ans, Old, I, C, D}       xbot:1171 */
    PSIM_MSG_XBOT_REPLACE = 18,            /* {replace, _, Old, I, C, D}                    xbot:1252 */
    PSIM_MSG_XBOT_REPLACE_REPLY = 19,      /* {replace_reply, Ans, Old, I, C, D}            xbot:1227 */
    PSIM_MSG_XBOT_SWITCH = 20,             /* {switch, _, Old, I, C, D}                     xbot:1295 */
    PSIM_MSG_XBOT_SWITCH_REPLY = 21,       /* {switch_reply, Ans, Old, I, C, D}             xbot:1270 */
    PSIM_MSG_NTYPES = 24
};

/* message types of a PLUGGABLE handle (same record and stats slots) */
enum psim_pl_msg_type {
    PSIM_PL_HELLO = 0,     /* client hello on connect             peer_service_client:246-260 */
    PSIM_PL_STATE = 1,     /* server reply {state, Tag, LocalState}  peer_service_server:125-148 */
    PSIM_PL_GOSSIP = 2,    /* full: {membership_strategy, {Myself, State}}   full:127-144 */
    PSIM_PL_FWD_SUB = 3,   /* scamp: {forward_subscription, Node}  scamp_v1:212-252, v2:284-327 */
    PSIM_PL_PING = 4,      /* scamp: {ping, SourceNode}           scamp_v1:177-188, v2:181-191 */
    PSIM_PL_KEEP_SUB = 5,  /* scamp v2: {keep_subscription, Node}  scamp_v2:328-338 */
    PSIM_PL_REMOVE_SUB = 6,  /* scamp v1: {remove_subscription, Node}  scamp_v1:102-122, :190-211 */
    PSIM_PL_BOOT_REMOVE = 7  /* scamp v2: {bootstrap_remove_subscription, Node}  scamp_v2:116-127, :192-238 */
};

/* cfg.manager */
#define PSIM_MANAGER_HYPARVIEW 0   /* partisan_hyparview_peer_service_manager (+ Plumtree) */
#define PSIM_MANAGER_PLUGGABLE 1   /* partisan_pluggable_peer_service_manager + cfg.strategy */
#define PSIM_MANAGER_XBOT 2        /* partisan_hyparview_xbot_peer_service_manager (+ Plumtree) */
/* cfg.strategy (PLUGGABLE) */
#define PSIM_STRATEGY_FULL 0       /* partisan_full_membership_strategy */
#define PSIM_STRATEGY_SCAMP_V1 1   /* partisan_scamp_v1_membership_strategy */
#define PSIM_STRATEGY_SCAMP_V2 2   /* partisan_scamp_v2_membership_strategy */
#define PSIM_SVIEW_CAP 128         /* SCAMP membership / partial_view / in_view slots */

/* Plumtree peer identities: an atom name is the bare node id; a node_spec
 * map (myself(), From, Root) has this bit set.  Erlang term order puts every
 * atom before every map, which is exactly unsigned order of the encoding.
 * See SURVEY.md App. A Q6 and plumtree:662-663. */
#define PSIM_MAP_BIT 0x80000000u
#define PSIM_NONE 0xFFFFFFFFu

/* capacities of the fixed-size per-node tables */
#define PSIM_ACTIVE_CAP 8
#define PSIM_PASSIVE_CAP 32
#define PSIM_IDMAP_CAP 64   /* sent_message_map / recv_message_map slots */
#define PSIM_PT_MEMBERS_CAP 8
/* Connections of a node's HyParView manager beyond its active view
 * (SURVEY App. A Q11): partisan_util:maybe_connect/2 opens one before every
 * send and only disconnect/2 (hyparview:1237-1258) or the peer's death
 * (EXIT, :609-654) closes it, so a shuffle terminal keeps the connection to
 * its Sender (:1127-1131), a neighbor_request receiver to a rejected
 * requester (:987), a promoting node to the passive peer it asked (:1701),
 * a joiner to its contact (:506).  The table holds those lingering peers and,
 * with PSIM_CONN_DOWN set, the rare active members whose connection a
 * neighbor_rejected closed (:1063) -- an add to a full table counts an
 * overflow (PSIM_OVF_CONN) and is dropped. */
#define PSIM_CONN_CAP 8
#define PSIM_CONN_DOWN 0x80000000u
/* X-BOT handles: an active member whose connection do_disconnect/2 stopped
 * while the state that pruned it was thrown away (xbot:1367-1379 -- every
 * optimization handler discards it), so the dead pid stays in the dict until
 * its 'EXIT' (xbot:608-653) is handled at the start of the next round; sends
 * to it draw the dispatch value and fail.  At most one per member. */
#define PSIM_CONN_CLOSING 0x40000000u
#define PSIM_PT_OUT_CAP 128
#define PSIM_EXCHANGE_CAP 8
/* Plumtree roots a node keeps per-root eager/lazy sets for at once
 * (eager_sets / lazy_sets orddicts, plumtree:76-84, :599-631): a root
 * touched with every slot taken counts an overflow and is served from the
 * common sets.  The sets of all slots share one pool of PSIM_PT_SET_POOL
 * eager and one of PSIM_PT_SET_POOL lazy entries (slot k's entries follow
 * those of slots 0..k-1); an add to a full pool counts an overflow. */
#define PSIM_PT_ROOTS 4
#define PSIM_PT_SET_POOL 64
/* Live broadcast messages: message id m owns slot m mod PSIM_MSG_SLOTS of
 * every node's delivery mask (plumtree_backend's ETS set, :140-167); a new
 * broadcast retires the previous id of its slot, and a message of a retired
 * id still in flight counts an overflow and is treated as stale. */
#define PSIM_MSG_SLOTS 64
/* psim_round_stats.overflow_by: which fixed table overflowed */
#define PSIM_OVF_IDMAP 0     /* sent / recv disconnect-id maps (oldest entry replaced) */
#define PSIM_OVF_PT_OUT 1    /* Plumtree outstanding IHAVE entries (the new entry dropped) */
#define PSIM_OVF_PT 2        /* Plumtree members, per-root sets, root slots, retired message ids */
#define PSIM_OVF_STRATEGY 3  /* pluggable: SCAMP views, full-membership snapshot payload */
#define PSIM_OVF_CONN 4      /* HyParView connections beyond the active view (the new one dropped) */
#define PSIM_OVF_NKINDS 5

typedef struct psim_config {
    uint32_t abi_version;        /* must be PSIM_ABI_VERSION */
    uint32_t n_nodes;            /* global node-id space [0, n_nodes) */
    uint64_t seed;               /* Philox key (partisan_config random_seed) */
    /* HyParView keys, partisan_config.erl:102-145 (init/0 defaults) */
    uint32_t max_active_size;    /* 6, includes self */
    uint32_t min_active_size;    /* 3 */
    uint32_t max_passive_size;   /* 30 */
    uint32_t arwl;               /* 5 */
    uint32_t prwl;               /* 30 */
    uint32_t k_active;           /* 3  (hyparview:1560) */
    uint32_t k_passive;          /* 4  (hyparview:1564) */
    uint32_t shuffle_period;     /* rounds; passive_view_shuffle_period 10000 ms */
    uint32_t promotion_period;   /* rounds; RANDOM_PROMOTION_INTERVAL 5000 ms */
    uint32_t random_promotion;   /* 1 */
    uint32_t persist_epoch;      /* 0: epoch restarts at 1 (no partisan_data_dir) */
    /* Plumtree */
    uint32_t plumtree;           /* 1: run the broadcast layer */
    uint32_t lazy_tick_period;   /* rounds; DEFAULT_LAZY_TICK_PERIOD 1000 ms */
    /* execution */
    int32_t device;              /* HIP device ordinal, -1 = current */
    uint32_t n_shards;           /* node-range shards of this process (virtual shards), 1 */
    uint32_t shard_rank;         /* RCCL rank (multi-process), 0 */
    uint32_t shard_world;        /* RCCL world size, 1 */
    const void *comm_id;         /* ncclUniqueId bytes when shard_world > 1; with shard_world = 1
                                    a non-NULL id selects the rank path on a one-rank communicator
                                    (the 1-GPU diagnostic of the RCCL path: owner partition,
                                    ncclAllToAll, self ncclSend/ncclRecv, ncclAllReduce,
                                    ncclAllGather); an id from psim_host_comm_id: a
                                    host-exchange handle over part of the id space (below);
                                    NULL = the in-place route.  Every manager and strategy
                                    runs over virtual shards and ranks, the full strategy
                                    included (its STATE and GOSSIP records take the ORSet rows
                                    they name along); a host-exchange
                                    handle of the full strategy is PSIM_EUNSUPPORTED */
    uint64_t max_msgs_per_round; /* 0 = auto */
    /* pluggable manager */
    uint32_t manager;            /* PSIM_MANAGER_*, 0 = HyParView */
    uint32_t strategy;           /* PSIM_STRATEGY_* when manager = PLUGGABLE */
    uint32_t periodic_interval;  /* rounds; periodic_interval 10000 ms (partisan_config.erl:130) */
    uint32_t scamp_c;            /* scamp_c, ?SCAMP_C_VALUE = 5 (partisan.hrl:31); <= 64 */
    uint32_t fanout;             /* full: 0 = gossip to every member (reference);
                                    k > 0 = k uniformly drawn members (config B extension); <= 64 */
    uint32_t strict;             /* 0: a fixed-table overflow is counted (stats.overflow_by) and the
                                    round goes on; 1: psim_step fails with PSIM_ECAPACITY after the
                                    round in which any overflow happened (e.g. a fifth live Plumtree
                                    root at a node, or a 65th live message id) */
    uint32_t xbot_period;        /* rounds; xbot_interval (partisan_config.erl:100, :145: 5000 +
                                    uniform(60000) ms, drawn per VM from an unseeded generator --
                                    a fixed period here, default 35); X-BOT handles */
    uint32_t reserved1;
} psim_config;

typedef struct psim_round_stats {
    uint64_t round;                          /* round number just executed */
    uint64_t emitted[PSIM_MSG_NTYPES];       /* messages sent (successful sends) by type */
    uint64_t delivered[PSIM_MSG_NTYPES];     /* messages processed by a live recipient */
    uint64_t dropped;                        /* messages whose recipient was down */
    uint64_t nodes_up;
    uint64_t nodes_processed;                /* nodes with inbox, timer or event work */
    uint64_t exits;                          /* EXIT events handled */
    uint64_t send_fail;                      /* sends refused: no connection */
    uint64_t first_deliveries;               /* plumtree merge() == true this round */
    uint64_t overflow;                       /* fixed-table overflows (must be 0 in parity runs) */
    uint64_t digest;                         /* sum of per-message hashes of emitted messages */
    uint64_t state_bytes;                    /* algorithmic state bytes read+written */
    uint64_t overflow_by[PSIM_OVF_NKINDS];   /* overflow by table (PSIM_OVF_*), summing to overflow */
    uint64_t omitted;                        /* pluggable: strategy messages an omission fault dropped
                                                (at the sender: never sent, no draw; at the
                                                receiver: never handled) -- psim_set_omission */
} psim_round_stats;

/* Canonical per-node view (inspection; unused slots zero). */
typedef struct psim_node_view {
    uint32_t up, epoch, start_round;
    uint32_t conn_n;                         /* entries of conn[] */
    uint64_t rng_ctr;
    uint32_t act_n, pas_n;
    uint32_t act[PSIM_ACTIVE_CAP];           /* sets:to_list order, self included */
    uint32_t pas[PSIM_PASSIVE_CAP];          /* sets:to_list order */
    uint32_t sent_n, sent_head, recv_n, recv_head;
    uint32_t sent_peer[PSIM_IDMAP_CAP], sent_id[PSIM_IDMAP_CAP];
    uint32_t recv_peer[PSIM_IDMAP_CAP], recv_id[PSIM_IDMAP_CAP];
    uint32_t pt_all_n, pt_common_n, pt_out_n, pt_pad;
    uint32_t pt_all[PSIM_PT_MEMBERS_CAP], pt_common[PSIM_PT_MEMBERS_CAP];
    /* per-root sets, slot k: root pt_root[k] (PSIM_NONE = free); its eager
     * entries are pt_eager[o .. o + pt_eager_n[k]) with o the sum of
     * pt_eager_n[0..k) (ordsets order), the lazy ones likewise */
    uint32_t pt_root[PSIM_PT_ROOTS], pt_eager_n[PSIM_PT_ROOTS], pt_lazy_n[PSIM_PT_ROOTS];
    uint32_t pt_eager[PSIM_PT_SET_POOL], pt_lazy[PSIM_PT_SET_POOL];
    uint32_t pt_out_peer[PSIM_PT_OUT_CAP], pt_out_msg[PSIM_PT_OUT_CAP], pt_out_round[PSIM_PT_OUT_CAP];
    uint64_t have;                           /* delivered: bit (msg id mod PSIM_MSG_SLOTS) */
    uint32_t trk_round, trk_hop;
    /* connections beyond the active view (lingering peers), and active
     * members without one (| PSIM_CONN_DOWN), in insertion order */
    uint32_t conn[PSIM_CONN_CAP];
} psim_node_view;

/* Per-node state of a PLUGGABLE handle (inspection; unused slots zero). */
typedef struct psim_strategy_view {
    uint32_t up, start_round;
    uint32_t pending;                        /* contact of an unfinished join, PSIM_NONE */
    uint32_t last_ping;                      /* scamp: round of the last ping, PSIM_NONE = undefined */
    uint64_t rng_ctr;
    uint32_t view_n, in_n;
    uint32_t view[PSIM_SVIEW_CAP];           /* scamp v1 membership (sets:to_list order) /
                                                scamp v2 partial_view (list order) */
    uint32_t in_view[PSIM_SVIEW_CAP];        /* scamp v2 in_view (list order) */
    uint32_t members;                        /* full: size of query(ORSet) */
    uint32_t view_slots;                     /* scamp v1: active slots of the membership set
                                                (OTP sets v1: 16, one more past each 5 per slot;
                                                0 for an empty view and other strategies) */
    uint64_t members_hash;                   /* full: sum of mix64(id + 1) over members */
} psim_strategy_view;

/* Overlay statistics of a HyParView handle (SURVEY 8(b) psim_get_histograms,
 * 8(d) configs C/D): histograms over live nodes, bin k = value k, the last
 * bin = PSIM_HIST_BINS - 1 or more.  Links count live -> live only.
 * Replaces the reference's overlay checks: orchestration graph BFS
 * (partisan_orchestration_backend.erl:333-413, 467-489) and the SUITE's
 * connected + symmetric active views (test/partisan_SUITE.erl:2044-2108). */
#define PSIM_HIST_BINS 64
typedef struct psim_histograms {
    uint64_t n_up;                           /* live nodes */
    uint64_t active_in[PSIM_HIST_BINS];      /* by active in-degree */
    uint64_t passive_in[PSIM_HIST_BINS];     /* by passive in-degree */
    uint64_t active_out[PSIM_HIST_BINS];     /* by active view size (self excluded) */
    uint64_t passive_fill[PSIM_HIST_BINS];   /* by passive view size */
    uint64_t hop[PSIM_HIST_BINS];            /* tracked broadcast: delivered nodes by hop count */
    uint64_t delivered;                      /* live nodes holding the tracked broadcast */
    uint64_t last_round;                     /* latest first-delivery round of it (0: none) */
    uint64_t active_links;                   /* directed active links between live nodes */
    uint64_t symmetric_links;                /* ... whose reverse link exists */
    uint64_t components;                     /* weakly connected components of live nodes over
                                                active links */
    uint64_t largest_component;
    uint64_t reserved[6];
} psim_histograms;

/* Overlay statistics of a PLUGGABLE handle (SCAMP
 * beside HyParView), computed on the device from a compact CSR of the whole
 * overlay (DESIGN.md "Overlay statistics of pluggable handles").  Binning as
 * psim_histograms: bin k = value k, the last bin = PSIM_HIST_BINS - 1 or
 * more.  A link is a distinct ordered pair: an id held twice by a view counts
 * once.
 *   SCAMP v1 / v2 handles: members_* and agreeing stay zero; the in_view
 *     fields (in_fill, in_sum, in_view_links, in_view_confirmed) are v2's
 *     and zero under v1.
 *   full handles: only n_up, members_* and agreeing are filled; every view,
 *     link and component field stays zero (the strategy keeps no partial
 *     view: its overlay is the member set itself). */
typedef struct psim_strategy_histograms {
    uint64_t n_up;                              /* live nodes */
    uint64_t view_fill[PSIM_HIST_BINS];         /* live nodes by view_n: the raw list length the strategy
                                                   itself sees, self and repeats included */
    uint64_t in_fill[PSIM_HIST_BINS];           /* scamp v2: live nodes by in_n; zero otherwise */
    uint64_t out_degree[PSIM_HIST_BINS];        /* live nodes by distinct ids != self in their view (live or not) */
    uint64_t in_degree[PSIM_HIST_BINS];         /* live nodes by distinct live nodes != self whose view holds them */
    uint64_t view_sum, in_sum;                  /* sums of view_n / in_n over live nodes (exact means past the last bin) */
    uint64_t view_max, in_degree_max;
    uint64_t links;                             /* distinct directed pairs i->p, i != p, both live */
    uint64_t mutual_links;                      /* ... of which p->i is also a link */
    uint64_t dangling_links;                    /* distinct pairs i->p, i live, p != i not live */
    uint64_t self_entries;                      /* live nodes whose view holds themselves */
    uint64_t duplicate_entries;                 /* view entries of live nodes beyond the first occurrence of their id */
    uint64_t in_view_links, in_view_confirmed;  /* scamp v2: distinct (i, j), j in i's in_view, j != i, both live;
                                                   ... of which j->i is a link */
    uint64_t components, largest_component;     /* weakly connected components of live nodes over `links` */
    uint64_t isolated;                          /* live nodes with no link in or out */
    uint64_t members_min, members_max, members_sum;  /* full: |query(ORSet)| = popcount(add & ~remove) over live nodes */
    uint64_t agreeing;                          /* full: live nodes whose member set equals that of the lowest live id */
    uint64_t reserved[8];
} psim_strategy_histograms;

/* Path lengths and clustering of the overlay, computed on the device
 * (DESIGN.md "Path lengths and clustering").  The link set L is the one the
 * two structs above count: for HyParView and X-BOT handles the ordered pairs
 * (i, p), i live, p in i's active view, p != i, p live
 * (psim_histograms.active_links); for SCAMP v1 / v2 handles the distinct
 * ordered pairs of psim_strategy_histograms.links.  N(i): the out-neighbours
 * of i in L, k_i = |N(i)|.  Bins as above: bin k = value k, the last bin =
 * PSIM_HIST_BINS - 1 or more.
 *   Clustering, over every live node: closed_i = the ordered pairs (a, b),
 *     a, b in N(i), a != b, with (a, b) in L.  cl_closed / cl_pairs is the
 *     transitivity; the mean local coefficient is cl_sum_q32 / 2^32 divided
 *     by n_up or by cl_nodes (fixed point: bit-exact whatever the order of
 *     the sum).
 *   Path lengths: directed shortest distances d(s, v) over L from the live
 *     nodes among the caller's sources, slot j = sources[j]; a dead source's
 *     slot stays zero. */
#define PSIM_GRAPH_SOURCES 64
#define PSIM_GRAPH_MAX_LEVELS 4096
typedef struct psim_graph_metrics {
    uint64_t n_up;                           /* live nodes */
    uint64_t links;                          /* |L| */
    uint64_t cl_nodes;                       /* live nodes with k_i >= 2 */
    uint64_t cl_closed;                      /* sum of closed_i */
    uint64_t cl_pairs;                       /* sum of k_i (k_i - 1) */
    uint64_t cl_sum_q32;                     /* sum over k_i >= 2 of floor(closed_i 2^32 / (k_i (k_i - 1))) */
    uint64_t sources_live;                   /* live nodes among the sources */
    uint64_t dist[PSIM_HIST_BINS];           /* pairs (slot j, live v != sources[j]) by finite distance; bin 0: 0 */
    uint64_t dist_sum;                       /* the exact sum of those distances (not saturated) */
    uint64_t pairs_reached;                  /* their number */
    uint64_t pairs_unreached;                /* sources_live (n_up - 1) - pairs_reached */
    uint64_t reach[PSIM_GRAPH_SOURCES];      /* per slot: the nodes reached */
    uint32_t ecc[PSIM_GRAPH_SOURCES];        /* per slot: the largest finite distance */
    uint64_t ecc_max;
    uint64_t levels;                         /* BFS levels run (the last one may have found nothing) */
    uint64_t truncated;                      /* 1: the level cap ended the BFS with a frontier still open;
                                                pairs farther apart than the cap count as unreached */
    uint64_t reserved[8];
} psim_graph_metrics;

/* The broadcast tree of one Plumtree root R, computed on the device
 * (DESIGN.md "Broadcast tree"): what partisan_plumtree_broadcast:
 * debug_get_tree/2 (pt:235-243) folds out of debug_get_peers/2 (pt:222-231,
 * all_peers/3 pt:627-631) over every node.  Everything is an integer, so the
 * struct is bit-exact whatever the order of any sum.
 *   Sets of a live node i for R: the first root slot k with
 *     pt_root[k] == (R | PSIM_MAP_BIT) gives its eager and lazy runs; a node
 *     without such a slot answers (common_eagers, []).
 *   An entry e names node p = e & ~PSIM_MAP_BIT.  p is live if p < n_nodes
 *     and node p is up.
 *   E_i: the distinct p over i's eager entries with p != i and p live; Z_i the
 *     same over its lazy entries.  T: the ordered pairs (i, p), p in E_i.
 *   Liveness is the only filter: partitions are ignored, as in
 *     psim_histograms.  Bins as there: bin k = value k, the last bin =
 *     PSIM_HIST_BINS - 1 or more.
 *   The two BFS passes start at R and run levels d = 1, 2, ... while
 *     d <= the level cap; a level that finds no node ends the pass.  L is the
 *     link set psim_graph_metrics counts: active view, p != i, p live, repeats
 *     dropped.  With R not live every field from `depth` on is zero. */
typedef struct psim_tree_metrics {
    uint64_t n_up;                           /* live nodes */
    uint64_t root_live;                      /* 1: R is live */
    uint64_t slot_nodes;                     /* live nodes that hold a slot for R */
    uint64_t eager_entries, lazy_entries;    /* raw entries of the live nodes' sets for R */
    uint64_t eager_links;                    /* |T| = sum of |E_i| */
    uint64_t lazy_links;                     /* sum of |Z_i| */
    uint64_t both_links;                     /* sum of |E_i & Z_i| */
    uint64_t eager_both_forms;               /* (i, p) in T whose eager entries hold both p and p | PSIM_MAP_BIT */
    uint64_t self_entries;                   /* entries, eager or lazy, that decode to i itself */
    uint64_t eager_dead, lazy_dead;          /* entries that decode to another node that is not live */
    uint64_t eager_nonmember;                /* (i, p) in T with p not in i's active view */
    uint64_t lazy_nonmember;                 /* p in Z_i not in i's active view */
    uint64_t eager_symmetric;                /* (i, p) in T with (p, i) in T */
    uint64_t eager_out[PSIM_HIST_BINS];      /* live nodes by |E_i| */
    uint64_t lazy_out[PSIM_HIST_BINS];       /* live nodes by |Z_i| */
    uint64_t eager_in[PSIM_HIST_BINS];       /* live nodes by in-degree in T */
    uint64_t depth[PSIM_HIST_BINS];          /* BFS over T: nodes v != R by finite depth; bin 0: 0 */
    uint64_t depth_sum;                      /* the exact sum of those depths (not saturated) */
    uint64_t depth_max;                      /* the largest finite depth */
    uint64_t reached;                        /* their number */
    uint64_t unreached;                      /* root_live (n_up - 1) - reached: the nodes a broadcast
                                                reaches only through graft */
    uint64_t links_from_reached;             /* sum of |E_i| over i at finite depth, R included: the
                                                payload copies of a broadcast over frozen sets */
    uint64_t levels;                         /* levels the BFS over T ran (the last one may have found nothing) */
    uint64_t truncated;                      /* 1: the level cap ended either BFS with level `cap` still
                                                finding a node; nodes farther away count as unreached */
    uint64_t overlay_reached;                /* BFS over L: nodes v != R at finite distance */
    uint64_t both_reached;                   /* v != R finite in both */
    uint64_t depth_sum_both, dist_sum_both;  /* over those: tree depths, overlay distances (the stretch) */
    uint64_t deeper;                         /* ... whose tree depth exceeds the overlay distance */
    uint64_t shallower;                      /* ... the opposite (eager links to non-members exist) */
    uint64_t reserved[8];
} psim_tree_metrics;

/* Latency-weighted paths over the overlay, computed on the device (DESIGN.md
 * "Latency-weighted paths").  The weight of a link (i, p) is
 * w(i, p) = psim_xbot_latency(cfg.seed, i, p), whatever the manager: 0 ..
 * 1024.  L is the link set psim_graph_metrics counts (i live, p != i, p live,
 * repeats dropped).  Everything is an integer, so the struct is bit-exact
 * whatever the order of any sum.
 *   Cheapest paths: D_r(s, v) is the least total weight of a path s -> v over
 *     L with at most r links (no such path: infinite).  Sweep r turns D_(r-1)
 *     into D_r; the call reports D_R, R the first r at which no distance of
 *     any slot fell, or the sweep cap if that comes first.  Slot j =
 *     sources[j]; a dead source's slot stays zero.  "Fell" is strictly lower:
 *     a link of weight 0 (two nodes in one torus cell) keeps no sweep alive.
 *   The tree half, with tree_root = R != PSIM_NONE: T is psim_tree_metrics'
 *     eager link set of R; the same computation with the one source R, once
 *     over T (the tree latency of v) and once over L (its overlay latency),
 *     under the same sweep cap.  With R not live every field from tree_links
 *     on is zero. */
#define PSIM_LAT_SOURCES 64
typedef struct psim_latency_metrics {
    uint64_t n_up;                           /* live nodes */
    uint64_t links;                          /* |L| */
    uint64_t link_cost_sum;                  /* sum of w over L */
    uint64_t link_cost[PSIM_HIST_BINS];      /* links by w >> 4, the last bin = 1008 or more (w = 1024 included) */
    uint64_t link_nodes;                     /* live nodes with k_i >= 1 */
    uint64_t worst_sum;                      /* over those: the sum of the largest w of their row (what X-BOT's
                                                select_worst_in_active_view looks at) */
    uint64_t best_sum;                       /* ... of the smallest */
    uint64_t sources_live;                   /* live nodes among the sources */
    uint64_t live_mask;                      /* bit j: sources[j] is live */
    uint64_t reach[PSIM_LAT_SOURCES];        /* per slot: the nodes v != sources[j] with finite D_R */
    uint64_t lat_sum[PSIM_LAT_SOURCES];      /* per slot: the sum of those D_R */
    uint64_t lat_ecc[PSIM_LAT_SOURCES];      /* per slot: the largest of them */
    uint64_t last_sweep[PSIM_LAT_SOURCES];   /* per slot: the last sweep that lowered a distance of the slot */
    uint64_t lat[PSIM_HIST_BINS];            /* pairs (slot j, v) with finite D_R by D_R >> 8, the last bin =
                                                16128 or more */
    uint64_t lat_sum_all;                    /* the exact sum of those D_R (not saturated) */
    uint64_t lat_max;                        /* the largest */
    uint64_t pairs_reached;                  /* their number */
    uint64_t pairs_unreached;                /* sources_live (n_up - 1) - pairs_reached */
    uint64_t sweeps;                         /* R: sweeps run (the last one may have lowered nothing) */
    uint64_t truncated_mask;                 /* bit j: the sweep cap ended slot j with sweep `cap` still lowering a
                                                distance; its figures are those of D_cap */
    uint64_t tree_root_live;                 /* 1: tree_root was given and is live */
    uint64_t tree_links;                     /* |T| */
    uint64_t tree_link_cost_sum;             /* sum of w over T */
    uint64_t tree_reached;                   /* over T: nodes v != R with finite tree latency */
    uint64_t tree_lat_sum;                   /* the sum of those latencies */
    uint64_t tree_lat_max;                   /* the largest */
    uint64_t tree_sweeps;                    /* sweeps the pass over T ran (as `sweeps`) */
    uint64_t overlay_reached;                /* over L: nodes v != R with finite overlay latency */
    uint64_t both_reached;                   /* v != R finite in both */
    uint64_t tree_lat_sum_both;              /* over those: tree latencies */
    uint64_t overlay_lat_sum_both;           /* ... overlay latencies (the ratio: the tree's latency stretch) */
    uint64_t slower;                         /* ... whose tree latency exceeds the overlay latency */
    uint64_t faster;                         /* ... the opposite (eager links to non-members exist) */
    uint64_t tree_truncated;                 /* 1: the sweep cap ended either pass with sweep `cap` still lowering
                                                a distance */
    uint64_t reserved[8];
} psim_latency_metrics;

/* Broadcast reach under mass node failure, computed on the device (DESIGN.md
 * "Reach under mass failure"): up to PSIM_FAIL_CASES failure cases in one
 * bit-parallel BFS, bit j of a node's word = "in case j this node survived
 * (and has been reached)".  A case fails a pseudo-random share of all nodes at
 * one instant and floods from its source over what is left of the overlay,
 * before any healing.  Everything is an integer, so the struct is bit-exact
 * whatever the order of any sum.
 *   u(v, salt) = (uint32_t)(mix64(fail_seed ^ mix64(((uint64_t)salt << 32) | v)) >> 32),
 *     mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *     z *= 0x94D049BB133111EB; z ^= z >> 31 (64-bit, wrapping).
 *   L: the link set psim_graph_metrics counts -- for HyParView and X-BOT
 *     handles the active view, p != i, p live, repeats dropped; for SCAMP
 *     v1 / v2 handles the distinct pairs of psim_strategy_histograms.links.
 *   Case j is live if node source_j is up.  A dead source's case is skipped
 *     and all its slots stay zero, as a dead source's are in
 *     psim_graph_metrics.
 *   A_j, the survivors of live case j: the up nodes v with v == source_j or
 *     u(v, salt_j) >= threshold_j.  L_j: the links of L with both ends in A_j.
 *   Liveness is the only other filter: partitions are ignored, as in every
 *     statistics call.  The BFS runs levels d = 1, 2, ... while d <= the level
 *     cap; a level that finds no node ends it.
 * Not modelled: passive views and healing -- that experiment is psim_crash
 * plus psim_step. */
#define PSIM_FAIL_CASES 64
typedef struct psim_failure_case {
    uint32_t source;     /* the flood starts here; it never fails in its own case */
    uint32_t threshold;  /* node v != source fails iff u(v, salt) < threshold: the failed share is threshold / 2^32 */
    uint32_t salt;       /* cases with equal salts fail nested sets; different salts, independent ones */
    uint32_t reserved;   /* 0 */
} psim_failure_case;
typedef struct psim_resilience {
    uint64_t n_up;                           /* live nodes */
    uint64_t links;                          /* |L| */
    uint64_t cases_live;                     /* number of live cases */
    uint64_t live_mask;                      /* bit j set: case j is live */
    uint64_t alive[PSIM_FAIL_CASES];         /* |A_j| */
    uint64_t links_alive[PSIM_FAIL_CASES];   /* |L_j| */
    uint64_t no_out[PSIM_FAIL_CASES];        /* nodes of A_j with no out-link in L_j */
    uint64_t no_in[PSIM_FAIL_CASES];         /* nodes of A_j with no in-link in L_j, the source included
                                                if it has none: a flood can never reach these */
    uint64_t reached[PSIM_FAIL_CASES];       /* nodes v != source_j at finite directed distance from
                                                source_j over L_j; reliability = reached / (alive - 1) */
    uint64_t hop_sum[PSIM_FAIL_CASES];       /* the exact sum of those distances */
    uint64_t ecc[PSIM_FAIL_CASES];           /* the largest finite distance */
    uint64_t ecc_max;                        /* the largest ecc[j] */
    uint64_t levels;                         /* BFS levels run (the last one may have found nothing) */
    uint64_t truncated;                      /* 1: the level cap ended the BFS with level `cap` still
                                                finding a node; farther nodes count as not reached */
    uint64_t reserved[8];
} psim_resilience;

/* Gossip with a fanout over the overlay, under the failure cases of
 * psim_resilience, computed on the device (DESIGN.md "Gossip with a fanout"):
 * the other side of that experiment -- a node pushes to at most `fanout` of
 * its links instead of flooding all of them.  Up to PSIM_FAIL_CASES cases in
 * one bit-parallel BFS; everything is an integer, so the struct is bit-exact
 * whatever the order of any sum.
 *   mix64, u, L, the live cases and A_j are psim_resilience's: for the same
 *     (source, threshold, salt, fail_seed) alive[j] is the same number.  N(i):
 *     the targets of i's links in L, k_i = |N(i)| (psim_graph_metrics).  View
 *     entries that name down nodes are not in L, so they are no candidates.
 *   h(i, salt) = mix64(fail_seed ^ mix64(((uint64_t)salt << 32) | i)), so
 *     u(v, salt) = (uint32_t)(h(v, salt) >> 32).
 *   w(i, p, salt) = mix64(h(i, salt) + 0x9E3779B97F4A7C15 * (p + 1)) (64-bit,
 *     wrapping).  S_j(i), the targets node i pushes to in case j: N(i) if
 *     fanout_j == 0 or fanout_j >= k_i; otherwise the fanout_j ids p of N(i)
 *     with the smallest (w(i, p, salt_j), p).  The choice depends on the set
 *     N(i), not on the order of a view, so it is the same for any shard count.
 *   A node chooses among all of N(i), the nodes failed in the case included:
 *     the failure is not yet detected (before any healing), and a copy to such
 *     a target is lost.
 *   Infect-and-die: a node sends once, when first reached, to S_j(i).  G_j:
 *     the pairs (i, p) with i, p in A_j and p in S_j(i).  The BFS from
 *     source_j over G_j runs levels d = 1, 2, ... while d <= the level cap; a
 *     level that finds no node in any case ends it.
 *   The senders of case j: the source and every node reached at a distance
 *     below the level cap.
 *   Liveness is the only other filter: partitions are ignored, as in every
 *     statistics call.  A dead source's case is skipped and its slots stay
 *     zero. */
typedef struct psim_gossip_case {
    uint32_t source;     /* the gossip starts here; it never fails in its own case */
    uint32_t threshold;  /* node v != source fails iff u(v, salt) < threshold (as psim_failure_case) */
    uint32_t salt;       /* failure set and target choice; equal salts: nested failure sets, same choices */
    uint32_t fanout;     /* 0: every link (a flood); f > 0: at most f links per node */
} psim_gossip_case;
typedef struct psim_gossip_reach {
    uint64_t n_up;                           /* live nodes */
    uint64_t links;                          /* |L| */
    uint64_t cases_live;                     /* number of live cases */
    uint64_t live_mask;                      /* bit j set: case j is live */
    uint64_t alive[PSIM_FAIL_CASES];         /* |A_j| */
    uint64_t reached[PSIM_FAIL_CASES];       /* nodes v != source_j at finite directed distance from
                                                source_j over G_j; reliability = reached / (alive - 1) */
    uint64_t hop_sum[PSIM_FAIL_CASES];       /* the exact sum of those distances */
    uint64_t ecc[PSIM_FAIL_CASES];           /* the largest finite distance */
    uint64_t sent[PSIM_FAIL_CASES];          /* copies sent: the sum of |S_j(i)| over the senders */
    uint64_t lost[PSIM_FAIL_CASES];          /* ... of which to a target outside A_j; sent - lost -
                                                reached: the copies that arrive at a node that has one */
    uint64_t ecc_max;                        /* the largest ecc[j] */
    uint64_t levels;                         /* BFS levels run (the last one may have found nothing) */
    uint64_t truncated;                      /* 1: the level cap ended the BFS with level `cap` still
                                                finding a node; those nodes do not send */
    uint64_t reserved[8];
} psim_gossip_reach;

/* Transitive unicast over the overlay, computed on the device (DESIGN.md
 * "Transitive unicast"): what a forward_message with {broadcast, true} and
 * {transitive, true} does under the HyParView manager -- the
 * {relay_message, Node, Message, TTL} flood down the "tree" out-links
 * (hyparview:1138-1163, :1274-1343, :1800-1868, :563-570) -- over the frozen
 * state, up to PSIM_RELAY_CASES (source, target, ttl) cases at once.  Nothing
 * deduplicates, so the flood counts walks: a level holds entries (node v,
 * remaining ttl t) -> c copies.  Everything is an integer, so the struct is
 * bit-exact whatever the order of any sum.
 *   Node p is live if p < n_nodes and node p is up.  Liveness is the only
 *     filter: partitions are ignored, as in every statistics call.
 *   state(i, p) for a live i, p != i and p live, from act and conn of
 *     psim_node_view, decided in this order: conn(i) holds p | PSIM_CONN_DOWN:
 *     `down` if p is in act(i), otherwise `none`; conn(i) holds plain p (a
 *     lingering peer): `connected`; p is in act(i): `connected`; otherwise
 *     `none` -- also for p == i or p not live.
 *   out(i): the entries e of pt_common[0 .. pt_common_n) with e != i -- the
 *     atom self is what `-- [node()]` removes; retrieve_outlinks/0 asks with
 *     the atom root, so all_peers/3 (pt:627-631) always answers common_eagers,
 *     never a per-root set.  Each entry is one send, to p = e & ~PSIM_MAP_BIT.
 *   The census, over live i: out_entries = the sum of |out(i)|; out_usable its
 *     entries with state(i, p) `connected`; out_nonmember its entries whose p
 *     is not in act(i); members_down the pairs (i, p), p in act(i), with
 *     state(i, p) `down`; out_degree bins the live nodes by their usable
 *     entries (bin k = value k, the last bin = PSIM_HIST_BINS - 1 or more).
 *   Case j = (s, d, T) is live if s and d are both live; a case that is not
 *     is skipped and its slots stay zero.
 *   Origin: state(s, d) `connected`: the send is direct -- bit j of
 *     direct_mask, delivered = first_hop = hop_sum = 1 and nothing else.
 *     Otherwise s runs forward(s, T, 1).
 *   forward(v, t, c): for each e of out(v): state(v, p) `connected`: relays +=
 *     c, and c copies arrive at (p, t - 1) on the next level; otherwise
 *     refused += c.
 *   Level l = 1, 2, ... takes the merged entries (v, t) -> c of that level:
 *     d in act(v) and state(v, d) `connected`: delivered += c, hop_sum +=
 *     c (l + 1), first_hop = l + 1 if it is still 0; d in act(v) with any
 *     other state: restarts += c and forward(v, T, c) -- do_send_message with
 *     {transitive, true} and no connection starts a new tree forward with a
 *     fresh ttl (hv:1150, :1289-1295, :1323-1335); d not in act(v) and t == 0:
 *     expired += c; otherwise forward(v, t, c).
 *   Levels run while l <= the level cap.  levels[j]: the last level run that
 *     had entries of case j; peak[j]: the most distinct (v, t) entries of the
 *     case on one level run.  If level cap + 1 would have entries of case j,
 *     bit j of truncated_mask is set and in_flight[j] is the sum of their
 *     counts (copies already counted in relays).
 *   pt_common holds at most PSIM_PT_MEMBERS_CAP = 8 entries, so no count
 *     exceeds 8^16 = 2^48 and no sum overflows. */
#define PSIM_RELAY_CASES 64
#define PSIM_RELAY_MAX_TTL 16      /* also the level cap's maximum */
typedef struct psim_relay_case {
    uint32_t source;     /* the node that calls forward_message */
    uint32_t target;     /* the node the message is for; != source */
    uint32_t ttl;        /* 1 .. PSIM_RELAY_MAX_TTL; the reference's RELAY_TTL is 5 (partisan.hrl:9) */
    uint32_t reserved;   /* 0 */
} psim_relay_case;
typedef struct psim_relay_reach {
    uint64_t n_up;                           /* live nodes */
    uint64_t out_entries;                    /* sum of |out(i)| */
    uint64_t out_usable;                     /* ... with state `connected` */
    uint64_t out_nonmember;                  /* ... whose p is not in act(i): stale entries */
    uint64_t members_down;                   /* (i, p), p in act(i), state `down` */
    uint64_t out_degree[PSIM_HIST_BINS];     /* live nodes by usable out entries */
    uint64_t cases_live;                     /* number of live cases */
    uint64_t live_mask;                      /* bit j set: case j is live */
    uint64_t direct_mask;                    /* bit j set: the source holds a connection to the target */
    uint64_t truncated_mask;                 /* bit j set: the level cap ended case j with copies in flight */
    uint64_t levels_max;                     /* the largest levels[j] */
    uint64_t delivered[PSIM_RELAY_CASES];    /* copies handed to the target */
    uint64_t first_hop[PSIM_RELAY_CASES];    /* sends on the shortest delivering walk, 0: none */
    uint64_t hop_sum[PSIM_RELAY_CASES];      /* sends summed over the delivered copies */
    uint64_t relays[PSIM_RELAY_CASES];       /* relay_message sends */
    uint64_t refused[PSIM_RELAY_CASES];      /* sends to an out entry without a connection */
    uint64_t expired[PSIM_RELAY_CASES];      /* copies dropped at ttl 0 */
    uint64_t restarts[PSIM_RELAY_CASES];     /* copies whose holder restarted the flood with a fresh ttl */
    uint64_t in_flight[PSIM_RELAY_CASES];    /* copies the level cap cut off */
    uint64_t levels[PSIM_RELAY_CASES];       /* the last level that had entries */
    uint64_t peak[PSIM_RELAY_CASES];         /* the most distinct (v, t) entries on one level */
    uint64_t reserved[8];
} psim_relay_reach;

typedef struct psim_handle psim_handle;

void psim_default_config(psim_config *cfg);
int psim_create(const psim_config *cfg, psim_handle **out);
void psim_destroy(psim_handle *h);
const char *psim_strerror(int code);
int psim_abi_version(void);

/* Events take effect at the start of the next round. */
int psim_join(psim_handle *h, const uint32_t *nodes, const uint32_t *contacts, size_t n);
int psim_crash(psim_handle *h, const uint32_t *nodes, size_t n);
/* Restart nodes (crashed, or never started) without a join: each comes back
 * with init/1 state -- empty views, a fresh incarnation (epoch + 1 when
 * persist_epoch), its draw counter back at 0 -- and waits to be reached
 * (hyparview:289-354; a node restarted by its supervisor, not told to
 * join).  Same as psim_join with every contact PSIM_NONE. */
int psim_revive(psim_handle *h, const uint32_t *nodes, size_t n);
/* leave/0 at each node (pluggable manager only; the HyParView manager's
 * leave answers `error`, hv:363-364, so PSIM_EUNSUPPORTED there).  The
 * manager stops inside handle_call({leave, Myself}) (pluggable:502-515)
 * before the Strategy:leave/2 messages it cast to itself are sent
 * (pluggable:1390-1420, :1585-1609), so the node goes down without a word,
 * exactly as psim_crash.  Revive with psim_revive. */
int psim_leave(psim_handle *h, const uint32_t *nodes, size_t n);
/* leave/1: actors[i] removes targets[i] from the cluster
 * (handle_call({leave, Node}) pluggable:502-515 -> internal_leave/2
 * :1390-1420); actor == target is leave/0 above.  SCAMP v1 / v2 handles:
 *   v1: the actor drops the target and sends {remove_subscription, T} to its
 *       old membership (scamp_v1:102-122); a receiver holding T crashes on
 *       the swapped sets:del_element/2 arguments (scamp_v1:197, SURVEY App. A
 *       Q12) -- T itself included;
 *   v2: the actor sends {bootstrap_remove_subscription, T} to its partial
 *       view (scamp_v2:116-127); T, on receipt, stops before its replacement
 *       casts go out (lists:nth(0, ..) or the self-less reset, :192-238);
 *   full: the actor tombstones T's add in its ORSet and gossips the new state
 *       to its old members (full:58-89); merges carry the removal on, and a
 *       node that merges a removal of itself stops (pluggable:1182-1188).
 * A stopping manager sends nothing in that round (its sends are casts to
 * itself) and is down from the next round on.  One call per actor per
 * round.  Multi-rank handles: every rank makes the same calls; a stop
 * reported by the target's rank is all-gathered after the round.
 * PSIM_EUNSUPPORTED for HyParView handles. */
int psim_leave_node(psim_handle *h, const uint32_t *actors, const uint32_t *targets, size_t n);
/* group[i]: node i's partition group, 0..PSIM_PARTITION_MAX (PSIM_EINVAL for
 * any other value); nodes in different groups cannot exchange messages from
 * the next round on (partisan_SUITE's partition injection). */
#define PSIM_PARTITION_MAX 254
int psim_set_partition(psim_handle *h, const uint8_t *group, size_t n);
/* View order.  Views are kept in sets:to_list/1 order of
 * OTP's sets v1, a linear hash table (stdlib sets.erl: 16 slots up to 80
 * elements, yielded slot 1..n, oldest first within a slot; one more slot
 * each time the size passes 5 n, one fewer when it drops below 3 n), so every
 * select_random index and every shuffle key pairing (hyparview:1230-1231,
 * :1346-1361; scamp_v1's membership, scamp_v1:45-279) depends on the slot of
 * each element, erlang:phash(NodeSpec, MaxN) with MaxN = 16, 32, ...
 * psim_set_phash_table takes the whole hash: phash[i] =
 * erlang:phash(NodeSpec_i, 4294967296) - 1 for node i (phash(T, R) - 1 is
 * that value mod R for every power of two R), n = n_nodes -- e.g. the table
 * the in-BEAM harness exports (erlang/harness, `B id hash` lines).  The
 * engine keeps its low 8 bits: every set it holds (views of <= 128 ids) has
 * MaxN <= 32.  psim_set_bucket_table takes the 16-slot bucket alone
 * (phash(NodeSpec, 16) - 1, 0..15): enough for every HyParView view; a SCAMP
 * v1 view past 80 ids then reads the missing bits as 0.  Without a table the
 * handle uses a stand-in hash (murmur3 fmix32(id)).  Valid only before the
 * first round (PSIM_ESTATE after); NULL restores the stand-in.  Multi-rank
 * handles: every rank passes the same table.  The table is not part of
 * psim_snapshot, but a snapshot records its hash: set the same table on the
 * new handle before psim_restore (PSIM_EINVAL otherwise). */
int psim_set_bucket_table(psim_handle *h, const uint8_t *buckets, size_t n);
int psim_set_phash_table(psim_handle *h, const uint32_t *phash, size_t n);
int psim_clear_partition(psim_handle *h);
/* Omission faults of the pluggable manager's interposition layer
 * (add_interposition_fun/2, remove_interposition_fun/1 pluggable:297-326;
 * the folds in handle_cast({forward_message, ..}) :669-836 and
 * handle_cast({receive_message, ..}) :634-667), as the crash-fault model
 * installs them (test/prop_partisan_crash_fault_model.erl:93-196):
 *   PSIM_OMIT_SEND     {send_omission, Dst} at Src (:158-196): a strategy
 *                      message Src forwards to Dst becomes `undefined` -- not
 *                      sent, no connection lookup, no dispatch draw;
 *   PSIM_OMIT_RECEIVE  {receive_omission, Src} at Dst (:117-155): a strategy
 *                      message Dst receives from Src is dropped unhandled.
 * on = 1 installs (src[i], dst[i]) pairs, on = 0 removes them (installing a
 * pair twice keeps one: the funs are a dict keyed by name).
 * psim_set_faulted is the general omission begin_omission/end_omission
 * (:93-114, `faulted` read by the interposition funs of
 * partisan_trace_orchestrator:621-656): every strategy message the node
 * sends or receives is dropped.  The hello/state handshake is the
 * client/server processes' and passes.  psim_clear_faults removes all
 * (resolve_all_faults_with_heal :198-229 removes every interposition fun,
 * the `faulted` reader included).  Changes take effect at the start of
 * the next round; dropped messages count in psim_round_stats.omitted.
 * PSIM_EUNSUPPORTED for HyParView handles (that manager has no interposition
 * layer). */
#define PSIM_OMIT_SEND 0
#define PSIM_OMIT_RECEIVE 1
int psim_set_omission(psim_handle *h, int kind, const uint32_t *src, const uint32_t *dst, size_t n, int on);
int psim_set_faulted(psim_handle *h, const uint32_t *nodes, size_t n, int on);
int psim_clear_faults(psim_handle *h);
/* broadcast/2 at `root` (plumtree:176-178) with the partisan_plumtree_backend
 * heartbeat semantics (backend:179-200), originated in the next round.  Any
 * node can be a root; per round at most one broadcast per root and per
 * message slot (msg_id mod PSIM_MSG_SLOTS), else PSIM_EINVAL.  The last call
 * names the tracked broadcast of psim_get_delivery / psim_get_histograms. */
int psim_broadcast(psim_handle *h, uint32_t root, uint32_t msg_id);

/* Run n_rounds BSP rounds; stats (may be NULL) receives one entry per round.
 * An error from inside a round (PSIM_ENOMEM, PSIM_EDEVICE, PSIM_ECOMM) leaves
 * the state off a round boundary: the handle is unusable -- every later
 * psim_step answers PSIM_ESTATE -- until psim_restore loads a snapshot into
 * it.  PSIM_ECAPACITY (cfg.strict) is returned after a whole round and does
 * not poison the handle. */
int psim_step(psim_handle *h, uint32_t n_rounds, psim_round_stats *stats);

/* Inspection: views of nodes [first, first+count) into caller buffers. */
int psim_get_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_node_view *out);
int psim_get_round(psim_handle *h, uint64_t *round);
/* PLUGGABLE handles: strategy state of nodes [first, first+count); as
 * psim_get_nodes, a rank handle answers for the ids it owns (PSIM_ERANGE
 * beyond them) */
int psim_get_strategy_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_strategy_view *out);
/* full strategy: the member bitset of one node (bit j of word j/32 = node j);
 * a rank handle answers for the ids it owns */
int psim_get_member_bits(psim_handle *h, uint32_t node, uint32_t *words, size_t n_words);
/* Delivery state of the tracked broadcast (the last psim_broadcast) at nodes
 * [first, first+count): have (0/1), first-delivery round and hop count
 * (plumtree_backend merge/2 + the broadcast's Round field, pt:288-293). */
int psim_get_delivery(psim_handle *h, uint32_t first, uint32_t count, uint8_t *have, uint32_t *round,
                      uint32_t *hop);
/* Overlay statistics (psim_histograms above); HyParView handles only.
 * Symmetry and connectivity cover the whole overlay for any shard count:
 * sharded handles gather every node's active row first (device copies, or an
 * ncclAllGather across RCCL ranks -- a collective: every rank must call). */
int psim_get_histograms(psim_handle *h, psim_histograms *out);
/* Overlay statistics of a pluggable handle (psim_strategy_histograms above).
 * PSIM_EINVAL for a null argument, PSIM_EUNSUPPORTED for HyParView and X-BOT
 * handles (psim_get_histograms is theirs).  Only the reduced counters come
 * back to the host.  Read-only: the rounds stepped after it are those of a
 * run without it.  Like psim_get_histograms a collective on rank handles
 * (every rank must call; every rank gets the same struct). */
int psim_get_strategy_histograms(psim_handle *h, psim_strategy_histograms *out);
/* Path lengths from up to PSIM_GRAPH_SOURCES sources (one bit-parallel BFS)
 * and the clustering of the whole overlay (psim_graph_metrics above), on the
 * device, for HyParView, X-BOT and SCAMP v1 / v2 handles.  n_sources == 0
 * fills the clustering half only.  max_levels caps the BFS: 0 means
 * PSIM_GRAPH_MAX_LEVELS, and larger values are clamped to it.
 * PSIM_EINVAL for a null h or out, null sources with n_sources > 0,
 * n_sources > PSIM_GRAPH_SOURCES or a repeated source; PSIM_ERANGE for a
 * source >= n_nodes (a dead source is legal and skipped); PSIM_EUNSUPPORTED
 * for full-membership handles (their overlay is the member set) and
 * host-exchange handles; PSIM_ESTATE with a round open.  Read-only: the
 * rounds stepped after it are those of a run without it.  A collective on
 * rank handles (every rank calls with the same arguments; every rank gets the
 * same struct). */
int psim_get_graph_metrics(psim_handle *h, const uint32_t *sources, size_t n_sources, uint32_t max_levels,
                           psim_graph_metrics *out);
/* The broadcast tree of Plumtree root `root` (psim_tree_metrics above), on
 * the device, for HyParView and X-BOT handles with cfg.plumtree set, of any
 * shard count.  max_levels caps both BFS passes: 0 means
 * PSIM_GRAPH_MAX_LEVELS, and larger values are clamped to it.  PSIM_EINVAL
 * for a null h or out; PSIM_EUNSUPPORTED for pluggable handles, host-exchange
 * handles and plumtree = 0; PSIM_ERANGE for root >= n_nodes (a dead root is
 * legal: the BFS fields stay zero); PSIM_ESTATE with a round open.
 * Read-only: the rounds stepped after it are those of a run without it.  A
 * collective on rank handles (every rank calls with the same arguments; every
 * rank gets the same struct).  No Erlang binding yet. */
int psim_get_tree_metrics(psim_handle *h, uint32_t root, uint32_t max_levels, psim_tree_metrics *out);
/* Reach of a flood under up to PSIM_FAIL_CASES failure cases
 * (psim_resilience above), on the device, for HyParView, X-BOT and SCAMP
 * v1 / v2 handles of any shard count; slot j of every per-case array is
 * cases[j].  Two cases may name the same source.  n_cases == 0 fills n_up and
 * links only.  max_levels caps the BFS: 0 means PSIM_GRAPH_MAX_LEVELS, and
 * larger values are clamped to it.  Errors, in this order: PSIM_EINVAL for a
 * null h or out, null cases with n_cases > 0, n_cases > PSIM_FAIL_CASES or a
 * non-zero `reserved`; PSIM_EUNSUPPORTED for full-membership and
 * host-exchange handles; PSIM_ESTATE with a round open; PSIM_ERANGE for a
 * source >= n_nodes (a dead source is legal and skipped).  Read-only: the
 * rounds stepped after it are those of a run without it.  A collective on
 * rank handles (every rank calls with the same arguments; every rank gets the
 * same struct).  No Erlang binding yet. */
int psim_get_resilience(psim_handle *h, const psim_failure_case *cases, size_t n_cases, uint64_t fail_seed,
                        uint32_t max_levels, psim_resilience *out);
/* Reach and cost of a gossip with a fanout under up to PSIM_FAIL_CASES cases
 * (psim_gossip_reach above), on the device, for HyParView, X-BOT and SCAMP
 * v1 / v2 handles of any shard count; slot j of every per-case array is
 * cases[j].  Any fanout is legal, and two cases may name the same source.
 * n_cases == 0 fills n_up and links only.  max_levels caps the BFS: 0 means
 * PSIM_GRAPH_MAX_LEVELS, and larger values are clamped to it.  Errors, in this
 * order: PSIM_EINVAL for a null h or out, null cases with n_cases > 0 or
 * n_cases > PSIM_FAIL_CASES; PSIM_EUNSUPPORTED for full-membership and
 * host-exchange handles; PSIM_ESTATE with a round open; PSIM_ERANGE for a
 * source >= n_nodes (a dead source is legal and skipped).  Read-only: the
 * rounds stepped after it are those of a run without it.  A collective on
 * rank handles (every rank calls with the same arguments; every rank gets the
 * same struct).  No Erlang binding yet. */
int psim_get_gossip_reach(psim_handle *h, const psim_gossip_case *cases, size_t n_cases, uint64_t fail_seed,
                          uint32_t max_levels, psim_gossip_reach *out);
/* Transitive unicasts over up to PSIM_RELAY_CASES (source, target, ttl) cases
 * (psim_relay_reach above), on the device, for HyParView handles with
 * Plumtree, of any shard count; slot j of every per-case array is cases[j].
 * Two cases may name the same pair.  n_cases == 0 fills the census only.
 * max_levels caps the levels: 0 means PSIM_RELAY_MAX_TTL, and larger values
 * are clamped to it.  Errors, in this order: PSIM_EINVAL for a null h or out,
 * null cases with n_cases > 0, n_cases > PSIM_RELAY_CASES, a non-zero
 * `reserved`, a ttl of 0 (the reference loops forever on it) or above
 * PSIM_RELAY_MAX_TTL, or source == target; PSIM_EUNSUPPORTED for pluggable,
 * X-BOT (its relay_message/3 carries no ttl, xbot:1157-1161: another rule) and
 * host-exchange handles and plumtree = 0; PSIM_ESTATE with a round open;
 * PSIM_ERANGE for a source or target >= n_nodes (a dead one is legal: the case
 * is skipped); PSIM_ENOMEM if the temporaries of the frontier cannot be had
 * (the handle stays usable).  Read-only: the rounds stepped after it are those
 * of a run without it.  A collective on rank handles (every rank calls with
 * the same arguments; every rank gets the same struct).  No Erlang binding yet
 * (INTEGRATION.md). */
int psim_get_relay_reach(psim_handle *h, const psim_relay_case *cases, size_t n_cases, uint32_t max_levels,
                         psim_relay_reach *out);
/* Link costs and cheapest paths by latency from up to PSIM_LAT_SOURCES
 * sources (psim_latency_metrics above), on the device, for HyParView, X-BOT
 * and SCAMP v1 / v2 handles of any shard count.  n_sources == 0 with
 * tree_root == PSIM_NONE fills the link census only.  tree_root != PSIM_NONE
 * adds the tree half (HyParView and X-BOT handles with cfg.plumtree set).
 * max_sweeps caps the sweeps of every pass: 0 means PSIM_GRAPH_MAX_LEVELS, and
 * larger values are clamped to it.  Errors, in this order: PSIM_EINVAL for a
 * null h or out, null sources with n_sources > 0 or n_sources >
 * PSIM_LAT_SOURCES; PSIM_EUNSUPPORTED for full-membership and host-exchange
 * handles, and for a tree_root on a pluggable handle or with plumtree = 0;
 * PSIM_ESTATE with a round open; PSIM_ERANGE for a source or a tree_root
 * >= n_nodes (a dead one is legal and skipped); PSIM_EINVAL for a repeated
 * source; PSIM_ENOMEM if the temporaries (two rows of 64 distances a node,
 * 512 B) cannot be had: the handle stays usable.  Read-only: the rounds
 * stepped after it are those of a run without it.  A collective on rank
 * handles (every rank calls with the same arguments; every rank gets the same
 * struct).  No Erlang binding yet. */
int psim_get_latency_metrics(psim_handle *h, const uint32_t *sources, size_t n_sources, uint32_t tree_root,
                             uint32_t max_sweeps, psim_latency_metrics *out);
/* Snapshot of the whole simulation state of this process (node rows,
 * in-flight messages, round, events not yet applied are not included):
 * with buf == NULL (or cap too small) only *need is set.  psim_restore
 * loads it into a handle created with the same config (and the same
 * view-order table, whose hash the snapshot records: PSIM_EINVAL otherwise);
 * the rounds that follow are identical to the original's (HyParView
 * handles).  A restore replaces the whole state -- events queued and not yet
 * applied are dropped -- and puts a handle a failed psim_step left unusable
 * back into service. */
int psim_snapshot(psim_handle *h, void *buf, size_t cap, size_t *need);
int psim_restore(psim_handle *h, const void *buf, size_t size);

/* Message trace: the records sent to or by watched nodes, captured on the
 * device ("Message trace") -- the engine's side of the
 * message stream partisan_trace_orchestrator records through interposition.
 * Read-only and off by default: an unarmed handle launches and allocates
 * nothing for it, and the rounds stepped with a watch armed are those of a run
 * without it (psim_step then runs single rounds, as under PSIM_NO_BATCH).
 *   While a watch is armed, after every round r stepped (r =
 * psim_round_stats.round) the engine captures the records sent in it -- the
 * inbox round r + 1 will read: every successful send, whether or not the
 * recipient is up to handle it.  A record is kept if bit (its type) of
 * type_mask is set (psim_msg_type / psim_pl_msg_type) and its dst is watched
 * with PSIM_TRACE_TO in dir, or its src is watched with PSIM_TRACE_FROM.
 *   A record is 16 words in psim_wire_encode's layout (dst, src, type |
 * ttl << 8 | nex << 16, seq, a0..a3, ex[0..8)); rounds[i] is the r of record
 * i.  Records come in ascending (round, dst, src, seq) order -- the inbox's
 * canonical order, round by round -- whatever the shard count.  Under the
 * full strategy the words past the first four of a STATE or GOSSIP record are
 * references into a shard-local arena, copied as they are: opaque.  (Word 7
 * of a pluggable handle's other records, an arena slot inside the engine and
 * no part of the message, comes out 0, as from psim_get_outbound.)
 * psim_trace_watch  arms a watch on the n ids of nodes (a set: a repeated id
 *     is legal; nodes == NULL with n == 0: every node), replacing the one
 *     before it with its buffered records and lost count; it takes effect with
 *     the next round stepped.  capacity: the records kept between two reads --
 *     the first `capacity` matches in the order above, whatever the number of
 *     virtual shards; every later match counts in `lost`.  Errors, in this
 *     order: PSIM_EINVAL for a null h, null nodes with n > 0, dir 0 or above
 *     3, type_mask 0 or with a bit at or above PSIM_MSG_NTYPES, capacity 0;
 *     PSIM_EUNSUPPORTED for a host-exchange handle (psim_get_outbound is its
 *     view); PSIM_ERANGE for an id >= n_nodes; PSIM_ENOMEM when the buffers
 *     (64 + 4 bytes a record and n_nodes / 8 bytes, per shard) cannot be
 *     allocated: the handle stays usable and the old watch as it was.
 * psim_trace_read   *n = the records kept, *lost (may be NULL) = the matches
 *     beyond them.  With recs == NULL or cap (in records) < *n that is all;
 *     otherwise every record is copied out (rounds must be non-NULL), the
 *     buffer emptied and lost zeroed, so the whole capacity is free again.
 *     PSIM_EINVAL for a null h or n, or rounds NULL with recs given;
 *     PSIM_ESTATE with no watch armed.  Works on a handle a failed psim_step
 *     left unusable.
 * psim_trace_clear  disarms the watch and frees its buffers; a no-op on an
 *     unarmed handle.
 * A rank handle traces the records whose dst it owns, with its own capacity,
 * and makes no collective (as psim_get_nodes answers for owned ids); since an
 * armed handle steps round by round, every rank arms and clears its watch
 * before the same psim_step.  psim_snapshot does not include the trace and
 * psim_restore leaves the watch and the buffered records alone.  No Erlang
 * binding yet. */
#define PSIM_TRACE_TO   1u   /* a record whose dst is watched */
#define PSIM_TRACE_FROM 2u   /* a record whose src is watched */
int psim_trace_watch(psim_handle *h, const uint32_t *nodes, size_t n, uint32_t dir,
                     uint32_t type_mask, size_t capacity);
int psim_trace_read(psim_handle *h, uint32_t *recs, uint32_t *rounds, size_t cap,
                    size_t *n, uint64_t *lost);
int psim_trace_clear(psim_handle *h);

/* The live Plumtree message slots (plumtree_backend's ETS set keyed by
 * message id, :140-167): ids[k] = the message id owning slot k (PSIM_NONE =
 * free) and roots[k] its root (node_spec identity, | PSIM_MAP_BIT), for
 * k < PSIM_MSG_SLOTS; cap must be >= PSIM_MSG_SLOTS.  A node's delivery bit
 * k (psim_node_view.have) answers is_stale/1 for ids[k] only. */
int psim_get_msg_slots(psim_handle *h, uint32_t *ids, uint32_t *roots, size_t cap);

/* X-BOT's latency oracle (is_better/3 + is_better_node_by_latency/2,
 * xbot:1318-1333: timer:tc of net_adm:ping from the deciding node).  The
 * simulator places every node on a 1024 x 1024 torus from a hash of (seed,
 * id) and takes the ping time from a to b as their toroidal L1 distance
 * (0 for a == b); a crashed or never-started node answers pang.  Exported so
 * hosts and tests can read the same metric. */
uint32_t psim_xbot_latency(uint64_t seed, uint32_t a, uint32_t b);

/* Wire format of a partisan peer connection, for mixed
 * clusters of real and simulated nodes: a frame is {packet, 4} -- a 4-byte
 * big-endian length (peer_service_client.erl:214) -- around
 * partisan_util:term_to_iolist/1 of the message -- what the connection's
 * send path writes (client:95, :130, :275; util:235-297; the receiver,
 * peer_service_server.erl:172-182, takes any term encoding).  A
 * record is the engine's 64-B message record (words: dst, src,
 * type | ttl << 8 | nex << 16, seq, a0, a1, a2, a3, ex[0..8)); its term is
 * the one the reference's handler sends (HyParView hv:506-1131, Plumtree as
 * {forward_message, partisan_plumtree_broadcast, {'$gen_cast', Msg}}
 * (cast_message/3 hv:147-154, forward_message hv:441-460) with the
 * backend's heartbeat ids {RootName, Counter}, X-BOT xbot:1171-1314; the
 * table is in partisan_amd/csrc/psim_wire.cpp).  Node id i is the node_spec
 * #{name => '<prefix><i>@<host>', listen_addrs => [#{ip => ip_base + i,
 * port => port}], channels => [undefined], parallelism => 1}
 * (partisan_peer_service_manager.erl:71-76). */
typedef struct psim_wire_names {
    const char *prefix;          /* node name prefix, e.g. "n" */
    const char *host;            /* node name host part, e.g. "127.0.0.1" */
    uint32_t ip_base;            /* IPv4 of node 0 (host order); node i has ip_base + i */
    uint32_t port;               /* listen port (PEER_PORT 9090, partisan.hrl:3) */
} psim_wire_names;
/* One record to one frame (*len bytes).  With buf == NULL or cap < *len only
 * *len is set.  PSIM_EINVAL for a record no handler sends (an IHAVE of a
 * retired id: no root). */
int psim_wire_encode(const uint32_t rec[16], const psim_wire_names *names, uint8_t *buf, size_t cap, size_t *len);
/* The first frame of buf back to a record (dst = the connection's peer,
 * passed in; seq = 0: the order of a connection is its sequence); *used =
 * the frame's bytes.  PSIM_ERANGE: buf holds no complete frame yet;
 * PSIM_EINVAL: not one of the messages above. */
int psim_wire_decode(const uint8_t *buf, size_t len, const psim_wire_names *names, uint32_t dst, uint32_t rec[16],
                     size_t *used);

/* Whether a record may enter a handle of this config (host code, beside the
 * codec: callable without a GPU).  PSIM_EINVAL: a type no handler of
 * cfg->manager receives (or, under the full strategy, one whose payload lives
 * in a shard-local arena), or nex > PSIM_EXCHANGE_CAP; PSIM_ERANGE: dst, src,
 * one of ex[0..nex) or a word the type's handler reads as a node id is >=
 * cfg->n_nodes -- a Plumtree identity may carry PSIM_MAP_BIT, an IHAVE's root
 * and X-BOT's DisconnectNode may be PSIM_NONE.  What keeps a wrong frame from
 * indexing outside a device table: psim_round_absorb copies no unchecked
 * record to the device. */
int psim_record_check(const uint32_t rec[16], const psim_config *cfg);

/* Diagnostic: per node-round kernel of the last round (k_relay, k_shuf,
 * the lite kernel, k_consume, k_ptl, k_pt; this process's first shard; the
 * lite kernel is k_lite_quarter, k_lite_half or k_consume_lite), 4 words
 * each: nodes processed, records delivered, records emitted, 0 -- the
 * kernel's share of the algorithmic bytes (bench.py --kernel-counts,
 * profiles/pmc_record.py).  With cap >= 28 a seventh entry, k_node_prep:
 * the quiet lazy ticks it counted without running their nodes (processed,
 * 0, 0, 0).  With cap >= 32 an eighth: the early part
 * of k_ptl's list (the nodes whose HyParView phase k_relay finished) where it
 * ran apart from the late one -- k_hv_phase's block range, or
 * PSIM_PTL_EARLY=2's launch; zeros where one k_ptl launch ran both parts.
 * The k_ptl entry is the sum of both parts either way.  Returns 6, 7 or 8
 * (0 under the pluggable manager). */
int psim_debug_kernel_counts(psim_handle *h, uint64_t *out, int cap);

/* Per-kernel device time (ms) accumulated over the last psim_step call:
 * names[i] is a static string; returns the number of entries.  A
 * host-exchange handle: over the last round (emit and absorb), the entries
 * k_host_export and k_host_import included (PSIM_PHASE_TIMERS=1). */
int psim_kernel_times(psim_handle *h, const char **names, double *ms, uint64_t *launches, int cap);

/* The cross-shard exchange since psim_create (G > 1: virtual shards or RCCL
 * ranks; this process's shards): *records = records sent to another shard,
 * *bytes = their bytes on the wire -- 32 B a record (dst, src, type word, seq,
 * a0-a2, word 7) plus 32 B for one with exchange ids (nex > 0), against 64 B
 * a record in memory.  A full-strategy handle adds the
 * ORSet rows shipped with its STATE and GOSSIP records to *bytes: fw words a
 * row (fw = ceil(n_nodes / 32) rounded up to 4), 2 fw once a leave/1 removal
 * exists, one row per distinct (snapshot, destination shard) pair of a round.
 * Both 0 on one shard. */
int psim_get_exchange_stats(psim_handle *h, uint64_t *records, uint64_t *bytes);

/* RCCL bootstrap for multi-process sharding (rank 0 creates, all pass it in cfg). */
int psim_comm_id_size(void);
int psim_get_comm_id(void *buf, size_t cap);
/* TEST VEHICLE, not a product backend: the id of a new loopback world
 * (psim_comm_id_size() bytes).  Handles created with it as cfg.comm_id
 * (shard_world = W, shard_rank = r, all on one device, in this process) run
 * the multi-rank code path -- owner partition, count all-to-all, record
 * exchange, stats reduce, leave/1 stop-list gather, overlay gathers -- with
 * device copies and a host barrier in place of RCCL, so it can run where
 * RCCL cannot (one GPU).  The W ranks are W host threads, each making the
 * same calls as RCCL ranks would (collective calls must be concurrent). */
int psim_loopback_comm_id(void *buf, size_t cap);

/* The host boundary: mixed clusters of simulated and outside nodes (DESIGN.md
 * section 7, "The host boundary").  psim_host_comm_id writes the id
 * (psim_comm_id_size() bytes: a magic value, lo, hi) of a host-exchange
 * handle; PSIM_EINVAL for a null or short buffer or lo >= hi.  psim_create
 * with it as cfg.comm_id (shard_world = 1, shard_rank = 0, n_shards <= 1,
 * hi <= n_nodes, else PSIM_EINVAL; the full strategy: PSIM_EUNSUPPORTED)
 * makes a handle that allocates and simulates exactly the nodes [lo, hi);
 * every other id of [0, n_nodes) is outside, and the host speaks for it
 * (lo = 0, hi = n_nodes: nothing is outside -- the boundary's one-party
 * diagnostic).
 *   Events follow the multi-rank rule: the host makes every event call on
 * this handle, those that name outside nodes included (psim_join,
 * psim_revive, psim_crash, psim_leave, psim_set_partition, psim_broadcast,
 * the omission calls, the view-order tables), so an outside node's start,
 * death, partition group and broadcast slots are known here as a remote
 * rank's are.  psim_step, psim_leave_node, psim_get_histograms,
 * psim_get_strategy_histograms and psim_get_graph_metrics answer
 * PSIM_EUNSUPPORTED (the last four need a collective across the parties).
 *   A round is three calls:
 * psim_round_emit    applies the pending events and runs the owned nodes'
 *     round up to its owner partition.  PSIM_ESTATE with a round open,
 *     PSIM_EUNSUPPORTED on any other kind of handle (as the two below).
 * psim_get_outbound  the open round's records addressed outside [lo, hi), 16
 *     words each, in psim_wire_encode's layout (dst, src, type | ttl << 8 |
 *     nex << 16, seq, a0..a3, ex[0..8)): first those for ids below lo, then
 *     those for ids at or above hi, each side in ascending (src, seq) order.
 *     recs == NULL or cap (in records) < *n: only *n is set.  May be called
 *     again.  PSIM_ESTATE with no round open.
 * psim_round_absorb  takes the n records outside nodes sent to owned nodes
 *     this round, in any order: the result does not depend on it, every inbox
 *     is built in the canonical (src, seq) order.  A host that decoded frames
 *     (psim_wire_decode leaves seq = 0) numbers each source's records of the
 *     round in their arrival order: seq = 0, 1, 2, ... per src.  Everything is
 *     checked on the host before any device work, and a rejected call leaves
 *     the handle unchanged, the round still open: a dst outside [lo, hi) or a
 *     src inside it PSIM_ERANGE; a record psim_record_check refuses, its
 *     code; a (src, seq) pair twice in the call PSIM_EINVAL.  On success the
 *     records are routed together with the owned nodes' own, the next inboxes
 *     built and the round closed; *stats (may be NULL) is this handle's share
 *     of the round: the shares of all parties sum to the unsharded round's
 *     stats in every field but `round`.  PSIM_ESTATE with no round open.
 * While a round is open event calls still queue (for the next emit);
 * psim_snapshot, psim_restore and the inspection getters (psim_get_nodes,
 * psim_get_strategy_nodes, psim_get_member_bits, psim_get_delivery) answer
 * PSIM_ESTATE.  Between rounds they behave as on a rank handle; a snapshot
 * restores into a handle created with the same range.
 * psim_get_exchange_stats counts outbound and absorbed records, 64 B each. */
int psim_host_comm_id(void *buf, size_t cap, uint32_t lo, uint32_t hi);
int psim_round_emit(psim_handle *h);
int psim_get_outbound(psim_handle *h, uint32_t *recs, size_t cap, size_t *n);
int psim_round_absorb(psim_handle *h, const uint32_t *recs, size_t n, psim_round_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* PARTISAN_GPU_SIM_H */
