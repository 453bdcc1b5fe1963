/*
 * tests/nif_run/psim_on_oracle.c -- TEST INFRASTRUCTURE ONLY: the psim_*
 * entry points the NIF shim calls, forwarded to the CPU oracle's orc_*
 * exports (oracle/psim_oracle.c, compiled into the same program), so that
 * the shim can run where there is no GPU.  Not a mock: every protocol call
 * goes into the real oracle.  What the oracle lacks answers
 * PSIM_EUNSUPPORTED: snapshot, restore, the strategy histograms, the graph
 * metrics, the host comm id.  On a GPU the program links
 * libpartisan_gpu_sim.so instead of this file.
 */
#include <string.h>

#include "partisan_gpu_sim.h"

void orc_default_config(psim_config *cfg);
int orc_create(const psim_config *cfg, psim_handle **out);
void orc_destroy(psim_handle *h);
int orc_join(psim_handle *h, const uint32_t *nodes, const uint32_t *contacts, size_t n);
int orc_crash(psim_handle *h, const uint32_t *nodes, size_t n);
int orc_revive(psim_handle *h, const uint32_t *nodes, size_t n);
int orc_leave(psim_handle *h, const uint32_t *nodes, size_t n);
int orc_leave_node(psim_handle *h, const uint32_t *actors, const uint32_t *targets, size_t n);
int orc_set_partition(psim_handle *h, const uint8_t *group, size_t n);
int orc_clear_partition(psim_handle *h);
int orc_set_bucket_table(psim_handle *h, const uint8_t *buckets, size_t n);
int orc_set_phash_table(psim_handle *h, const uint32_t *phash, size_t n);
int orc_set_omission(psim_handle *h, int kind, const uint32_t *src, const uint32_t *dst, size_t n, int on);
int orc_set_faulted(psim_handle *h, const uint32_t *nodes, size_t n, int on);
int orc_clear_faults(psim_handle *h);
int orc_broadcast(psim_handle *h, uint32_t root, uint32_t msg_id);
int orc_step(psim_handle *h, uint32_t n_rounds, psim_round_stats *stats);
int orc_get_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_node_view *out);
int orc_get_round(psim_handle *h, uint64_t *round);
int orc_get_strategy_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_strategy_view *out);
int orc_get_member_bits(psim_handle *h, uint32_t node, uint32_t *words, size_t n_words);
int orc_get_delivery(psim_handle *h, uint32_t first, uint32_t count, uint8_t *have, uint32_t *round, uint32_t *hop);
int orc_get_histograms(psim_handle *h, psim_histograms *out);
int orc_get_msg_slots(psim_handle *h, uint32_t *ids, uint32_t *roots, size_t cap);
int orc_round_emit(psim_handle *h, psim_round_stats *st);
int orc_get_outbox(psim_handle *h, uint32_t *out, size_t cap, size_t *n);
int orc_round_absorb(psim_handle *h, const uint32_t *recs, size_t n);

/* restated from the library (the oracle has neither) */
const char *psim_strerror(int code) {
    switch (code) {
    case PSIM_OK: return "ok";
    case PSIM_EINVAL: return "invalid argument";
    case PSIM_ENOMEM: return "out of memory";
    case PSIM_EDEVICE: return "HIP runtime error";
    case PSIM_ESTATE: return "invalid state";
    case PSIM_ERANGE: return "node id out of range";
    case PSIM_ECOMM: return "communication error";
    case PSIM_EUNSUPPORTED: return "unsupported";
    case PSIM_ECAPACITY: return "a fixed table overflowed (strict)";
    default: return "unknown error";
    }
}
int psim_abi_version(void) { return PSIM_ABI_VERSION; }

void psim_default_config(psim_config *cfg) { orc_default_config(cfg); }
int psim_create(const psim_config *cfg, psim_handle **out) { return orc_create(cfg, out); }
static void forget_open_round(psim_handle *h);
void psim_destroy(psim_handle *h) { forget_open_round(h); orc_destroy(h); }
int psim_join(psim_handle *h, const uint32_t *nodes, const uint32_t *contacts, size_t n) { return orc_join(h, nodes, contacts, n); }
int psim_crash(psim_handle *h, const uint32_t *nodes, size_t n) { return orc_crash(h, nodes, n); }
int psim_revive(psim_handle *h, const uint32_t *nodes, size_t n) { return orc_revive(h, nodes, n); }
int psim_leave(psim_handle *h, const uint32_t *nodes, size_t n) { return orc_leave(h, nodes, n); }
int psim_leave_node(psim_handle *h, const uint32_t *a, const uint32_t *t, size_t n) { return orc_leave_node(h, a, t, n); }
int psim_set_partition(psim_handle *h, const uint8_t *group, size_t n) { return orc_set_partition(h, group, n); }
int psim_clear_partition(psim_handle *h) { return orc_clear_partition(h); }
int psim_set_bucket_table(psim_handle *h, const uint8_t *b, size_t n) { return orc_set_bucket_table(h, b, n); }
int psim_set_phash_table(psim_handle *h, const uint32_t *p, size_t n) { return orc_set_phash_table(h, p, n); }
int psim_set_omission(psim_handle *h, int kind, const uint32_t *src, const uint32_t *dst, size_t n, int on) {
    return orc_set_omission(h, kind, src, dst, n, on);
}
int psim_set_faulted(psim_handle *h, const uint32_t *nodes, size_t n, int on) { return orc_set_faulted(h, nodes, n, on); }
int psim_clear_faults(psim_handle *h) { return orc_clear_faults(h); }
int psim_broadcast(psim_handle *h, uint32_t root, uint32_t msg_id) { return orc_broadcast(h, root, msg_id); }
int psim_step(psim_handle *h, uint32_t n_rounds, psim_round_stats *stats) { return orc_step(h, n_rounds, stats); }
int psim_get_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_node_view *out) {
    return orc_get_nodes(h, first, count, out);
}
int psim_get_round(psim_handle *h, uint64_t *round) { return orc_get_round(h, round); }
int psim_get_strategy_nodes(psim_handle *h, uint32_t first, uint32_t count, psim_strategy_view *out) {
    return orc_get_strategy_nodes(h, first, count, out);
}
int psim_get_member_bits(psim_handle *h, uint32_t node, uint32_t *words, size_t n_words) {
    return orc_get_member_bits(h, node, words, n_words);
}
int psim_get_delivery(psim_handle *h, uint32_t first, uint32_t count, uint8_t *have, uint32_t *round, uint32_t *hop) {
    return orc_get_delivery(h, first, count, have, round, hop);
}
int psim_get_histograms(psim_handle *h, psim_histograms *out) { return orc_get_histograms(h, out); }
int psim_get_msg_slots(psim_handle *h, uint32_t *ids, uint32_t *roots, size_t cap) {
    return orc_get_msg_slots(h, ids, roots, cap);
}

/* The oracle's round halves (its sharded protocol): the stats of a round are
 * complete after the emit half, which wants them at once; they are kept here
 * until the absorb half hands them out, as psim_round_absorb does. */
#define OPEN_CAP 16
static struct { psim_handle *h; psim_round_stats st; } open_round[OPEN_CAP];

static void forget_open_round(psim_handle *h) {
    for (int i = 0; i < OPEN_CAP; i++)
        if (open_round[i].h == h) open_round[i].h = NULL;
}

int psim_round_emit(psim_handle *h) {
    int k = -1;
    for (int i = 0; i < OPEN_CAP; i++) {
        if (open_round[i].h == h) return PSIM_ESTATE;          /* a round is open */
        if (!open_round[i].h && k < 0) k = i;
    }
    if (k < 0) return PSIM_ENOMEM;
    int rc = orc_round_emit(h, &open_round[k].st);
    if (!rc) open_round[k].h = h;
    return rc;
}

int psim_get_outbound(psim_handle *h, uint32_t *recs, size_t cap, size_t *n) {
    int open = 0;
    for (int i = 0; i < OPEN_CAP; i++) open |= open_round[i].h == h;
    if (!open) return PSIM_ESTATE;
    size_t have = 0;
    orc_get_outbox(h, NULL, 0, &have);
    *n = have;
    if (!recs || cap < have) return PSIM_OK;
    return orc_get_outbox(h, recs, cap, n);
}

int psim_round_absorb(psim_handle *h, const uint32_t *recs, size_t n, psim_round_stats *stats) {
    for (int i = 0; i < OPEN_CAP; i++)
        if (open_round[i].h == h) {
            int rc = orc_round_absorb(h, recs, n);
            if (rc == PSIM_ERANGE) return rc;                   /* refused: the round stays open */
            if (!rc && stats) *stats = open_round[i].st;
            open_round[i].h = NULL;
            return rc;
        }
    return PSIM_ESTATE;
}

int psim_snapshot(psim_handle *h, void *buf, size_t cap, size_t *need) { return PSIM_EUNSUPPORTED; }
int psim_restore(psim_handle *h, const void *buf, size_t size) { return PSIM_EUNSUPPORTED; }
int psim_get_strategy_histograms(psim_handle *h, psim_strategy_histograms *out) { return PSIM_EUNSUPPORTED; }
int psim_get_graph_metrics(psim_handle *h, const uint32_t *sources, size_t n_sources, uint32_t max_levels,
                           psim_graph_metrics *out) {
    return PSIM_EUNSUPPORTED;
}
int psim_comm_id_size(void) { return 128; }
int psim_host_comm_id(void *buf, size_t cap, uint32_t lo, uint32_t hi) { return PSIM_EUNSUPPORTED; }
