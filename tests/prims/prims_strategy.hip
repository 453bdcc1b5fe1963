// prims_strategy.hip -- test kernels over psim_strategy.hip's primitives: the
// two-register list L2 (ins2, has2, get2), the sets v1 order (add_set2,
// del_set2) and the pluggable wave's uniform_n and sublist.  As
// prims_consume.hip: the product's text is included, this file holds
// __global__ kernels and launchers only, and every launcher checks its cases
// on the host before it launches.
#include "psim_strategy.hip"

#include "prims_host.h"

namespace psim {
namespace primtest {

// op 0 ins2(pos a, e b); 1 has2(e b); 2 get2(i a)
__global__ void tk_l2(RoundArgs, const uint32_t* in, uint32_t* out) {
    const uint32_t l = lane_id();
    const uint32_t* c = in + (size_t)blockIdx.x * L2_IN;
    uint32_t* o = out + (size_t)blockIdx.x * L2_OUT;
    L2 V = {c[L2_V + l], c[L2_V + 64 + l]};
    uint32_t n = c[1], ret = 0;
    if (c[0] == 0) ins2(V, n, c[2], c[3]);
    else if (c[0] == 1) ret = has2(V, n, c[3]) ? 1u : 0u;
    else ret = get2(V, uni(c[2]));
    if (l == 0) { o[0] = n; o[1] = ret; }
    o[2 + l] = V.a; o[2 + 64 + l] = V.b;
}
// a chain of add_set2 / del_set2 (bit 31) from the empty set of 16 slots
__global__ void tk_set2(RoundArgs, const uint32_t* in, uint32_t* out) {
    __shared__ uint32_t lds[128];
    const uint32_t l = lane_id();
    const uint32_t* c = in + (size_t)blockIdx.x * S2_IN;
    const uint32_t nops = c[0];
    uint32_t* o = out + (size_t)blockIdx.x * S2_MAXOPS * S2_SOUT;
    L2 V = {0u, 0u};
    uint32_t n = 0, ns = 16;
    for (uint32_t s = 0; s < nops; s++, o += S2_SOUT) {
        const uint32_t op = c[1 + s];
        if (op >> 31) del_set2(lds, V, n, op & 0x7FFFFFFFu, ns);
        else add_set2(lds, V, n, op, ns);
        if (l == 0) { o[0] = n; o[1] = ns; }
        o[2 + l] = V.a; o[2 + 64 + l] = V.b;
    }
}
#define PW_SETUP()                                                              \
    __shared__ uint32_t lds[128];                                               \
    const uint32_t l = lane_id();                                               \
    const uint32_t* const c = in + (size_t)blockIdx.x * RC_IN;                  \
    uint32_t* const o = out + (size_t)blockIdx.x * RC_OUT;                      \
    Pw w = {};                                                                  \
    w.lds = lds; w.me = c[0];                                                   \
    w.h.rng = (uint64_t)c[1] | ((uint64_t)c[2] << 32);                          \
    w.dc_base = (uint64_t)c[3] | ((uint64_t)c[4] << 32);                        \
    w.DCL = c[RC_DCL + l]; w.DCH = c[RC_DCH + l]
__global__ void tk_pw_uniform(RoundArgs, const uint32_t* in, uint32_t* out) {
    PW_SETUP();
    const uint32_t r = uniform_n(w, c[RC_P]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)w.h.rng; o[2] = (uint32_t)(w.h.rng >> 32); }
}
// V = R0 (entries 0-63), R1 (64-127); n = p0, k = p1
__global__ void tk_pw_sublist(RoundArgs, const uint32_t* in, uint32_t* out) {
    PW_SETUP();
    const L2 V = {c[RC_R0 + l], c[RC_R1 + l]};
    uint32_t OUT = 0;
    const uint32_t r = sublist(w, V, c[RC_P], c[RC_P + 1], OUT);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)w.h.rng; o[2] = (uint32_t)(w.h.rng >> 32); }
    o[RC_ARR + l] = OUT;
}

}  // namespace primtest
}  // namespace psim

using namespace psim;
using namespace psim::primtest;

#define PDOM(...) return prims_edom(__VA_ARGS__)
#define LAUNCHER_HEAD()                                                           \
    if (!prims_cfg_ok(cfg) || !in || !out) PDOM("null argument or table without length"); \
    if (ncases == 0 || ncases > (1u << 22)) PDOM("ncases %u", ncases)

static int run_waves(void (*k)(RoundArgs, const uint32_t*, uint32_t*), const PrimCfg* cfg, const uint32_t* in,
                     uint32_t ncases, size_t iw, uint32_t* out, size_t ow) {
    return prims_run(cfg, in, ncases * iw * 4, out, ncases * ow * 4,
                     [&](const RoundArgs& a, const uint32_t* di, uint32_t* dout) {
                         k<<<dim3(ncases), dim3(64)>>>(a, di, dout);
                     });
}

extern "C" int psim_prims_l2(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD();
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * L2_IN;
        const uint32_t op = c[0], n = c[1], a = c[2];
        if (op > 2 || n > 128) PDOM("case %u: op %u n %u", i, op, n);
        if (op == 0 && (n > 127 || a > n)) PDOM("case %u: ins2 n %u pos %u", i, n, a);
        if (op == 2 && a > 127) PDOM("case %u: get2 of entry %u", i, a);
        for (uint32_t l = n; l < 128; l++)
            if (c[L2_V + l]) PDOM("case %u: entry %u past the count is not 0", i, l);
    }
    return run_waves(tk_l2, cfg, in, ncases, L2_IN, out, L2_OUT);
}
// adds of non-members into fewer than 128 entries; deletes of anything
extern "C" int psim_prims_set2(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD();
    if (ncases > 64) PDOM("ncases %u", ncases);
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * S2_IN;
        if (c[0] > S2_MAXOPS) PDOM("case %u: %u ops", i, c[0]);
        uint32_t v[128], n = 0;
        for (uint32_t s = 0; s < c[0]; s++) {
            const uint32_t e = c[1 + s] & 0x7FFFFFFFu;
            if (!prims_id_ok(cfg, e, false)) PDOM("case %u op %u: id %u past the table", i, s, e);
            uint32_t at = n;
            for (uint32_t j = 0; j < n; j++) if (v[j] == e) at = j;
            if (c[1 + s] >> 31) {
                if (at < n) v[at] = v[--n];
            } else {
                if (e == 0) PDOM("case %u op %u: id 0 is the list's empty entry", i, s);
                if (at < n) PDOM("case %u op %u: add of a member", i, s);
                if (n >= 128) PDOM("case %u op %u: add into a full list", i, s);
                v[n++] = e;
            }
        }
    }
    return run_waves(tk_set2, cfg, in, ncases, S2_IN, out, (size_t)S2_MAXOPS * S2_SOUT);
}
extern "C" int psim_prims_pw_uniform(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD();
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * RC_IN;
        if (c[RC_P] < 1 || c[RC_P] > 65535) PDOM("case %u: n %u outside [1, 65535]", i, c[RC_P]);
        for (uint32_t l = 0; l < 64; l++)
            if (c[RC_DCH + l] >> 26) PDOM("case %u: cached draw %u is no 58-bit value", i, l);
    }
    return run_waves(tk_pw_uniform, cfg, in, ncases, RC_IN, out, RC_OUT);
}
extern "C" int psim_prims_pw_sublist(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD();
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * RC_IN;
        if (c[RC_P] > 128 || c[RC_P + 1] > 64) PDOM("case %u: n %u k %u", i, c[RC_P], c[RC_P + 1]);
    }
    return run_waves(tk_pw_sublist, cfg, in, ncases, RC_IN, out, RC_OUT);
}
