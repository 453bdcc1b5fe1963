// prims_host.h -- host side shared by the two TUs of the test-only module
// libpsim_prims_test.so (tests/_prims.py loads it): the launch configuration,
// the copy-in / launch once / synchronise / copy-out runner, and the domain
// error reporting.  Host code only: every device function the test kernels
// call is the product's own text, included by the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "psim_kernels.h"

// what a test kernel sees through kargs(): the fields below, everything else null
struct PrimCfg {
    uint64_t seed;
    uint32_t max_passive, max_active, k_active, k_passive;
    const uint8_t* btab;        // host bytes, or null for the default hash
    uint64_t btab_len;          // ids a case may name when btab is set
};

// One case of a kernel that runs on a node's draw counter ("RC" layout), in
// 32-bit words: me, rng lo/hi, draw-cache base lo/hi (~0: empty), p[0..10],
// then five 64-word lane arrays: the cache's low and high words, R0, R1, R2.
// Its output: eight scalars and one 64-word lane array.
enum : uint32_t { RC_P = 5, RC_DCL = 16, RC_DCH = 80, RC_R0 = 144, RC_R1 = 208, RC_R2 = 272, RC_IN = 336,
                  RC_OUT = 72, RC_ARR = 8 };
// a Pas<W>::step chain: n0, 32 ids, then 64 steps of (id, k or ~0: no
// eviction); after every step 32 ids, n, dirty
enum : uint32_t { PS_ROW = 1, PS_STEPS = 33, PS_NSTEP = 64, PS_IN = PS_STEPS + 2 * PS_NSTEP, PS_SOUT = 34,
                  PS_OUT = PS_NSTEP * PS_SOUT };
// a 32-bit / 64-bit wave list case: op, n, a, b, (b's high word,) the list;
// its output n, the return value, the list
enum : uint32_t { L32_V = 4, L32_IN = 68, L32_OUT = 66, L64_V = 5, L64_IN = 5 + 128, L64_OUT = 2 + 128 };
// a two-register list case (psim_strategy.hip L2): op, n, a, b, 128 entries
enum : uint32_t { L2_V = 4, L2_IN = 4 + 128, L2_OUT = 2 + 128 };
// a sets v1 chain: the count, then up to S2_MAXOPS ops (bit 31: delete);
// after every op n, ns and the 128 entries
enum : uint32_t { S2_MAXOPS = 400, S2_IN = 1 + S2_MAXOPS, S2_SOUT = 130 };

constexpr int PRIMS_EDOM = -22;      // a case outside the primitive's domain: nothing launched

inline char* prims_err_buf() {
    static thread_local char buf[256];
    return buf;
}
inline int prims_edom(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(prims_err_buf(), 256, fmt, ap);
    va_end(ap);
    return PRIMS_EDOM;
}

struct PrimsDev {
    void* p = nullptr;
    ~PrimsDev() { if (p) (void)hipFree(p); }
};

// copies `in` and the table in, calls launch(args, in, out) once,
// synchronises, copies `out` back; returns the first HIP error code
template <class L>
int prims_run(const PrimCfg* cfg, const void* in, size_t in_bytes, void* out, size_t out_bytes, L launch) {
    PrimsDev din, dout, dtab;
    hipError_t e;
    if ((e = hipMalloc(&din.p, in_bytes ? in_bytes : 4)) != hipSuccess) return (int)e;
    if ((e = hipMalloc(&dout.p, out_bytes ? out_bytes : 4)) != hipSuccess) return (int)e;
    if (in_bytes && (e = hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if ((e = hipMemset(dout.p, 0, out_bytes ? out_bytes : 4)) != hipSuccess) return (int)e;
    psim::RoundArgs a = {};
    a.seed = cfg->seed;
    a.max_passive = cfg->max_passive; a.max_active = cfg->max_active;
    a.k_active = cfg->k_active; a.k_passive = cfg->k_passive;
    if (cfg->btab) {
        if ((e = hipMalloc(&dtab.p, cfg->btab_len)) != hipSuccess) return (int)e;
        if ((e = hipMemcpy(dtab.p, cfg->btab, cfg->btab_len, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
        a.btab = static_cast<const uint8_t*>(dtab.p);
    }
    launch(a, static_cast<const uint32_t*>(din.p), static_cast<uint32_t*>(dout.p));
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
    if (out_bytes && (e = hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    return 0;
}

// an id a kernel may hash: below 2^27 where tags are used, and inside the table
inline bool prims_id_ok(const PrimCfg* cfg, uint32_t id, bool tagged) {
    if (tagged && id >= (1u << 27)) return false;
    return !cfg->btab || id < cfg->btab_len;
}
inline uint32_t prims_bucket(const PrimCfg* cfg, uint32_t id) {
    return cfg->btab ? cfg->btab[id] & 15u : psim::bucket16_default(id);
}
inline bool prims_cfg_ok(const PrimCfg* cfg) {
    return cfg && (cfg->btab == nullptr) == (cfg->btab_len == 0);
}
