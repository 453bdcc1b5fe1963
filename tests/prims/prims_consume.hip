// prims_consume.hip -- test kernels over the device primitives of
// psim_device.h, psim_wave.h, psim_lite.h and psim_consume.hip, one
// primitive a kernel.  The product's text is *included*, never copied: this
// file holds __global__ kernels and their extern "C" launchers only
// (tests/test_prims_models.py greps for anything else).
//
// Every kernel takes a RoundArgs first, because the product's kargs() reads
// the start of the kernarg segment as one.  A block is one wave.  A wave
// carries as many cases as the primitive has lane groups (1, 2 halves, 4
// rows), case N * block + group, and every cross-lane read runs with its
// whole group active: control flow diverges between groups only.
// Every launcher checks its cases against the primitive's domain on the host
// and returns PRIMS_EDOM without launching: a wrong test parameter never
// indexes past LDS or a buffer.
#include "psim_consume.hip"

#include "prims_host.h"

namespace psim {
namespace primtest {

#define RC_CASE(ci) const uint32_t* const c = in + (size_t)(ci) * RC_IN; uint32_t* const o = out + (size_t)(ci) * RC_OUT
#define RC_U64(c, i) ((uint64_t)(c)[i] | ((uint64_t)(c)[(i) + 1] << 32))
// a wave's Wv, field by field (no load path runs)
#define WV_SETUP()                                                              \
    __shared__ uint32_t lds[64];                                                \
    const uint32_t l = lane_id();                                               \
    RC_CASE(blockIdx.x);                                                        \
    Wv w = {};                                                                  \
    w.lds = lds; w.me = c[0]; w.rng = RC_U64(c, 1); w.dc_base = RC_U64(c, 3);   \
    w.DCL = c[RC_DCL + l]; w.DCH = c[RC_DCH + l]; w.KM = magic_lanes()
// a group's lite::Node<W> and lite::Lds<W>
#define LITE_SETUP()                                                            \
    using G = lite::Grp<W>;                                                     \
    __shared__ uint32_t lds[G::N * G::SCR];                                     \
    const uint32_t l = G::lane();                                               \
    RC_CASE(blockIdx.x * G::N + G::idx());                                      \
    lite::Node<W> x = {};                                                       \
    x.me = c[0]; x.rng = RC_U64(c, 1); x.dcb = RC_U64(c, 3);                    \
    x.DCL = c[RC_DCL + l]; x.DCH = c[RC_DCH + l];                               \
    lite::Lds<W> w = {};                                                        \
    w.scr = lds + G::idx() * G::SCR; w.KM = G::magic_lanes()
#define PAS_SET(x, n)                                                                       \
    do {                                                                                    \
        if constexpr (W == 32) (x).pas.set(c[RC_R0 + l], (n));                              \
        else (x).pas.set(make_uint2(c[RC_R0 + 2 * l], c[RC_R0 + 2 * l + 1]), (n));          \
        (x).pas_n = (n);                                                                    \
    } while (0)
#define PAS_OUT(p, o)                                                                       \
    do {                                                                                    \
        if constexpr (W == 32) (o)[l] = (p).P;                                              \
        else { (o)[2 * l] = (p).P0; (o)[2 * l + 1] = (p).P1; }                              \
    } while (0)

// ------------------------------------------------------- per-thread ones --
__global__ void tk_philox(RoundArgs, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = in + (size_t)i * 6;
    uint32_t o0, o1;
    philox(c[0], c[1], c[2], c[3], c[4], c[5], o0, o1);
    out[2 * i] = o0; out[2 * i + 1] = o1;
}
__global__ void tk_draw58(RoundArgs, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = in + (size_t)i * 5;
    const uint64_t v = draw58_at(RC_U64(c, 0), c[2], RC_U64(c, 3));
    out[2 * i] = (uint32_t)v; out[2 * i + 1] = (uint32_t)(v >> 32);
}
// (v lo, v hi, n, which): 0 mod_small, 1 mod58
__global__ void tk_mod(RoundArgs, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = in + (size_t)i * 4;
    out[i] = c[3] ? mod58(RC_U64(c, 0), c[2]) : mod_small(RC_U64(c, 0), c[2]);
}
// (id, ns)
__global__ void tk_set_slot(RoundArgs, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    out[i] = set_slot(kargs().btab, in[2 * i], in[2 * i + 1]);
}

// One Horner step of mod_small_m, x - mul_hi(x, M) * n, against the
// compiler's x % n for every x < n * 2^20, with M fetched as the product
// fetches it -- mode 0: kMagic[n]; 1: rl(magic_lanes(), n & 63); 2:
// Grp<32>::magic; 3: Grp<16>::magic.  Block (bx, by): group g takes
// n = n_lo + (by + 7 g) mod (n_hi - n_lo + 1), a different n in each group of
// the wave, and the x of chunk bx.  res[n]: M; res[128 + 2 n], [.. + 1]:
// mismatches and compares, 64-bit.
template <uint32_t W>
__global__ void tk_modstep(RoundArgs, const uint32_t*, uint32_t* res, uint32_t mode, uint32_t n_lo, uint32_t n_hi) {
    using G = lite::GrpBase<W>;
    const uint32_t n = n_lo + (blockIdx.y + 7 * G::idx()) % (n_hi - n_lo + 1);
    uint32_t M;
    if constexpr (W == 64) {
        const uint32_t KM = magic_lanes();
        M = mode == 0 ? kMagic[n] : rl(KM, uni(n) & 63);
    } else {
        const typename lite::Grp<W>::Magic KM = lite::Grp<W>::magic_lanes();
        M = lite::Grp<W>::magic(KM, n);
    }
    unsigned long long bad = 0, cnt = 0;
    if (n >= 2) {
        const uint32_t end = n << 20;
        for (uint32_t x = blockIdx.x * W + G::lane(); x < end; x += gridDim.x * W) {
            bad += (x - __umulhi(x, M) * n) != x % n ? 1u : 0u;
            cnt++;
        }
    }
    unsigned long long* const r64 = reinterpret_cast<unsigned long long*>(res + 128);
    if (bad) atomicAdd(&r64[2 * n], bad);
    atomicAdd(&r64[2 * n + 1], cnt);
    if (blockIdx.x == 0 && G::lane() == 0) res[n] = M;
}

// ------------------------------------------------------------ wave lists --
__global__ void tk_wave_min(RoundArgs, const uint32_t* in, uint32_t* out) {
    const uint32_t r = wave_min(in[blockIdx.x * 64 + lane_id()]);
    if (lane_id() == 0) out[blockIdx.x] = r;
}
// op 0 vins(pos a, e b); 1 vdel(k a); 2 vdel_val(e b); 3 view_add(e b);
// 4 has(e b); 5 idx_of(e b)
__global__ void tk_list32(RoundArgs, const uint32_t* in, uint32_t* out) {
    const uint32_t l = lane_id();
    const uint32_t* c = in + (size_t)blockIdx.x * L32_IN;
    uint32_t* o = out + (size_t)blockIdx.x * L32_OUT;
    const uint32_t op = c[0], a = c[2], b = c[3];
    uint32_t n = c[1], V = c[L32_V + l], ret = 0;
    if (op == 0) vins(V, n, a, b);
    else if (op == 1) vdel(V, n, a);
    else if (op == 2) ret = vdel_val(V, n, b) ? 1u : 0u;
    else if (op == 3) view_add(kargs().btab, V, n, b);
    else if (op == 4) ret = has(V, n, b) ? 1u : 0u;
    else ret = (uint32_t)idx_of(V, n, b);
    if (l == 0) { o[0] = n; o[1] = ret; }
    o[2 + l] = V;
}
// op 0 vins64(pos a, e); 1 vdel64(k a)
__global__ void tk_list64(RoundArgs, const uint32_t* in, uint32_t* out) {
    const uint32_t l = lane_id();
    const uint32_t* c = in + (size_t)blockIdx.x * L64_IN;
    uint32_t* o = out + (size_t)blockIdx.x * L64_OUT;
    uint32_t n = c[1];
    uint64_t V = (uint64_t)c[L64_V + l] | ((uint64_t)c[L64_V + 64 + l] << 32);
    if (c[0] == 0) vins64(V, n, c[2], RC_U64(c, 3));
    else vdel64(V, n, c[2]);
    if (l == 0) { o[0] = n; o[1] = 0; }
    o[2 + l] = (uint32_t)V; o[2 + 64 + l] = (uint32_t)(V >> 32);
}

// ------------------------------------------------------ the wave's (Wv) --
// p0 = 0: usort_mask(E = R0, p1 | p2 << 32); 1: usort_lanes(E, p1)
__global__ void tk_wv_usort(RoundArgs, const uint32_t* in, uint32_t* out) {
    WV_SETUP();
    uint32_t E = c[RC_R0 + l];
    const uint32_t r = c[RC_P] == 0 ? usort_mask(w, E, RC_U64(c, RC_P + 1)) : usort_lanes(w, E, c[RC_P + 1]);
    if (l == 0) o[0] = r;
    o[RC_ARR + l] = E;
}
__global__ void tk_wv_uniform(RoundArgs, const uint32_t* in, uint32_t* out) {
    WV_SETUP();
    const uint32_t r = uniform_n(w, c[RC_P]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)w.rng; o[2] = (uint32_t)(w.rng >> 32); }
}
// V = R0, n = p0, omitted ids p1..p3
__global__ void tk_wv_select(RoundArgs, const uint32_t* in, uint32_t* out) {
    WV_SETUP();
    const uint32_t r = select_random(w, c[RC_R0 + l], c[RC_P], c[RC_P + 1], c[RC_P + 2], c[RC_P + 3]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)w.rng; o[2] = (uint32_t)(w.rng >> 32); }
}
// V = R0, n = p0, k = p1, on = p2, OUT = R2
__global__ void tk_wv_sublist(RoundArgs, const uint32_t* in, uint32_t* out) {
    WV_SETUP();
    uint32_t OUT = c[RC_R2 + l];
    const uint32_t r = sublist(w, c[RC_R0 + l], c[RC_P], c[RC_P + 1], OUT, c[RC_P + 2]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)w.rng; o[2] = (uint32_t)(w.rng >> 32); }
    o[RC_ARR + l] = OUT;
}
// passive = R0 (pas_n = p1), active = R1 (act_n = p0), EX = R2 (nex = p2)
__global__ void tk_wv_merge(RoundArgs, const uint32_t* in, uint32_t* out) {
    WV_SETUP();
    w.act_n = c[RC_P]; w.pas_n = c[RC_P + 1];
    w.A = l < w.act_n ? c[RC_R1 + l] : 0u;
    w.P = l < w.pas_n ? c[RC_R0 + l] : 0u;
    const uint32_t nex = c[RC_P + 2];
    merge_exchange(w, l < nex ? c[RC_R2 + l] : 0u, nex);
    if (l == 0) { o[0] = w.pas_n; o[1] = (uint32_t)w.rng; o[2] = (uint32_t)(w.rng >> 32); o[3] = (w.vd >> 1) & 1u; }
    o[RC_ARR + l] = w.P;
}

// ------------------------------------------------ the lane groups' (lite) --
// E = R0's lanes 0-7, valid = bit l of p0
template <uint32_t W>
__global__ void tk_lite_usort(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    uint32_t E = c[RC_R0 + l];
    const uint32_t r = lite::usort(w, E, l < 8 && ((c[RC_P] >> l) & 1u));
    if (l == 0) o[0] = r;
    o[RC_ARR + l] = E;
}
template <uint32_t W>
__global__ void tk_lite_uniform(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    const uint32_t r = lite::uniform_n(x, w, c[RC_P]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)x.rng; o[2] = (uint32_t)(x.rng >> 32); }
}
template <uint32_t W>
__global__ void tk_lite_select(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    const uint32_t r = lite::select_random(x, w, c[RC_R0 + l], c[RC_P], c[RC_P + 1], c[RC_P + 2]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)x.rng; o[2] = (uint32_t)(x.rng >> 32); }
}
// the one-entry-a-lane sublist: V = R0, n = p0, k = p1, on = p2, OUT = R2
template <int MAXN, uint32_t W>
__global__ void tk_lite_sublist(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    uint32_t OUT = c[RC_R2 + l];
    const uint32_t r = lite::sublist<MAXN>(x, w, c[RC_R0 + l], c[RC_P], c[RC_P + 1], OUT, c[RC_P + 2]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)x.rng; o[2] = (uint32_t)(x.rng >> 32); }
    o[RC_ARR + l] = OUT;
}
// the passive view's: Pas<32> one entry a lane, Pas<16> two (Philox in place)
template <uint32_t W>
__global__ void tk_pas_sublist(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    PAS_SET(x, c[RC_P]);
    uint32_t OUT = c[RC_R2 + l];
    const uint32_t r = lite::Pas<W>::sublist(x, w, c[RC_P + 1], OUT, c[RC_P + 2]);
    if (l == 0) { o[0] = r; o[1] = (uint32_t)x.rng; o[2] = (uint32_t)(x.rng >> 32); }
    o[RC_ARR + l] = OUT;
}
// passive = R0 (pas_n = p1), active = R1 (act_n = p0), EX = R2 (nex = p2), sorted = p3
template <uint32_t W>
__global__ void tk_lite_merge(RoundArgs, const uint32_t* in, uint32_t* out) {
    LITE_SETUP();
    x.act_n = c[RC_P];
    x.A = l < x.act_n ? c[RC_R1 + l] : 0u;
    PAS_SET(x, c[RC_P + 1]);
    const uint32_t nex = c[RC_P + 2];
    lite::merge_exchange(x, w, l < nex ? c[RC_R2 + l] : 0u, nex, c[RC_P + 3] != 0);
    if (l == 0) {
        o[0] = x.pas_n; o[1] = (uint32_t)x.rng; o[2] = (uint32_t)(x.rng >> 32);
        o[3] = (x.fl & lite::HF_PDIRTY) ? 1u : 0u;
    }
    PAS_OUT(x.pas, o + RC_ARR);
}
// a chain of Pas<W>::step on the tagged view
template <uint32_t W>
__global__ void tk_pas_step(RoundArgs, const uint32_t* in, uint32_t* out, uint32_t nstep) {
    using G = lite::Grp<W>;
    const uint32_t l = G::lane();
    const size_t ci = blockIdx.x * G::N + G::idx();
    const uint32_t* const c = in + ci * PS_IN;
    uint32_t* o = out + ci * PS_OUT;
    const uint8_t* bt = kargs().btab;
    uint32_t n = c[0], dirty = 0;
    lite::Pas<W> p;
    if constexpr (W == 32) p.set(c[PS_ROW + l], n);
    else p.set(make_uint2(c[PS_ROW + 2 * l], c[PS_ROW + 2 * l + 1]), n);
    lite::Pas<W> pt = p.tagged(bt, n);
    for (uint32_t s = 0; s < nstep; s++, o += PS_SOUT) {
        const uint32_t id = c[PS_STEPS + 2 * s], evk = c[PS_STEPS + 2 * s + 1];
        const uint32_t tt = lite::tag_of(bt, id, true);
        const bool mem = pt.has(tt);
        const bool ev = !mem && evk != 0xFFFFFFFFu;
        pt.step(n, dirty, tt, mem, ev, ev ? evk : 0u);
        const lite::Pas<W> u = pt.untagged();
        PAS_OUT(u, o);
        if (l == 0) { o[32] = n; o[33] = dirty; }
    }
}

}  // namespace primtest
}  // namespace psim

// ------------------------------------------------------------ launchers --
using namespace psim;
using namespace psim::primtest;

#define PDOM(...) return prims_edom(__VA_ARGS__)
#define LAUNCHER_HEAD(words)                                                      \
    if (!prims_cfg_ok(cfg) || !in || !out) PDOM("null argument or table without length"); \
    if (ncases == 0 || ncases > (1u << 22)) PDOM("ncases %u", ncases);            \
    const size_t in_words = (words)

extern "C" int psim_prims_abi() { return PSIM_ABI_VERSION; }
extern "C" const char* psim_prims_last_error() { return prims_err_buf(); }

static int run_threads(void (*k)(RoundArgs, const uint32_t*, uint32_t*, uint32_t), const PrimCfg* cfg,
                       const uint32_t* in, uint32_t ncases, uint32_t iw, uint32_t* out, uint32_t ow) {
    return prims_run(cfg, in, (size_t)ncases * iw * 4, out, (size_t)ncases * ow * 4,
                     [&](const RoundArgs& a, const uint32_t* di, uint32_t* dout) {
                         k<<<dim3((ncases + 63) / 64), dim3(64)>>>(a, di, dout, ncases);
                     });
}
static int run_waves(void (*k)(RoundArgs, const uint32_t*, uint32_t*), const PrimCfg* cfg, const uint32_t* in,
                     uint32_t ncases, uint32_t groups, uint32_t iw, uint32_t* out, uint32_t ow) {
    if (ncases % groups) return prims_edom("ncases %u is no multiple of the wave's %u groups", ncases, groups);
    return prims_run(cfg, in, (size_t)ncases * iw * 4, out, (size_t)ncases * ow * 4,
                     [&](const RoundArgs& a, const uint32_t* di, uint32_t* dout) {
                         k<<<dim3(ncases / groups), dim3(64)>>>(a, di, dout);
                     });
}

extern "C" int psim_prims_philox(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(6);
    return run_threads(tk_philox, cfg, in, ncases, in_words, out, 2);
}
extern "C" int psim_prims_draw58(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(5);
    return run_threads(tk_draw58, cfg, in, ncases, in_words, out, 2);
}
extern "C" int psim_prims_mod(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(4);
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * 4;
        if ((c[1] >> 26) != 0) PDOM("case %u: v is no 58-bit value", i);
        if (c[3] > 1) PDOM("case %u: which %u", i, c[3]);
        if (c[2] < 1 || c[2] > (c[3] ? 65535u : 64u)) PDOM("case %u: n %u outside the function's range", i, c[2]);
    }
    return run_threads(tk_mod, cfg, in, ncases, in_words, out, 1);
}
extern "C" int psim_prims_set_slot(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(2);
    for (uint32_t i = 0; i < ncases; i++) {
        if (!prims_id_ok(cfg, in[2 * i], false)) PDOM("case %u: id %u past the table", i, in[2 * i]);
        if (in[2 * i + 1] < 16 || in[2 * i + 1] > 256) PDOM("case %u: ns %u", i, in[2 * i + 1]);
    }
    return run_threads(tk_set_slot, cfg, in, ncases, in_words, out, 1);
}

// res: 128 words of M, then 128 pairs of 64-bit (mismatches, compares)
extern "C" int psim_prims_modstep(const PrimCfg* cfg, uint32_t mode, uint32_t n_lo, uint32_t n_hi, uint32_t* res) {
    if (!prims_cfg_ok(cfg) || !res) PDOM("null argument");
    if (mode > 3) PDOM("mode %u", mode);
    const uint32_t cap = mode >= 2 ? 31u : 64u;      // Grp<W>::magic: n in [1, 31]
    if (n_lo < 1 || n_lo > n_hi || n_hi > cap) PDOM("n range [%u, %u] outside [1, %u]", n_lo, n_hi, cap);
    const uint32_t span = n_hi - n_lo + 1;
    return prims_run(cfg, nullptr, 0, res, (128 + 4 * 128) * 4,
                     [&](const RoundArgs& a, const uint32_t* di, uint32_t* dout) {
                         const dim3 grid(256, span);
                         if (mode <= 1) tk_modstep<64><<<grid, dim3(64)>>>(a, di, dout, mode, n_lo, n_hi);
                         else if (mode == 2) tk_modstep<32><<<grid, dim3(64)>>>(a, di, dout, mode, n_lo, n_hi);
                         else tk_modstep<16><<<grid, dim3(64)>>>(a, di, dout, mode, n_lo, n_hi);
                     });
}

extern "C" int psim_prims_wave_min(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(64);
    return run_waves(tk_wave_min, cfg, in, ncases, 1, in_words, out, 1);
}
extern "C" int psim_prims_list32(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(L32_IN);
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * L32_IN;
        const uint32_t op = c[0], n = c[1], a = c[2];
        if (op > 5 || n > 64) PDOM("case %u: op %u n %u", i, op, n);
        if ((op == 0 || op == 3) && n > 63) PDOM("case %u: insert into a full register", i);
        if (op == 0 && a > n) PDOM("case %u: pos %u > n %u", i, a, n);
        if (op == 1 && a >= n) PDOM("case %u: k %u >= n %u", i, a, n);
        for (uint32_t l = 0; l < 64; l++) {
            if (l >= n && c[L32_V + l] != 0) PDOM("case %u: lane %u past the count is not 0", i, l);
            if (op == 3 && !prims_id_ok(cfg, c[L32_V + l], false)) PDOM("case %u: id past the table", i);
        }
        if (op == 3 && !prims_id_ok(cfg, c[3], false)) PDOM("case %u: id past the table", i);
    }
    return run_waves(tk_list32, cfg, in, ncases, 1, in_words, out, L32_OUT);
}
extern "C" int psim_prims_list64(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(L64_IN);
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * L64_IN;
        const uint32_t op = c[0], n = c[1], a = c[2];
        if (op > 1 || n > 64) PDOM("case %u: op %u n %u", i, op, n);
        if (op == 0 && (n > 63 || a > n)) PDOM("case %u: vins64 n %u pos %u", i, n, a);
        if (op == 1 && a >= n) PDOM("case %u: k %u >= n %u", i, a, n);
        for (uint32_t l = n; l < 64; l++)
            if (c[L64_V + l] || c[L64_V + 64 + l]) PDOM("case %u: lane %u past the count is not 0", i, l);
    }
    return run_waves(tk_list64, cfg, in, ncases, 1, in_words, out, L64_OUT);
}

// the RC cases' common checks: the draw cache, n against its register
static int rc_check(const PrimCfg* cfg, const uint32_t* c, uint32_t i) {
    if (c[0] >= (1u << 27)) return prims_edom("case %u: me %u", i, c[0]);
    for (uint32_t l = 0; l < 64; l++)
        if (c[RC_DCH + l] >> 26) return prims_edom("case %u: cached draw %u is no 58-bit value", i, l);
    (void)cfg;
    return 0;
}
#define RC_CHECKS(body)                                                           \
    for (uint32_t i = 0; i < ncases; i++) {                                       \
        const uint32_t* c = in + (size_t)i * RC_IN;                               \
        if (int e = rc_check(cfg, c, i)) return e;                                \
        const uint32_t* p = c + RC_P; (void)p;                                    \
        body                                                                      \
    }

extern "C" int psim_prims_wv_usort(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    RC_CHECKS(if (p[0] > 1) PDOM("case %u: mode", i);)
    return run_waves(tk_wv_usort, cfg, in, ncases, 1, in_words, out, RC_OUT);
}
extern "C" int psim_prims_wv_uniform(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    RC_CHECKS(if (p[0] < 1 || p[0] > 64) PDOM("case %u: n %u outside [1, 64]", i, p[0]);)
    return run_waves(tk_wv_uniform, cfg, in, ncases, 1, in_words, out, RC_OUT);
}
extern "C" int psim_prims_wv_select(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    RC_CHECKS(if (p[0] > 64) PDOM("case %u: n %u > 64", i, p[0]);)
    return run_waves(tk_wv_select, cfg, in, ncases, 1, in_words, out, RC_OUT);
}
extern "C" int psim_prims_wv_sublist(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    RC_CHECKS(const uint32_t m = p[0] < p[1] ? p[0] : p[1];
              if (p[0] > 64) PDOM("case %u: n %u > 64", i, p[0]);
              if (p[2] + m > 64) PDOM("case %u: on %u + m %u past the 64 scratch words", i, p[2], m);)
    return run_waves(tk_wv_sublist, cfg, in, ncases, 1, in_words, out, RC_OUT);
}
// a merge's views and candidates: |Active| <= 8, |Passive| <= max_passive <= 30, ids < 2^27
static int merge_check(const PrimCfg* cfg, const uint32_t* c, uint32_t i, bool lite) {
    const uint32_t* p = c + RC_P;
    if (cfg->max_passive < 1 || cfg->max_passive > PSIM_PASSIVE_CAP - 2)
        return prims_edom("max_passive %u outside [1, 30]", cfg->max_passive);
    if (p[0] > PSIM_ACTIVE_CAP || p[1] > cfg->max_passive || p[2] > PSIM_EXCHANGE_CAP)
        return prims_edom("case %u: act_n %u pas_n %u nex %u", i, p[0], p[1], p[2]);
    for (uint32_t l = 0; l < p[0]; l++)
        if (!prims_id_ok(cfg, c[RC_R1 + l], true)) return prims_edom("case %u: active id", i);
    for (uint32_t l = 0; l < 64; l++) {
        // (the kernels hash the lanes past the count too: zeros)
        if (l >= p[1] && c[RC_R0 + l]) return prims_edom("case %u: passive lane %u past the count", i, l);
        if (!prims_id_ok(cfg, c[RC_R0 + l], true)) return prims_edom("case %u: passive id", i);
    }
    for (uint32_t l = 0; l < p[2]; l++) {
        if (!prims_id_ok(cfg, c[RC_R2 + l], true)) return prims_edom("case %u: exchange id", i);
        if (lite && p[3] && l && c[RC_R2 + l] <= c[RC_R2 + l - 1])
            return prims_edom("case %u: sorted exchange is not ascending", i);
    }
    return 0;
}
extern "C" int psim_prims_wv_merge(const PrimCfg* cfg, const uint32_t* in, uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    RC_CHECKS(if (int e = merge_check(cfg, c, i, false)) return e;)
    return run_waves(tk_wv_merge, cfg, in, ncases, 1, in_words, out, RC_OUT);
}

// width 32 or 16
#define BY_WIDTH(k32, k16, groups32) \
    (width == 32 ? run_waves(k32, cfg, in, ncases, groups32, in_words, out, RC_OUT) \
                 : run_waves(k16, cfg, in, ncases, 2 * groups32, in_words, out, RC_OUT))
#define WIDTH_OK() if (width != 32 && width != 16) PDOM("width %u", width)

extern "C" int psim_prims_lite_usort(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                     uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    RC_CHECKS(if (p[0] > 0xFF) PDOM("case %u: valid lanes past 7", i);
              for (uint32_t l = 0; l < 8; l++)
                  if (((p[0] >> l) & 1u) && c[RC_R0 + l] == PSIM_NONE) PDOM("case %u: PSIM_NONE is no value", i);)
    return BY_WIDTH(tk_lite_usort<32>, tk_lite_usort<16>, 2);
}
extern "C" int psim_prims_lite_uniform(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                       uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    RC_CHECKS(if (p[0] < 1 || p[0] > 31) PDOM("case %u: n %u outside [1, 31]", i, p[0]);)
    return BY_WIDTH(tk_lite_uniform<32>, tk_lite_uniform<16>, 2);
}
extern "C" int psim_prims_lite_select(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                      uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    RC_CHECKS(if (p[0] > (width == 32 ? 31u : 16u)) PDOM("case %u: n %u", i, p[0]);)
    return BY_WIDTH(tk_lite_select<32>, tk_lite_select<16>, 2);
}
// maxn 30 (width 32) or 8 (either width): the product's two instantiations
extern "C" int psim_prims_lite_sublist(const PrimCfg* cfg, uint32_t width, uint32_t maxn, const uint32_t* in,
                                       uint32_t ncases, uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    if (!(maxn == 8 || (maxn == 30 && width == 32))) PDOM("maxn %u at width %u", maxn, width);
    RC_CHECKS(if (p[0] > maxn) PDOM("case %u: n %u > %u", i, p[0], maxn);
              if (p[2] > 8) PDOM("case %u: on %u > 8", i, p[2]);)
    if (maxn == 30) return run_waves(tk_lite_sublist<30, 32>, cfg, in, ncases, 2, in_words, out, RC_OUT);
    return BY_WIDTH((tk_lite_sublist<8, 32>), (tk_lite_sublist<8, 16>), 2);
}
extern "C" int psim_prims_pas_sublist(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                      uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    RC_CHECKS(if (p[0] > 30) PDOM("case %u: n %u > 30", i, p[0]);
              if (p[2] > 8) PDOM("case %u: on %u > 8", i, p[2]);)
    return BY_WIDTH(tk_pas_sublist<32>, tk_pas_sublist<16>, 2);
}
extern "C" int psim_prims_lite_merge(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                     uint32_t* out) {
    LAUNCHER_HEAD(RC_IN);
    WIDTH_OK();
    RC_CHECKS(if (int e = merge_check(cfg, c, i, true)) return e;)
    return BY_WIDTH(tk_lite_merge<32>, tk_lite_merge<16>, 2);
}

// Pas<W>::step's domain: n <= 29 before a plain insert, 1 <= n <= 30 and
// k < n before an eviction, ids < 2^27; the launcher follows the view to know
// which steps are member no-ops
extern "C" int psim_prims_pas_step(const PrimCfg* cfg, uint32_t width, const uint32_t* in, uint32_t ncases,
                                   uint32_t nstep, uint32_t* out) {
    LAUNCHER_HEAD(PS_IN);
    WIDTH_OK();
    if (nstep > PS_NSTEP) PDOM("nstep %u", nstep);
    for (uint32_t i = 0; i < ncases; i++) {
        const uint32_t* c = in + (size_t)i * PS_IN;
        uint32_t n = c[0], v[32];
        if (n > 30) PDOM("case %u: n %u > 30", i, n);
        for (uint32_t l = 0; l < 32; l++) {
            v[l] = c[PS_ROW + l];
            if (!prims_id_ok(cfg, v[l], true)) PDOM("case %u: id %u", i, v[l]);
        }
        for (uint32_t s = 0; s < nstep; s++) {
            const uint32_t id = c[PS_STEPS + 2 * s], k = c[PS_STEPS + 2 * s + 1];
            if (!prims_id_ok(cfg, id, true)) PDOM("case %u step %u: id %u", i, s, id);
            bool mem = false;
            for (uint32_t l = 0; l < n; l++) mem |= v[l] == id;
            if (mem) continue;
            if (k != 0xFFFFFFFFu) {
                if (n < 1 || k >= n) PDOM("case %u step %u: eviction at %u of %u", i, s, k, n);
                for (uint32_t l = k; l + 1 < n; l++) v[l] = v[l + 1];
                n--;
            } else if (n > 29) {
                PDOM("case %u step %u: plain insert into %u entries", i, s, n);
            }
            uint32_t pos = 0;
            while (pos < n && prims_bucket(cfg, v[pos]) <= prims_bucket(cfg, id)) pos++;
            for (uint32_t l = n; l > pos; l--) v[l] = v[l - 1];
            v[pos] = id;
            n++;
        }
    }
    const uint32_t groups = 64 / width;
    if (ncases % groups) PDOM("ncases %u is no multiple of the wave's %u groups", ncases, groups);
    return prims_run(cfg, in, ncases * in_words * 4, out, (size_t)ncases * PS_OUT * 4,
                     [&](const RoundArgs& a, const uint32_t* di, uint32_t* dout) {
                         if (width == 32) tk_pas_step<32><<<dim3(ncases / 2), dim3(64)>>>(a, di, dout, nstep);
                         else tk_pas_step<16><<<dim3(ncases / 4), dim3(64)>>>(a, di, dout, nstep);
                     });
}
