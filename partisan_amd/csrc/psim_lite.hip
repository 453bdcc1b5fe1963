// psim_lite.hip -- k_lite_quarter / k_lite_half, the lite list's kernels: the
// entry points, their launch descriptors and this TU's diagnostics.  The
// kernels' text is psim_lite.h (shared with k_hv_phase, psim_consume.hip).
#include "psim_lite.h"

namespace psim {

using namespace lite;

// (two entry points: the launch bounds differ, and profilers and
// psim_kernel_times name them)
__global__ void __launch_bounds__(64 * PSIM_HALF_WPB, PSIM_HALF_WAVES) k_lite_half(RoundArgs args) {
    __shared__ __attribute__((aligned(16))) uint32_t pool[Carve<32>::WORDS];
    lite_kernel<32>(blockIdx.x, gridDim.x, pool);
}
__global__ void __launch_bounds__(64 * PSIM_QUARTER_WPB, PSIM_QUARTER_WAVES) k_lite_quarter(RoundArgs args) {
    __shared__ __attribute__((aligned(16))) uint32_t pool[Carve<16>::WORDS];
    lite_kernel<16>(blockIdx.x, gridDim.x, pool);
}

// k_lite_quarter's grid is a row per local node, capped (psim_create); the
// half's is a block per 2 x block local nodes, the 2048 blocks at 2^20 nodes
// it was tuned with in round 4
LiteKernel lite_kernel_groups(bool half) {
    constexpr uint32_t hb = 64 * Grp<32>::WPB, qb = 64 * Grp<16>::WPB;
    if (half) return {k_lite_half, hb, 2 * hb, resident_grid((const void*)k_lite_half, hb), false};
    return {k_lite_quarter, qb, qb / 16, resident_grid((const void*)k_lite_quarter, qb), false};
}

#ifdef PSIM_STAMPS
int debug_stamps_half(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_half), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_half), z, sizeof z) != hipSuccess) return -1;
    return 32;
}
#else
int debug_stamps_half(unsigned long long*) { return 0; }
#endif
// this TU's layout (psim_kernels.h layout_sig, checked by psim_create)
uint32_t layout_sig_lite() { return layout_sig(); }

}  // namespace psim
