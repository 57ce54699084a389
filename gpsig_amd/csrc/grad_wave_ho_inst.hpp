// instances of the higher-order reverse sweeps (grad_wave_ho_kernel.hpp): lanes per pair x columns per lane x order (2, 3, 4); the scratch-free
// kernel with num_levels 2-5 at compile time, the slot kernel (prefixes through HBM) with num_levels <= 5 at run time
#include "launchers.hpp"
#include "grad_wave_ho_kernel.hpp"

namespace gpsig {

#ifndef GPSIG_HO_UNDO_ONLY
template <int G, int C, int O>
static hipError_t wave_ho_launch(const WaveHoArgs& a, int nblocks, size_t, hipStream_t s) {
    hipLaunchKernelGGL((seq_grad_wave_ho_kernel<G, C, 4, O>), dim3(nblocks), dim3(64), 0, s, a);
    return hipGetLastError();
}
template <int G, int C>
static WaveHoLaunchFn pick(int order) {
#define X_HO(O_) if (order == O_) return &wave_ho_launch<G, C, O_>;
    GPSIG_HO_SLOT_ORDERS(X_HO)
#undef X_HO
    return nullptr;
}
// order: min(order, num_levels) >= 2.  Forms and orders: GPSIG_HO_SLOT_FORMS / GPSIG_HO_SLOT_ORDERS of grad_plan.hpp
WaveHoLaunchFn wave_ho_lookup(int G, int C, int order, int M) {
    if (M < HO_SLOT_MIN_LEVELS || M > HO_SLOT_MAX_LEVELS) return nullptr;
#define X_HO(G_, C_) if (G == G_ && C == C_) return pick<G_, C_>(order);
    GPSIG_HO_SLOT_FORMS(X_HO)
#undef X_HO
    return nullptr;
}
#endif

#ifndef GPSIG_HO_UNDO_ONLY
// first order from a dM lattice (seq_grad_wave_o1_kernel): 16 lanes per lattice, 2 / 4 columns per lane (lattices of at most 64 columns), 3 or 7 levels kept
template <int G, int C, int LQ>
static hipError_t wave_o1_launch(const WaveHoArgs& a, int nblocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((seq_grad_wave_o1_kernel<G, C, LQ>), dim3(nblocks), dim3(64), lds, s, a);
    return hipGetLastError();
}
WaveHoLaunchFn wave_o1_lookup(int G, int C, int M) {
    if (M < 1 || M > 8 || G != 16) return nullptr;
    if (C == 2) return M <= 4 ? &wave_o1_launch<16, 2, 3> : &wave_o1_launch<16, 2, 7>;
    if (C == 4) return M <= 4 ? &wave_o1_launch<16, 4, 3> : &wave_o1_launch<16, 4, 7>;
    return nullptr;
}
#endif

#ifdef GPSIG_HO_UNDO_G
template <int G, int C, int MM, int O>
static hipError_t wave_ho_undo_launch(const WaveHoArgs& a, int nblocks, size_t lds, hipStream_t s) {
    auto kern = seq_grad_wave_ho_undo_kernel<G, C, MM, O>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), lds, s, a);
    return hipGetLastError();
}
// (num_levels, order): GPSIG_HO_UNDO_LEVELS of grad_plan.hpp
template <int G, int C>
static WaveHoLaunchFn pick_undo(int order, int M) {
#define X_HO(M_, O_) if (M == M_ && order == O_) return &wave_ho_undo_launch<G, C, M_, O_>;
    GPSIG_HO_UNDO_LEVELS(X_HO)
#undef X_HO
    return nullptr;
}
template <int G, int C, int MM, int O>
static hipError_t wave_ho_levels_launch(const WaveHoArgs& a, int nblocks, size_t, hipStream_t s) {
    hipLaunchKernelGGL((seq_levels_wave_ho_kernel<G, C, MM, O>), dim3(nblocks), dim3(64), 0, s, a);
    return hipGetLastError();
}
template <int G, int C>
static WaveHoLaunchFn pick_levels(int order, int M) {
#define X_HO(M_, O_) if (M == M_ && order == O_) return &wave_ho_levels_launch<G, C, M_, O_>;
    GPSIG_HO_UNDO_LEVELS(X_HO)
#undef X_HO
    return nullptr;
}
// this unit's share (lanes per pair GG) of GPSIG_HO_UNDO_FORMS: the other forms are discarded statements, not instantiated
template <int GG>
static WaveHoLaunchFn undo_lookup_of(int C, int order, int M) {
#define X_HO(G_, C_) if constexpr (GG == G_) { if (C == C_) return pick_undo<G_, C_>(order, M); }
    GPSIG_HO_UNDO_FORMS(X_HO)
#undef X_HO
    return nullptr;
}
template <int GG>
static WaveHoLaunchFn levels_lookup_of(int C, int order, int M) {
#define X_HO(G_, C_) if constexpr (GG == G_) { if (C == C_) return pick_levels<G_, C_>(order, M); }
    GPSIG_HO_UNDO_FORMS(X_HO)
#undef X_HO
    return nullptr;
}
#define HO_CAT2(a, b) a##b
#define HO_CAT(a, b) HO_CAT2(a, b)
WaveHoLaunchFn HO_CAT(wave_ho_undo_lookup_g, GPSIG_HO_UNDO_G)(int C, int order, int M) { return undo_lookup_of<GPSIG_HO_UNDO_G>(C, order, M); }
WaveHoLaunchFn HO_CAT(wave_ho_levels_lookup_g, GPSIG_HO_UNDO_G)(int C, int order, int M) { return levels_lookup_of<GPSIG_HO_UNDO_G>(C, order, M); }
#endif
}  // namespace gpsig
