// grad_wave_inst.hpp -- instantiation list of seq_grad_wave_kernel for one lattice mode (included by grad_wave_inst_*.hip)
#pragma once
#include "launchers.hpp"
#include "grad_plan.hpp"
#include "grad_wave_kernel.hpp"

namespace gpsig {

template <int G, int C, int DP, int LQ, int MODE>
hipError_t wave_launch(const WaveGradArgs& a, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL((seq_grad_wave_kernel<G, C, DP, LQ, MODE>), dim3(nblocks), dim3(64), 0, s, a);
    return hipGetLastError();
}

// The shapes (G, C, DP) are GPSIG_WAVE_SHAPES of grad_plan.hpp, which the planners read too.
// Level variants of the scratch-free kernels (grad_w2_variant there): num_levels 4 and 5 at compile time (LQ = 3, 4), otherwise LQ = 4 or 7 at run time.
#define GPSIG_W2_PICK(LAUNCH, G_, C_, D_)                                           \
    if (G == G_ && C == C_ && DP == D_) {                                           \
        const GradLevelVariant v = grad_w2_variant(LQ);                             \
        return v == GRAD_LV_CT3 ? LAUNCH<G_, C_, D_, 3, MODE, true>                 \
                                : (v == GRAD_LV_CT4 ? LAUNCH<G_, C_, D_, 4, MODE, true> : (v == GRAD_LV_RT4 ? LAUNCH<G_, C_, D_, 4, MODE, false> : LAUNCH<G_, C_, D_, 7, MODE, false>)); \
    }

#ifdef GPSIG_INST_WAVE2
template <int G, int C, int DP, int LQ, int MODE, bool MX>
hipError_t wave2_launch(const Wave2Args& a, int nblocks, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((seq_grad_wave2_kernel<G, C, DP, LQ, MODE, MX>), dim3(nblocks), dim3(64), lds, s, a);
    return hipGetLastError();
}
template <int MODE>
Wave2LaunchFn wave2_lookup_mode(int G, int C, int DP, int LQ) {
#define X_W2(G_, C_, D_) GPSIG_W2_PICK(wave2_launch, G_, C_, D_)
    GPSIG_WAVE_SHAPES(X_W2)
#undef X_W2
    return nullptr;
}
#endif

#ifdef GPSIG_INST_LAM
// KIND is part of every name here: the translation units of the two kernel families instantiate different functions
template <int KIND>
struct LamUndoInst {
    template <int G, int C, int DP, int LQ, int MODE, bool MX>
    static hipError_t launch(const Wave2Args& a, int nblocks, size_t lds, hipStream_t s) {
        hipLaunchKernelGGL((seq_lam_undo_kernel<G, C, DP, LQ, MODE, MX, KIND>), dim3(nblocks), dim3(64), lds, s, a);
        return hipGetLastError();
    }
    template <int MODE>
    static Wave2LaunchFn lookup(int G, int C, int DP, int LQ) {
#define X_LU(G_, C_, D_) GPSIG_W2_PICK(launch, G_, C_, D_)
        GPSIG_WAVE_SHAPES(X_LU)
#undef X_LU
        return nullptr;
    }
};
#endif

template <int MODE>
WaveLaunchFn wave_lookup_mode(int G, int C, int DP, int LQ) {
#define X_W(G_, C_, D_)                                                              \
    if (G == G_ && C == C_ && DP == D_) return grad_wave_variant(LQ) == GRAD_LV_RT4 ? wave_launch<G_, C_, D_, 4, MODE> : wave_launch<G_, C_, D_, 7, MODE>;
    GPSIG_WAVE_SHAPES(X_W)
#undef X_W
    return nullptr;
}
}  // namespace gpsig
