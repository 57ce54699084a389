// seq_inst_ho_exact.hpp -- exact higher-order seq-gram instances for one Matern family (round 6, as seq_inst_ho_ptdrbf_exact.hip for the RBF kernel):
// points with differences, num_levels AND order at compile time, prescaled records + table exp + v_rsq_f64 (seq_core.hpp: seq_step_matern_prescaled_ho);
// 16 lanes per pair, 4 columns per lane, 8 / 4 feature columns, order 2, num_levels 3 / 4 / 5.  signature_algs.py:37-74.
// Each seq_inst_ho_ptdm*_exact.hip defines GPSIG_INST_NAME and GPSIG_INST_KIND (its family) and includes this file; the lookup is null for any other kind.
#include "launchers.hpp"
#include "seq_configs.hpp"
#include "seq_gram_kernel.hpp"

namespace gpsig {
SeqLaunchFn GPSIG_INST_NAME(int kind, int G, int C, int D, int M, int order) {
#define GPSIG_HO_EXACT_M(D_, M_, O_)                                                                  \
    if (kind == GPSIG_INST_KIND && G == 16 && C == 4 && D == D_ && M == M_ && order == O_)            \
        return &seq_gram_launch<double, 16, 4, D_, M_, MODE_PT_DIFF, true, O_, GPSIG_INST_KIND>;
    GPSIG_HO_EXACT_M(8, 4, 2) GPSIG_HO_EXACT_M(8, 5, 2) GPSIG_HO_EXACT_M(4, 4, 2) GPSIG_HO_EXACT_M(4, 5, 2) GPSIG_HO_EXACT_M(8, 3, 2) GPSIG_HO_EXACT_M(4, 3, 2)
#undef GPSIG_HO_EXACT_M
    return nullptr;
}
}  // namespace gpsig
