// seq_inst_ho.hpp -- explicit instantiation helper for the higher-order kernels (see seq_inst.hpp).
#include "launchers.hpp"
#include "seq_configs.hpp"
#include "seq_gram_kernel.hpp"

#ifndef GPSIG_INST_T
#define GPSIG_INST_T double
#endif

namespace gpsig {
#define GPSIG_INST_HO_CASE(G_, C_, D_, MM_, OM_) \
    if (G == G_ && C == C_ && D == D_ && MMAX == MM_ && OMAX == OM_) \
        return &seq_gram_launch<GPSIG_INST_T, G_, C_, D_, MM_, GPSIG_INST_MODE, false, OM_>;

SeqLaunchFn GPSIG_INST_NAME(int G, int C, int D, int MMAX, int OMAX) {
    GPSIG_INST_LIST(GPSIG_INST_HO_CASE)
    return nullptr;
}

// the unit's descriptor (launchers.hpp: SeqHoUnit); a unit serves the one padded width of its list
#ifndef __HIP_DEVICE_COMPILE__          // host data: the device pass would emit a copy that points at a host function
#define GPSIG_INST_HO_D(G_, C_, D_, MM_, OM_) D_,
constexpr int GPSIG_INST_HO_DS[] = {GPSIG_INST_LIST(GPSIG_INST_HO_D)};
#define GPSIG_INST_HO_SAME(G_, C_, D_, MM_, OM_) static_assert(D_ == GPSIG_INST_HO_DS[0], "one padded width per higher-order unit");
GPSIG_INST_LIST(GPSIG_INST_HO_SAME)
#define GPSIG_INST_CAT2(a, b) a##b
#define GPSIG_INST_CAT(a, b) GPSIG_INST_CAT2(a, b)
const SeqHoUnit GPSIG_INST_CAT(GPSIG_INST_NAME, _unit) = {sizeof(GPSIG_INST_T) == 4, GPSIG_INST_MODE, GPSIG_INST_HO_DS[0], &GPSIG_INST_NAME};
#endif
}  // namespace gpsig
