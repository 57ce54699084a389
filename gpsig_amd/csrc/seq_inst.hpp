// seq_inst.hpp -- explicit instantiation helper: each seq_inst_*.hip defines GPSIG_INST_NAME, GPSIG_INST_MODE and
// GPSIG_INST_LIST and includes this file, which emits the kernels of that list, a lookup function and the unit's descriptor
// (launchers.hpp: SeqUnit), which is how api.hip finds the unit.
#include "launchers.hpp"
#include "seq_configs.hpp"
#include "seq_gram_kernel.hpp"

#ifndef GPSIG_INST_T
#define GPSIG_INST_T double
#endif
#ifndef GPSIG_INST_KIND
#define GPSIG_INST_KIND -1
#endif

namespace gpsig {
#define GPSIG_INST_CASE(G_, C_, D_, MM_, EX_) \
    if (G == G_ && C == C_ && D == D_ && MMAX == MM_ && exact == EX_) \
        return &seq_gram_launch<GPSIG_INST_T, G_, C_, D_, MM_, GPSIG_INST_MODE, EX_, 0, GPSIG_INST_KIND>;

SeqLaunchFn GPSIG_INST_NAME(int G, int C, int D, int MMAX, bool exact) {
    GPSIG_INST_LIST(GPSIG_INST_CASE)
    return nullptr;
}

#ifndef __HIP_DEVICE_COMPILE__          // host data: the device pass would emit a copy that points at a host function
#define GPSIG_INST_CAT2(a, b) a##b
#define GPSIG_INST_CAT(a, b) GPSIG_INST_CAT2(a, b)
const SeqUnit GPSIG_INST_CAT(GPSIG_INST_NAME, _unit) = {sizeof(GPSIG_INST_T) == 4, GPSIG_INST_MODE, GPSIG_INST_KIND, &GPSIG_INST_NAME};
#endif
}  // namespace gpsig
