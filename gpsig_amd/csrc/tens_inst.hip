// Dispatch over the tens_vs_seq_kernel translation units (tens_inst_{f64,f32}_{lo,m6,m7,m8}.hip; the tensor-lane variant: tens_inst_lanet.hip).
#include "launchers.hpp"
#include "aux_kernels.hpp"

namespace gpsig {
TvsLaunchFn tvs_lookup(int M, int TT, bool incr, bool f32) {
    if (M <= 5) return f32 ? tvs_lookup_f32_lo(M, TT, incr) : tvs_lookup_f64_lo(M, TT, incr);
    if (M == 6) return f32 ? tvs_lookup_f32_m6(M, TT, incr) : tvs_lookup_f64_m6(M, TT, incr);
    if (M == 7) return f32 ? tvs_lookup_f32_m7(M, TT, incr) : tvs_lookup_f64_m7(M, TT, incr);
    return f32 ? tvs_lookup_f32_m8(M, TT, incr) : tvs_lookup_f64_m8(M, TT, incr);
}
}  // namespace gpsig
