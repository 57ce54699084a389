// api_common.hpp -- what the evaluation entry points of api.hip (the exact kernels) and of lr_api.hip (low-rank mode) both open with: the
// parameter check and the device copies of what a gpsig_params carries; and the timed-launch helper of every host unit that times.
// Defined in api.hip; host code only.
#pragma once
#include "ctx.hpp"

namespace gpsig {
struct ScaleParams;

// low_rank: the low-rank entry points, whose float32 forms carry the spectral base kernel too.  lr_wide: the entry points of low-rank mode that
// serve SignatureSpectral beyond the SPECTRAL_STRIDE columns of its packed table for a kernel object that opts in (base_params[2] != 0)
int check_params(gpsig_ctx* c, const gpsig_params* p, bool low_rank = false, bool lr_wide = false);
// lengthscales, lags and gamma for a launch: state spaces wider than MAX_FEATURES read their lengthscales from a device copy (cached by content)
int scale_params(gpsig_ctx* c, const gpsig_params* p, bool apply_scaling, ScaleParams* out);
// BASE_SPECTRAL: alpha[Q], omega[Q][SPECTRAL_STRIDE], gamma[Q][SPECTRAL_STRIDE] on the device (zero padded); NULL otherwise
int spectral_table(gpsig_ctx* c, const gpsig_params* p, const double** dev);
// ... beyond SPECTRAL_STRIDE columns (low-rank evaluation with lr_spectral_wide, exact evaluation with spectral_wide): alpha[Q], omega[Q][d], gamma[Q][d]
// as the caller holds them, on the device in B_SPECW (lr_api.hip)
int spectral_table_wide(gpsig_ctx* c, const gpsig_params* p, const double** dev);
void base_p(const gpsig_params* p, double* p0, double* p1);
// weights sigma * variances[m] on the device
int upload_weights(gpsig_ctx* c, const gpsig_params* p, const double** w);
// A pair of events from the context's pool around the launches a call times (gpsig_timing_*); *e0 is recorded here, *e1 by the caller.  Timing covers
// the launches since gpsig_timing_reset, up to TIMING_MAX_EVENTS events (a long-running caller that never reads the timing must not accumulate
// them); *on says whether this launch is timed.  Never inside a graph capture.  Used by api.hip, sig_feat_api.hip and wide_api.hip.
constexpr size_t TIMING_MAX_EVENTS = 8192;
int timing_begin(gpsig_ctx* c, hipEvent_t* e0, hipEvent_t* e1, bool* on);
// lr_api.hip: the context is going away -- its low-rank states outlive it as plain memory blocks (gpsig_ctx_destroy)
void lr_detach_states(gpsig_ctx* c);

}  // namespace gpsig

#define ENTER(c, p)                         \
    CHK(check_params((c), (p)));            \
    HIPCHK((c), hipSetDevice((c)->device));
#define ENTER_LR(c, p)                       \
    CHK(check_params((c), (p), true, true)); \
    HIPCHK((c), hipSetDevice((c)->device));
#define ENTER_GRAM(c, p)                      \
    CHK(check_params((c), (p), false, true)); \
    HIPCHK((c), hipSetDevice((c)->device));
