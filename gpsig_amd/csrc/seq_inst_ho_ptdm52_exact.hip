// exact higher-order seq-gram instances (num_levels and order at compile time): MODE_PT_DIFF, BASE_MATERN52
#define GPSIG_INST_NAME seq_lookup_ho_ptdm52_exact
#define GPSIG_INST_KIND BASE_MATERN52
#include "seq_inst_ho_exact.hpp"
