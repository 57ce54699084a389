// exact higher-order seq-gram instances (num_levels and order at compile time): MODE_PT_DIFF, BASE_MATERN12
#define GPSIG_INST_NAME seq_lookup_ho_ptdm12_exact
#define GPSIG_INST_KIND BASE_MATERN12
#include "seq_inst_ho_exact.hpp"
