// test_grad_plan.cpp -- the plan of the sequence-gradient sweeps (gpsig_amd/csrc/grad_plan.hpp) on the host, driven by tests/test_grad_plan_host.py.
//   test_grad_plan list     the compiled instances, one per line
//   test_grad_plan sweep    every plan over R <= 520, DP in {4, 8, 16}, num_levels <= 8, orders <= 4 (and a few long row sides): prints
//                           "<plans outside the compiled list> <plans made>"
//   test_grad_plan plan     cases on stdin, one per line, the planned instance(s) of each on stdout:
//                             wave  <mode> <R2> <DP> <num_levels>
//                             wave2 <mode> <R1> <R2> <DP> <num_levels> <one_side>          (both launches, "x | y")
//                             lam   <mode> <rbf> <R1> <R2> <DP> <num_levels>
//                             ho    <grad_impl> <ho_g32> <num_levels> <order> <R1> <R2>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "grad_plan.hpp"

using namespace gpsig;

static const char* variant_name(int v) {
    static const char* names[4] = {"3c", "4c", "4r", "7r"};           // levels kept, at compile / run time
    return names[v];
}

static std::string name_of(const GradInstance& g) {
    char b[96];
    switch (g.family) {
    case GRAD_WAVE: snprintf(b, sizeof b, "wave %d %d %d %d %s", g.mode, g.G, g.C, g.DP, variant_name(g.variant)); break;
    case GRAD_WAVE2: snprintf(b, sizeof b, "wave2 %d %d %d %s", g.G, g.C, g.DP, variant_name(g.variant)); break;
    case GRAD_LAM_UNDO: snprintf(b, sizeof b, "lam %d %s %d %d %d %s", g.mode, g.rbf ? "rbf" : "gen", g.G, g.C, g.DP, variant_name(g.variant)); break;
    case GRAD_HO_UNDO: snprintf(b, sizeof b, "ho_undo %d %d %d %d", g.G, g.C, g.num_levels, g.order); break;
    case GRAD_HO_SLOT: snprintf(b, sizeof b, "ho_slot %d %d %d", g.G, g.C, g.order); break;
    default: snprintf(b, sizeof b, "none");
    }
    return b;
}

static long key_of(const GradInstance& g) {
    return ((((((((long(g.family) * 4 + g.mode) * 128 + g.G) * 16 + g.C) * 32 + g.DP) * 8 + g.variant) * 2 + g.rbf) * 8 + g.num_levels) * 8 + g.order);
}

static std::vector<GradInstance> compiled() {
    std::vector<GradInstance> out;
    GradInstance g;
    const int variants[4] = {GRAD_LV_CT3, GRAD_LV_CT4, GRAD_LV_RT4, GRAD_LV_RT7};
#define X_T(G_, C_, D_)                                                                                                         \
    g = GradInstance(); g.G = G_; g.C = C_; g.DP = D_;                                                                          \
    for (int mode : {GRAD_MODE_INC, GRAD_MODE_PT_DIFF, GRAD_MODE_PT_NODIFF})                                                     \
        for (int v : {GRAD_LV_RT4, GRAD_LV_RT7}) { g.family = GRAD_WAVE; g.mode = mode; g.variant = v; out.push_back(g); } \
    for (int v : variants) { g.family = GRAD_WAVE2; g.mode = GRAD_MODE_INC; g.variant = v; out.push_back(g); }          \
    for (int mode : {GRAD_MODE_PT_DIFF, GRAD_MODE_PT_NODIFF})                                                                    \
        for (int rbf : {0, 1})                                                                                                   \
            for (int v : variants) { g.family = GRAD_LAM_UNDO; g.mode = mode; g.rbf = rbf; g.variant = v; out.push_back(g); }
    GPSIG_WAVE_SHAPES(X_T)
#undef X_T
#define X_L(M_, O_) g.num_levels = M_; g.order = O_; out.push_back(g);
#define X_T(G_, C_) g = GradInstance(); g.family = GRAD_HO_UNDO; g.G = G_; g.C = C_; GPSIG_HO_UNDO_LEVELS(X_L)
    GPSIG_HO_UNDO_FORMS(X_T)
#undef X_T
#undef X_L
#define X_L(O_) g.order = O_; out.push_back(g);
#define X_T(G_, C_) g = GradInstance(); g.family = GRAD_HO_SLOT; g.G = G_; g.C = C_; GPSIG_HO_SLOT_ORDERS(X_L)
    GPSIG_HO_SLOT_FORMS(X_T)
#undef X_T
#undef X_L
    return out;
}

static int sweep() {
    std::set<long> have;
    for (const GradInstance& g : compiled()) have.insert(key_of(g));
    long bad = 0, plans = 0;
    auto check = [&](const GradInstance& g) {
        if (g.family == GRAD_NONE) return;
        ++plans;
        if (!have.count(key_of(g))) { if (++bad < 20) fprintf(stderr, "not compiled: %s\n", name_of(g).c_str()); }
    };
    std::vector<int> rows;                                             // the row side enters through the LDS bounds only
    for (int r = 1; r <= 520; r += 7) rows.push_back(r);
    for (int r : {520, 1170, 1171, 2048, 2340, 2341, 2730, 2731, 4096, 8192, 8193, 20000}) rows.push_back(r);
    for (int DP : {4, 8, 16})
        for (int M = 1; M <= 8; ++M)
            for (int R2 = 1; R2 <= 520; ++R2) {
                for (int mode = 0; mode < 3; ++mode) {
                    check(wave_plan_shape(mode, R2, DP, M));
                    check(wave2_plan_shape(mode, R2, DP, M));
                }
                for (int R1 : rows) {
                    GradInstance gx, gy;
                    for (int one = 0; one < 2; ++one)
                        if (wave2_plan_call(GRAD_MODE_INC, R1, R2, DP, M, one != 0, &gx, &gy)) { check(gx); check(gy); }
                    for (int mode = 1; mode < 3; ++mode)
                        for (int rbf = 0; rbf < 2; ++rbf) check(lam_undo_plan_shape(mode, rbf != 0, R1, R2, DP, M));
                }
            }
    for (int impl = 0; impl <= 4; ++impl)
        for (int g32 = -1; g32 <= 1; ++g32)
            for (int M = 1; M <= 8; ++M)
                for (int order = 1; order <= 4; ++order)
                    for (int R2 = 1; R2 <= 520; ++R2)
                        for (int R1 : rows) {
                            size_t lds = 0;
                            const GradInstance g = ho_sweeps_plan_shape(impl, g32, M, order, R1, R2, &lds);
                            check(g);
                            if ((g.family == GRAD_HO_UNDO) != (lds > 0) || lds > WAVE_HO_UNDO_LDS_MAX) ++bad;
                        }
    printf("%ld %ld\n", bad, plans);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "list")) {
        for (const GradInstance& g : compiled()) puts(name_of(g).c_str());
        return 0;
    }
    if (!strcmp(argv[1], "sweep")) return sweep();
    if (strcmp(argv[1], "plan")) return 2;
    char line[256], fam[16];
    while (fgets(line, sizeof line, stdin)) {
        int a[6] = {0, 0, 0, 0, 0, 0};
        const int n = sscanf(line, "%15s %d %d %d %d %d %d", fam, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
        if (n < 1) continue;
        if (!strcmp(fam, "wave") && n == 5) {
            puts(name_of(wave_plan_shape(a[0], a[1], a[2], a[3])).c_str());
        } else if (!strcmp(fam, "wave2") && n == 7) {
            GradInstance gx, gy;
            wave2_plan_call(a[0], a[1], a[2], a[3], a[4], a[5] != 0, &gx, &gy);
            printf("%s | %s\n", name_of(gx).c_str(), name_of(gy).c_str());
        } else if (!strcmp(fam, "lam") && n == 7) {
            puts(name_of(lam_undo_plan_shape(a[0], a[1] != 0, a[2], a[3], a[4], a[5])).c_str());
        } else if (!strcmp(fam, "ho") && n == 7) {
            size_t lds = 0;
            puts(name_of(ho_sweeps_plan_shape(a[0], a[1], a[2], a[3], a[4], a[5], &lds)).c_str());
        } else {
            fprintf(stderr, "bad case: %s", line);
            return 2;
        }
    }
    return 0;
}
