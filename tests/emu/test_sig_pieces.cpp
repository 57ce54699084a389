// Host check of gpsig_amd/csrc/sig_pieces.hpp: the depth pieces of the feature contraction cover the slabs exactly once, in order, the
// equal ones follow the round-3 formula, the graded tail halves.  Prints the number of violations.
//
// And of sig_piece_counts, the model that chooses the two counts (sig_feat_api.hip: sig_features_K): its bounds over a grid of problem sizes,
// and pinned values.  argv[1]: SG_MAX_PIECES of sig_feat_kernel.hpp (the caller reads it there: that header needs HIP).  argv[2] = "plans":
// prints "N d M nslab nsplit graded" of symmetric Grams instead, for the caller to hold against the Python restatements of the model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sig_pieces.hpp"

static const long long SIZES[] = {1, 2, 64, 127, 128, 129, 257, 512, 1000, 2048, 4096, 5000, 8192, 20000, 65536, 100000};

static int slabs_of(int d, int M) {              // the depth of the whole feature width: ld = F + 1 rounded up to 16, in slabs of SG_BK = 16
    long long F = 0, w = 1;
    for (int m = 1; m <= M; ++m) { w *= d; F += w; }
    return int(((F + 1 + 15) / 16 * 16 + 15) / 16);
}

static int check_counts(int max_pieces) {
    int bad = 0;
    std::vector<int> b(max_pieces + 1);          // SigGramArgs::bound: exactly as long (the address sanitizer sees a piece too many)
    for (long long N1 : SIZES)
        for (long long N2 : SIZES)
            for (int sym = 0; sym < 2; ++sym)
                for (int nslab : {1, 2, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 100, 274, 1000, 2341, 20000})
                    for (int on = 0; on < 2; ++on) {
                        int nsplit = -1, graded = -1;
                        gpsig::sig_piece_counts(N1, N2, sym != 0, nslab, on != 0, &nsplit, &graded);
                        const long long nt = (N1 + 127) / 128, tiles = sym ? nt * (nt + 1) / 2 : nt * ((N2 + 127) / 128);
                        if (nsplit < 1 || nsplit > 128) ++bad;
                        // pieces of at least 8 slabs, unless "large Grams keep at least 4" raised the count
                        if (nsplit * 8 > nslab + 7 && !(tiles > 1024 && nsplit == 4 && nslab >= 32)) ++bad;
                        if (graded < 1 || graded > 5) ++bad;
                        if ((!on || tiles * nsplit <= 512) && graded != 1) ++bad;
                        if (nsplit - 1 + graded > max_pieces) { ++bad; continue; }
                        if (gpsig::sig_piece_bounds(nslab, nsplit, graded, b.data()) > max_pieces) ++bad;
                    }
    // pinned: {N1, N2, sym, nslab_all, sig_graded} -> {nsplit, graded}, from the model as it stood inside sig_features_K before it moved here.
    // BASELINE configs[1] first (11 equal pieces, a graded tail of 4); d = 16, M = 3 at N = 4,096 (274 slabs) is the small shape with a graded tail
    const long long pins[][7] = {
        {4096, 4096, 1, 2341, 1, 11, 4}, {4096, 4096, 1, 2341, 0, 11, 1}, {4096, 4096, 1, 274, 1, 4, 3}, {4096, 4096, 1, 274, 0, 4, 1},
        {1, 1, 1, 1, 1, 1, 1}, {129, 129, 1, 6, 1, 1, 1}, {257, 257, 1, 22, 1, 3, 1}, {1000, 3000, 0, 274, 1, 5, 1}, {300, 5000, 0, 100, 1, 2, 1},
        {65536, 65536, 1, 2341, 1, 4, 1}, {65536, 65536, 1, 40, 1, 4, 1}, {20000, 20000, 1, 32, 1, 4, 1}, {512, 16384, 0, 98, 1, 1, 1},
        {8192, 8192, 1, 2341, 1, 6, 3}, {2048, 2048, 1, 2341, 1, 11, 1}};
    for (const auto& q : pins) {
        int nsplit = -1, graded = -1;
        gpsig::sig_piece_counts(q[0], q[1], q[2] != 0, int(q[3]), q[4] != 0, &nsplit, &graded);
        if (nsplit != q[5] || graded != q[6]) ++bad;
    }
    return bad;
}

int main(int argc, char** argv) {
    const int max_pieces = argc > 1 ? atoi(argv[1]) : 144;
    if (argc > 2 && !strcmp(argv[2], "plans")) {
        const int shapes[][2] = {{1, 2}, {3, 2}, {3, 4}, {2, 8}, {8, 3}, {6, 4}, {16, 3}, {8, 5}, {32, 3}};
        for (long long N : SIZES)
            for (const auto& s : shapes) {
                int nsplit = -1, graded = -1;
                gpsig::sig_piece_counts(N, N, true, slabs_of(s[0], s[1]), true, &nsplit, &graded);
                printf("%lld %d %d %d %d %d\n", N, s[0], s[1], slabs_of(s[0], s[1]), nsplit, graded);
            }
        return 0;
    }
    int bad = 0;
    std::vector<int> b(300);
    for (int nslab : {1, 2, 7, 8, 16, 31, 64, 100, 213, 1000, 2341, 20000})
        for (int equal : {1, 2, 3, 4, 11, 16, 31, 128})
            for (int graded : {1, 2, 3, 4, 5}) {
                const int n = gpsig::sig_piece_bounds(nslab, equal, graded, b.data());
                const int eq = equal > nslab ? nslab : equal;
                if (b[0] != 0 || b[n] != nslab) ++bad;
                for (int s = 0; s < n; ++s)
                    if (b[s + 1] < b[s] || (nslab >= eq && b[s + 1] == b[s] && graded == 1)) ++bad;
                for (int s = 0; s < eq; ++s)
                    if (b[s] != int((long long)nslab * s / eq)) ++bad;                       // the equal pieces: round 3's boundaries
                const int len = nslab - b[eq - 1];
                const bool cut = graded > 1 && len >= 2 * graded;
                if (n != eq - 1 + (cut ? graded : 1)) ++bad;
                if (cut) {
                    for (int s = eq - 1; s + 2 < n; ++s) {                                   // each graded piece: half of what was left
                        const int a = b[s + 1] - b[s], rest = nslab - b[s];
                        if (a != rest / 2) ++bad;
                    }
                    if (b[n] - b[n - 1] < 1) ++bad;
                }
            }
    // BASELINE configs[1]: 2341 slabs, 11 equal pieces, the last one as 1/2, 1/4, 1/8, 1/8
    const int n = gpsig::sig_piece_bounds(2341, 11, 4, b.data());
    if (n != 14 || b[10] != 2128 || b[11] != 2128 + 106 || b[12] != 2128 + 106 + 53 || b[13] != 2128 + 106 + 53 + 27 || b[14] != 2341) ++bad;
    bad += check_counts(max_pieces);
    printf("%d\n", bad);
    return 0;
}
