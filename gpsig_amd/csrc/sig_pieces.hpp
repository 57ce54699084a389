// sig_pieces.hpp -- how the feature contraction (sig_feat_kernel.hpp) cuts its depth into pieces.  Plain C++ (no HIP): compiled on the
// host by tests/test_device_headers.py as well.
#pragma once

#include <math.h>
#include <stdint.h>

namespace gpsig {

// Slab ranges of the depth pieces.  `equal` pieces of the same size, the last of which is cut into `graded` finer ones of halving size
// (1/2, 1/4, .., the last two alike) when graded > 1: workgroups are handed out piece after piece, so equal pieces end in a last round
// that is as long as the others but only partly full (configs[1]: 528 tiles x 11 pieces on 512 workgroup slots = 11.34 rounds, paid as
// 12), while finer pieces at the end fill the slots that fall free there, and the launch ends within one SMALL piece of
// (total work / slots).  Returns the number of pieces.  Depends on the depth and the two counts alone (sig_piece_counts below: chosen
// from the full problem's size), so an entry's summation order is the same in every tile, row block and rank.
inline int sig_piece_bounds(int nslab, int equal, int graded, int* bound) {
    if (equal < 1) equal = 1;
    if (equal > nslab) equal = nslab < 1 ? 1 : nslab;
    int n = 0;
    for (int s = 0; s < equal - 1; ++s) bound[n++] = int(int64_t(nslab) * s / equal);
    const int last0 = int(int64_t(nslab) * (equal - 1) / equal), len = nslab - last0;
    bound[n++] = last0;
    if (graded > 1 && len >= 2 * graded) {
        int at = last0, left = len;
        for (int g = 1; g < graded; ++g) {         // 1/2, 1/4, ... of the last piece; the final one takes what is left
            const int take = left / 2 > 0 ? left / 2 : 1;
            at += take; left -= take;
            bound[n++] = at;
        }
    }
    bound[n] = nslab;
    return n;
}

constexpr int SIG_PIECE_TILE = 128;        // the contraction's tile edge (sig_feat_kernel.hpp: SG_BM == SG_BN; sig_feat_api.hip asserts it)

// Workgroups per tile along the depth.  One piece per tile leaves a launch of a few hundred tiles with a nearly empty last round
// (528 tiles on the chip's 512 workgroup slots: two rounds) and a launch of a few tiles with most of the chip idle; many pieces cost
// a partial sum each to write and add (the whole result once per piece).  The count minimises a small model of the launch --
// rounds of 512 workgroups x (slabs per piece x 3.6 us + 10 us; 1.8 us per slab while no CU holds two workgroups) + 2 x pieces x result bytes at 3 TB/s --
// evaluated for the FULL problem (the Gram's total size N1 x (sym ? N1 : N2) and the depth nslab_all), not for the tiles of one call: the order
// in which an entry's products are added is then the same whichever tile, row block or rank computes it, and row blocks
// (gpsig_kernel_K_symm_rows*) reassemble the one-call Gram bit for bit.  16 pieces at N = 4,096 (configs[1]); large Grams keep
// at least 4 (a rank's chunk of one is a launch of ~1,000 tiles); pieces of at least 8 slabs.
// *nsplit: equal depth pieces; *graded: the last of them cut into that many finer ones (sig_piece_bounds); graded_on: option "sig_graded".
inline void sig_piece_counts(int64_t N1, int64_t N2, bool sym, int nslab_all, bool graded_on, int* nsplit_out, int* graded_out) {
    int nsplit = 1, graded = 1;
    const int64_t nt_full = (N1 + SIG_PIECE_TILE - 1) / SIG_PIECE_TILE;
    const int64_t tiles_full = sym ? nt_full * (nt_full + 1) / 2 : nt_full * ((N2 + SIG_PIECE_TILE - 1) / SIG_PIECE_TILE);
    const double result_bytes = 8.0 * double(N1) * double(sym ? N1 : N2) * (sym ? 0.5 : 1.0);
    double best = 1e300;
    for (int ns = 1; ns <= 128 && ns * 8 <= nslab_all + 7; ++ns) {
        const double wgs = double(tiles_full) * ns, per_piece = double(nslab_all) / ns;
        const double t = (wgs <= 256.0 ? per_piece * 1.8e-6 + 10e-6 : ceil(wgs / 512.0) * (per_piece * 3.6e-6 + 10e-6)) +
                         (ns > 1 ? 2.0 * ns * result_bytes / 3e12 : 0.0);          // (a piece's sum is written, then read)
        if (t < best * 0.999) { best = t; nsplit = ns; }
    }
    if (tiles_full > 1024 && nsplit < 4 && nslab_all >= 32) nsplit = 4;
    // Equal pieces end in a last round of workgroups that takes as long as the others but is only partly full (configs[1]: 528 tiles
    // x 11 pieces = 11.34 rounds of 512, paid as 12).  Cutting the LAST piece into finer ones of halving size (sig_piece_bounds) lets
    // the launch end within one small piece of (total work / slots): the waste of the equal pieces' last round against the finest
    // piece plus a partial sum per extra piece (round 4; option "sig_graded" 0 keeps the equal pieces).
    const double wgs = double(tiles_full) * nsplit, piece_t = double(nslab_all) / nsplit * 3.6e-6;
    if (graded_on && wgs > 512.0 && nslab_all / nsplit >= 32) {
        const double rounds = wgs / 512.0, waste_equal = (ceil(rounds) - rounds) * piece_t;
        double best_t = waste_equal;
        for (int g = 2; g <= 5; ++g) {
            const double t = piece_t / double(1 << (g - 1)) + (g - 1) * 2.0 * result_bytes / 3e12;
            if (t < best_t * 0.95 && (nslab_all / nsplit) >> (g - 1) >= 8) { best_t = t; graded = g; }
        }
    }
    *nsplit_out = nsplit;
    *graded_out = graded;
}

}  // namespace gpsig
