// Prints the tile plan of the evaluation side's tiled low-rank feature kernels (csrc/lr_tile_plan.hpp: lr_eval_tile_dir) for the shapes given
// on the command line, one line per shape: "f32 c r d l pad" in, "TL ntiles lp lds whole" out (whole: the whole-sequence footprint of the
// element type at l + 1 points).  tests/test_lowrank_eval_long_host.py recomputes the numbers.
#include <cstdio>
#include <cstdlib>

#include "lr_tile_plan.hpp"

int main(int argc, char** argv) {
    using namespace gpsig;
    for (int i = 1; i + 5 < argc; i += 6) {
        const int f32 = std::atoi(argv[i]), c = std::atoi(argv[i + 1]), r = std::atoi(argv[i + 2]), d = std::atoi(argv[i + 3]),
                  l = std::atoi(argv[i + 4]), pad = std::atoi(argv[i + 5]);
        const LrTileDir D = lr_eval_tile_dir(f32 != 0, c, r, d, l, pad);
        const size_t whole = lr_fused_lds_bytes(c, r, d, l + 1, pad) / (f32 ? 2 : 1);
        std::printf("%d %d %d %zu %zu\n", D.TL, D.ntiles, D.lp, D.lds, whole);
    }
    return 0;
}
