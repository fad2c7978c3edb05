// Prints the shape helpers of the full banded solve (starfish_amd/csrc/sf_band_shape.h) for every (half-width, nrhs) the LDS
// window admits, with the window's own figures beside them; tests/test_banded_gradient_host.py compiles and runs it and compares
// with a restatement in Python.  One line per shape:
//   w nrhs nbr nrb window_lds_bytes | column_blocks block(3,2) doubles(n=1000) | T part doubles bytes | nwaves blocks_per_wave
// then one line "max" with sf_band_max_halfwidth(nrhs), nrhs = 1 .. 49.
#include <cstdio>

#include "sf_band_shape.h"

int main() {
    for (int w = 0; w <= 176; ++w)
        for (int nrhs = 1; nrhs <= 49; ++nrhs) {
            if (sfb_admit(w, nrhs) != SFB_WINDOW) continue;
            const int nbr = sfb_nbr(w), nrb = sfb_nrb(nrhs);
            const sfb_back_lds L = sfb_back_lds_layout(nbr, nrb);
            std::printf("%d %d %d %d %zu %d %zu %zu %d %d %d %zu %d %d\n", w, nrhs, nbr, nrb, sfb_lds_layout(nbr, nrb).bytes,
                        sfb_keep_column_blocks(nbr, nrb), sfb_keep_block(3, 2, nbr, nrb), sfb_keep_doubles(1000, nbr, nrb), L.T, L.part,
                        L.doubles, L.bytes, sfb_back_nwaves(nrb), sfb_back_blocks_per_wave(nbr));
        }
    std::printf("max");
    for (int nrhs = 1; nrhs <= 49; ++nrhs) std::printf(" %d", sf_band_max_halfwidth(nrhs));
    std::printf("\n%d %d %d\n", SFB_BACK_SPLIT, SFB_BACK_MAX_BLOCKS, SFB_LDS_MAX);
    return 0;
}
