// Tile constants of the Cholesky kernels (every sequence; sf_chol.hip includes the layers in dependency order).
#pragma once

#define GT 128  // C tile edge of the MFMA kernel
#define GK 16   // K slab staged in LDS per step
#define GLD 17  // LDS row stride (doubles), odd: the 16 rows of a fragment hit 16 distinct bank pairs for
                // ds_read_b64 (64 banks) and ds_read2_b64 (32 banks) alike

// 16 x 16 blocks of the diagonal-tile kernels (k_diag_mfma, k_diag_lds) as they sit in LDS
#define DBS (16 * 17)  // doubles per block
#define DLD 17         // row stride (doubles), odd as GLD

#define CLD 33  // row stride (doubles) of the 128 x 32 chunk buffer
