// The HIP-free part of the shared declarations (internal): status codes, the error text and the constants of the host
// numerics.  sf_common.h and sf_transform.h include it; sf_hostmath.cpp and sf_error.cpp include nothing else of the library.
#pragma once
#include "../../include/starfish_amd.h"

#define SF_C_KMS 2.99792458e5
#define SF_KB 5      // sub/super-diagonals stored for the quintic collocation LU
#define SF_IW 64     // half-width of the truncated inverse of the collocation matrix (decay ~0.43^k: < 1e-23)

void sf_set_error(const char* fmt, ...);  // text of sf_last_error(), per calling thread (sf_error.cpp)
