// nk_solid.h -- the solid fraction of the field's cells (nk_cell_solid_volume): what the host hands the two kernels of
// nk_solid.hip.  A set-up helper beside the engine, without a context: this header reads none of the engine's.
#pragma once
#include <stdint.h>

// k_solid_clip: one single-wave workgroup, each lane with two polygons of its own in LDS
#define NK_SOLID_WG 64
// vertices a stored polygon can have: a triangle, plus one per clip, five clips stored (the sixth is consumed as it is made)
#define NK_SOLID_MAXV 8

struct NkSolidDev {
    const double *tri;          // [nf * 9] the triangles in grid units u = (x - lo) / h, snapped into [0, n]
    const int32_t *rng;         // [nf * 6] cells offered to every triangle: first ix, iy, iz, last ix, iy, iz
    const int64_t *first;       // [nf + 1] the first (triangle, column) pair of every triangle; first[nf] = pairs
    int64_t pairs;
    int32_t nf;
    int32_t n[3];
    double sA, sP;              // 2^k_A, 2^k_P
    unsigned long long *A, *P;  // [ncells] sums of a 2^k_A and p 2^k_P (two's complement)
};
