// What lg_tube_rows_build hands to the kernels of tube_data_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TD_CHUNK 64                 // steps per chunk: one wave

struct TubeRowsP {
    const float *z, *pz, *v;
    const uint8_t *done;
    float *data, *target;
    int64_t *n_rows;
    const int64_t *offs;
    int64_t nchunks;
    int32_t n_env, T, cpe;          // cpe: chunks per env
    int32_t kind, N, dN, recursive, n, m;
    int32_t compact, mark, epoch_envs;
    int32_t I, O, bw, L, nz, zoff;  // block: L leading error columns, nz columns of z from zoff, m of v
};

extern "C" {
void tubedatak_rows(const TubeRowsP *P, int32_t *counts, int64_t *offs, hipStream_t st);
void tubedatak_horizon(const float *z, const float *pz, const float *v, int64_t n_env, int T, int n, int m, int H, float *w,
                       float *znp, float *vpad, hipStream_t st);
}
