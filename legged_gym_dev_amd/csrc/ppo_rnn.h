// Arguments of the LSTM kernels (ppo_rnn.hip).  Index 0 = memory_a (actor), 1 = memory_c (critic) on blockIdx.z.
#pragma once
#include <stdint.h>

struct RnnNetArgs {
    const float *X; int ldx, K;            // input rows [M][ldx], K = input width; K = 0: the input part comes from P
    const float *P; int ldp;               // x . W_ih^T + b_ih per row (4H wide), computed beforehand; nullptr: from X here
    const float *Wih, *Whh, *bih, *bhh;    // [4H][K], [4H][H], [4H], [4H]
    const float *h_prev, *c_prev;          // state of the previous step, row r (nullptr: every row starts from h_sv / c_sv)
    const float *h_sv, *c_sv;              // saved state, row r: where the row reloads
    float *h_out, *c_out;                  // new state [M][H]; must not alias any input state
    float *gates;                          // stash for the backward pass: sigma(i), sigma(f), tanh(g), sigma(o) [M][4H] (or nullptr)
    float *h_used, *c_used;                // stash: the state the step started from [M][H] (or nullptr)
};
struct RnnStepArgs {
    RnnNetArgs n[2];
    const uint8_t *reload;                 // per row: the row starts from its saved state (done at the previous step)
    int reload_all;                        // every row reloads (first step of a sequence)
    int M, H;                              // rows, hidden size (multiple of 32)
};

struct RnnBwdNet {
    const float *dG_next;                  // dG of the next step [M][4H] (nullptr: last step)
    const float *Whh;
    const float *dh_mlp;                   // dL/dh from the MLP on this step's output [M][H]
    float *dc;                             // cell-state carry [M][H]: in f_{t+1} dc_{t+1}, out f_t dc_t (zero where this step reloaded)
    const float *gates, *c_t, *c_used;     // this step's stash, cell output and the cell state it started from
    float *dG;                             // out: pre-activation gate gradients [M][4H]
};
struct RnnBwdArgs {
    RnnBwdNet n[2];
    const uint8_t *cut_next;               // per row: the next step reloaded (no gradient flows back across it)
    const uint8_t *cut;                    // per row: this step reloaded
    int cut_all;                           // this step is the first of the sequence
    int M, H;
};

struct RnnBiasArgs {
    const float *dG[2];
    float *db_ih[2], *db_hh[2];
    int M, H;
};
