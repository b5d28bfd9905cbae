// Body of k_tube_adam and k_tube_adam_sweep (tube_kernels.hip), included inside each kernel.  Names it takes from the including
// kernel: D (the kernel's TubeDev argument, or a sweep kernel's TubeDevView), nwg (int), t (int64_t), lr0, gamma (double), step_size (int64_t),
// norm (float), rows (int64_t).  The blocks along x share one model; its done_ctr / normpart tell the last of them to write the log.
// It returns early in all blocks but the last, so it must be the last thing in the kernel.
//
// Why a fragment and not a function: inside a `__device__ __forceinline__` function blockDim.x lost the kernel's
// uniform-work-group-size form (a load of the group size became a compare of the block index against the grid, a select and a
// 16-bit load), and k_tube_adam grew from 2020 to 2039 lines of gfx950 assembly.  tube_rows_tile.inl says how the comparison is made.
    __shared__ float red[256];
    __shared__ bool last;
    const int64_t P = D.num_params;
    const double lr = lr0 * pow(gamma, (double)((t - 1) / step_size));
    const double bc1 = 1.0 - pow(0.9, (double)t), bc2 = 1.0 - pow(0.999, (double)t);
    const float neg_step = (float)(-(lr / bc1)), bc2s = (float)sqrt(bc2);
    float sq = 0.f;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
        float g = 0.f;
        for (int w = 0; w < nwg; ++w) g += D.slab[(size_t)w * D.slab_ld + p];
        D.grads[p] = g;
        sq = fmaf(g, g, sq);
        float m = D.adam_m[p], v = D.adam_v[p];
        m = m + 0.1f * (g - m);                       // exp_avg.lerp_(grad, 1 - beta1)
        v = v * 0.999f + 0.001f * g * g;              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) / bc2s + 1e-8f;
        const float np = D.params[p] + neg_step * (m / denom);
        D.adam_m[p] = m; D.adam_v[p] = v; D.params[p] = np;
        for (int li = 0; li <= D.layers; ++li) {      // keep the transposed weight copy current
            const int64_t o = p - D.off_w[li];
            if (o >= 0 && o < (int64_t)D.din[li] * D.dout[li]) {
                const int K = D.din[li], N = D.dout[li], j = (int)(o / K), k = (int)(o - (int64_t)j * K);
                D.wt[D.off_w[li] + (int64_t)k * N + j] = np;
            }
        }
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        D.normpart[blockIdx.x] = red[0];
        __threadfence();
        last = atomicAdd(D.done_ctr, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    float n2 = 0.f, ls = 0.f;
    for (unsigned b = 0; b < gridDim.x; ++b) n2 += __hip_atomic_load(D.normpart + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int w = 0; w < nwg; ++w) ls += D.slab[(size_t)w * D.slab_ld + P];
    float *lg = D.log + (size_t)((t - 1) % D.log_cap) * 4;
    lg[0] = ls / norm;
    lg[1] = (float)(lr0 * pow(gamma, (double)(t / step_size)));   // get_last_lr() after lr_scheduler.step()
    lg[2] = sqrtf(n2);
    lg[3] = (float)rows;
    atomicExch(D.done_ctr, 0u);
