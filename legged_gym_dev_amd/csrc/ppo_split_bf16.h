// Split-bf16 ("bf16x6") arithmetic shared by every kernel that computes an fp32 product on the bf16 matrix cores (ppo_gemm.hip,
// ppo_gemm_glds.h, ppo_mlp_fused.hip), and the hidden-layer activations their epilogues apply.  One copy of each: the results of
// those kernels are bit-identical to one another only as long as they split the same way and sum the same products in the same order.
//
// Each fp32 operand is split exactly into three bf16 terms x = h + m + l (round-to-nearest at each level: |m| <= 2^-8 |x|,
// |l| <= 2^-16 |x|, and the 24-bit significand is covered, so the split itself loses nothing).  The product a.b is summed from
// the six term products of weight >= 2^-16 (X6_TERMS), each EXACT in the fp32 accumulator of v_mfma_f32_32x32x16_bf16; the three
// dropped ones (ml, lm, ll) are <= 2^-23 |ab| worst case and unbiased -- below one fp32 rounding of the product.
#pragma once
#include <cstdint>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (x0, x1) -> packed bf16 pairs of the three split terms
__device__ __forceinline__ void split2(float x0, float x1, uint32_t &h, uint32_t &m, uint32_t &l) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));      // v_pk_add_f32: both remainders in one instruction
    h = cvt_pk_bf16(x0, x1);
    f32x2 r = f32x2{x0, x1} - f32x2{__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
    m = cvt_pk_bf16(r.x, r.y);
    r -= f32x2{__uint_as_float(m << 16), __uint_as_float(m & 0xffff0000u)};
    l = cvt_pk_bf16(r.x, r.y);
}
// 8 consecutive floats (lo, hi) -> the three bf16x8 terms
__device__ __forceinline__ void split8(const float4 &lo, const float4 &hi, bf16x8 &h, bf16x8 &m, bf16x8 &l) {
    uint32_t hh[4], mm[4], ll[4];
    split2(lo.x, lo.y, hh[0], mm[0], ll[0]);
    split2(lo.z, lo.w, hh[1], mm[1], ll[1]);
    split2(hi.x, hi.y, hh[2], mm[2], ll[2]);
    split2(hi.z, hi.w, hh[3], mm[3], ll[3]);
    h = __builtin_bit_cast(bf16x8, make_uint4(hh[0], hh[1], hh[2], hh[3]));
    m = __builtin_bit_cast(bf16x8, make_uint4(mm[0], mm[1], mm[2], mm[3]));
    l = __builtin_bit_cast(bf16x8, make_uint4(ll[0], ll[1], ll[2], ll[3]));
}

// The six term products (A term, B term; 0 = h, 1 = m, 2 = l) in the order they are added to the accumulator: smallest first.
struct X6Term { int a, b; };
constexpr X6Term X6_TERMS[6] = {{1, 1}, {0, 2}, {2, 0}, {0, 1}, {1, 0}, {0, 0}};
// acc += a . b over the six term products of one fragment pair (a[3], b[3]: the h, m, l terms)
__device__ __forceinline__ f32x16 mfma_x6(const bf16x8 *a, const bf16x8 *b, f32x16 acc) {
#pragma unroll
    for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[X6_TERMS[t].a], b[X6_TERMS[t].b], acc, 0, 0, 0);
    return acc;
}

// One bf16x8 MFMA operand (8 consecutive k of one column) from a k-major LDS image through gfx950's transposing LDS read: two
// ds_read_b64_tr_b16, each 4 k x 16 columns per 16-lane group, at this lane's addresses of the two 4-k halves.
__device__ __forceinline__ bf16x8 lds_read_tr_frag(const unsigned char *lo, const unsigned char *hi) {
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)lo);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)hi);
    const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// Workgroup barrier of the GEMM mainloops: LDS traffic only.  __syncthreads() carries workgroup-scope fences, for which hipcc drains
// EVERY outstanding memory operation (s_waitcnt vmcnt(0)) -- including the global loads issued two k-tiles ahead, whose latency
// the prefetch distance exists to hide.  The mainloops exchange data through LDS alone: waiting for this wave's LDS operations
// and the barrier is all the ordering they need; the loaded registers are waited for where they are used (counted vmcnt).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Hidden-layer activations of rsl_rl's get_activation (ActorCritic cfg `activation`, legged_robot_config.py:244):
// code 0 none, 1 elu, 2 selu, 3 relu, 4 lrelu (slope 0.01), 5 tanh, 6 sigmoid.  act_bwd is the derivative expressed
// through the activation's OUTPUT a (the only thing the forward pass keeps).
#define SELU_L 1.0507009873554804934193349852946f
#define SELU_LA (1.0507009873554804934193349852946f * 1.6732632423543772848170429916717f)
__device__ __forceinline__ float act_fwd(int code, float v) {
    switch (code) {
    case 1: return v > 0.f ? v : __expf(v) - 1.0f;
    case 2: return v > 0.f ? SELU_L * v : SELU_LA * (__expf(v) - 1.0f);
    case 3: return fmaxf(v, 0.f);
    case 4: return v > 0.f ? v : 0.01f * v;
    case 5: return 2.0f * __frcp_rn(1.0f + __expf(-2.0f * v)) - 1.0f;
    case 6: return __frcp_rn(1.0f + __expf(-v));
    default: return v;
    }
}
__device__ __forceinline__ float act_bwd(int code, float a) {
    switch (code) {
    case 1: return a > 0.f ? 1.0f : a + 1.0f;
    case 2: return a > 0.f ? SELU_L : a + SELU_LA;
    case 3: return a > 0.f ? 1.0f : 0.f;
    case 4: return a > 0.f ? 1.0f : 0.01f;
    case 5: return 1.0f - a * a;
    case 6: return a * (1.0f - a);
    default: return 1.0f;
    }
}
