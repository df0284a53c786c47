// The per-element statements that the entropy-model kernels of entropy.hip and hyperprior.hip must agree on to the bit, in device
// code: the Gaussian likelihood of a centred value with its backward, and the Philox4x32-10 noise stream with the rule that maps
// an element to its counter and word.  The kernels keep their own loads, quantisation, grids and records and call these leaves.
#pragma once
#include "stem_common.h"

// ---- GaussianConditional (entropy_models.py:570-596) ----------------------------------------------------------------------------
__device__ __forceinline__ float std_cum(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }

// likelihood of a value at distance v = |out - mu| from its mean, both LowerBounds applied
__device__ __forceinline__ float gauss_lik(float v, float sc, float scale_bound, float lik_bound)
{
    const float s = fmaxf(sc, scale_bound);
    return fmaxf(std_cum((0.5f - v) / s) - std_cum((-0.5f - v) / s), lik_bound);
}

// backward of gauss_lik for d = out - mu and g = d loss / d likelihood: ds = d loss / d scale, dvs = d loss / d out (the caller
// writes dy = dvs or dmeans = -dvs, exact negations of each other), both LowerBound pass-through rules (bound_ops.py:28-31) applied;
// -> max(|ds|, |dv|), the element's entry in the scale record of (dscales | dmeans).
// Contraction is off in this body.  When each kernel carried its own copy of these lines, the stand-alone backward kernel and the
// fused training forward came out of the compiler rounding pa * a and pb * b separately (one packed multiply held both, so neither
// was fused into the subtraction): an accident of code generation that the copies had to meet alike.  Four elements side by side
// (the float4 kernel of hyperprior.hip) got a packed FMA for pa * a - pb * b instead, and so did this function inlined into the
// fused training forward under default contraction (one v_pk_mul_f32 fewer, one FMA more), which moves dscales by 1 - 2 ulp
// against the stand-alone kernel.  With the pragma every product and every difference is rounded wherever the function is inlined:
// the bits all callers produced before, now by statement (tests/test_hip_train_tail.py, tests/test_hip_hyperprior_ops.py).
__device__ __forceinline__ float gauss_bwd_elem(float d, float sc, float g, float scale_bound, float lik_bound, float &ds_out, float &dvs_out)
{
#pragma clang fp contract(off)
    const float v = fabsf(d);
    const float s = fmaxf(sc, scale_bound);
    const float a = (0.5f - v) / s, b = (-0.5f - v) / s;
    const float lraw = std_cum(a) - std_cum(b);
    if (!(lraw >= lik_bound || g < 0.f)) g = 0.f;
    const float k = 0.39894228040143267794f;
    const float pa = k * expf(-0.5f * a * a), pb = k * expf(-0.5f * b * b);
    const float dv = g * (-(pa - pb) / s);
    float ds = g * (-(pa * a - pb * b) / s);
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (!(sc >= scale_bound || ds < 0.f)) ds = 0.f;
    ds_out = ds;
    dvs_out = dv * sgn;
    return fmaxf(fabsf(ds), fabsf(dv));
}

// ---- noise: Philox4x32-10, counter (ctr, 0, 0), key (seed_lo, seed_hi) --------------------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1)
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// the four values of one counter: the top 24 bits of each word as a uniform in [-1/2, 1/2)
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t ctr, float r[4])
{
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const uint32_t v[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)(v[e] >> 8) * (1.0f / 16777216.0f) - 0.5f;
}

struct NoiseSrc {            // either an explicit tensor (parity tests, injected sources) or the Philox stream (seed, offset [+ epoch * stride])
    const float *ptr;
    uint64_t seed, offset, stride;
    const long long *epoch;
};
// epoch != nullptr: the counter additionally advances by epoch[0] * stride, a device-resident draw count, so that a captured
// hipGraph produces fresh noise on every replay (the host-side offset is frozen into the graph at capture)
__device__ __forceinline__ uint64_t noise_base(const NoiseSrc &s) { return s.offset + (s.epoch ? (uint64_t)s.epoch[0] * s.stride : 0); }

// the noise of dense element i, which sits at offset_of_i of the explicit tensor: that tensor's value, else word i & 3 of counter
// base + (i >> 2) -- what stem_uniform_noise writes to element i of a dense tensor
__device__ __forceinline__ float noise_at(const NoiseSrc &s, size_t i, size_t offset_of_i)
{
    if (s.ptr) return s.ptr[offset_of_i];
    float r[4];
    philox4(s.seed, noise_base(s) + (i >> 2), r);
    return r[i & 3];
}
