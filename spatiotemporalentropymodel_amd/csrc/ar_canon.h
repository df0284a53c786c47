// The canonical product of the coding loops, in device code: the one place where the arithmetic that include/stem_ar_batch.h states
// ("the canonical product") is written for the GPU.  The kernels of ar.hip, ar_persistent.hip, symbols.hip and build_indexes_kernel
// (entropy.hip) keep their own loops, loads and grids and call these leaves; tests/ar_ref.py is the same statement in numpy.
//
// Every function that does floating-point arithmetic turns contraction off in its own body: the rounding of each product and each sum
// belongs to the function, not to where the header happens to be included (entropy.hip contracts above its own pragma, and must go on
// doing so).
#pragma once
#include "stem_common.h"

// one 16-byte step of a lane's partial sum: ((x0 w0 + x1 w1) + x2 w2) + x3 w3, every product and every sum rounded
__device__ __forceinline__ float dot4(const f32x4 xv, const f32x4 wv)
{
#pragma clang fp contract(off)
    return xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
}

// the xor butterfly over the 64 lane accumulators, off = 32 .. 1: every lane returns the sum
__device__ __forceinline__ float wave_sum(float acc)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// y = sum + bias, then v > 0 ? v : v * slope for STEM_ACT_LRELU
__device__ __forceinline__ float finish(float sum, float bias, int act, float slope)
{
#pragma clang fp contract(off)
    float v = sum + bias;
    if (act == STEM_ACT_LRELU) v = v > 0.f ? v : v * slope;
    return v;
}

// the scale-to-index search: T - 1 - #{t < T - 1 : max(scale, bound) <= table[t]}
__device__ __forceinline__ int scale_index(float scale, float bound, const float *table, int T)
{
    const float s = fmaxf(scale, bound);
    int k = T - 1;
    for (int t = 0; t < T - 1; ++t) k -= (s <= table[t]) ? 1 : 0;
    return k;
}

// rounding to the nearest integer, ties to even: a symbol as a float
__device__ __forceinline__ float round_ties_even(float v) { return rintf(v); }

// q = rintf(pix - mean), the symbol as a float ((int32_t)q is what is coded) -> y_hat = q + mean
__device__ __forceinline__ float quantise(float pix, float mean, float &q)
{
#pragma clang fp contract(off)
    q = round_ties_even(pix - mean);
    return q + mean;
}

// the decoder's y_hat = (float)symbol + mean: the float `quantise` returned
__device__ __forceinline__ float dequantise(int32_t sym, float mean)
{
#pragma clang fp contract(off)
    return (float)sym + mean;
}

// ---- wavefront steps (include/stem_ar_batch.h, "wavefront symbol order") ------------------------------------------------------------
// step t of an H x Wd latent holds rows h0 .. h0 + np - 1, position p of the step being (h0 + p, t - 3 (h0 + p)); np <= 0 for the steps
// between two rows of a latent with Wd < 3
__host__ __device__ __forceinline__ void wave_range(int t, int H, int Wd, int &h0, int &np)
{
    int lo = t - (Wd - 1);
    lo = lo > 0 ? (lo + 2) / 3 : 0;
    int hi = t / 3;
    if (hi > H - 1) hi = H - 1;
    h0 = lo;
    np = hi - lo + 1;
}

// positions in steps 0 .. t-1: row h' holds min(max(t - 3h', 0), Wd) of them
__host__ __device__ __forceinline__ long wave_positions_before(int t, int H, int Wd)
{
    long n = 0;
    for (int h = 0; h < H && 3 * h < t; ++h) n += t - 3 * h < Wd ? t - 3 * h : Wd;
    return n;
}

// element i of step t of G images, one thread per (image, position of the step, channel): i = (g * np + p) * M + c
struct WaveElem {
    int g, p, c;     // image, position within the step, channel
    int h, w;        // the position in the latent
};
// false for the threads beyond the step's G * np * M elements
__device__ __forceinline__ bool wave_elem(int i, int t, int H, int Wd, int M, int G, WaveElem &e)
{
    int h0, np;
    wave_range(t, H, Wd, h0, np);
    if (i >= G * np * M) return false;
    const int j = i / M;
    e.c = i - j * M;
    e.g = j / np;
    e.p = j - e.g * np;
    e.h = h0 + e.p;
    e.w = t - 3 * e.h;
    return true;
}
