// Device passes of the zero-mean members of the hyper-prior family ("bmshj2018-hyperprior": compressai/models/priors.py:196-313):
//   gc_scale forward / backward: GaussianConditional.forward(inputs, scales, means=None) and its gradient in one launch each --
//                                entropy.hip's gc_forward_kernel / gc_backward_kernel without the mean tensor, the noise drawn inline
//                                (as gc_forward_train_kernel draws it) and the gradient arriving at `out` added while dy is written
//   abs forward / backward:      the |y| in front of h_a (priors.py:258)
// All fp32 NHWC with a pixel pitch per tensor (channel-slice views need no copy), all HBM-bound, no atomics: every output element
// has exactly one writer.  Where the channel count and every pitch of a call are multiples of 4 (and the bases 16-byte aligned)
// a thread moves one float4 per tensor; any other call takes one float per thread.
//
// The per-element expressions and the noise stream are the header's (entropy_elem.h: gauss_lik, gauss_bwd_elem, noise_at), the ones
// the mean kernels of entropy.hip call, here with the centred value d = out (a zero mean): the results compare equal to the mean
// kernels fed zeros, and the backward's bit for bit (tests/test_hip_hyperprior_ops.py).  The one place where a zero mean is NOT the
// identity is the eval-mode output: rintf(y - 0) + 0 turns -0.0 into +0.0, rintf(y) keeps it, which is what the reference's
// means=None branch returns -- so the quantisation is written here.
#include "stem_common.h"
#include "entropy_elem.h"
#include "../../include/stem_hyperprior.h"

namespace {

// ---- one element: quantise (noise nv | round), then the likelihood at |out| ---------------------------------------------------
__device__ __forceinline__ void gcs_forward_elem(float yv, float nv, float sc, int mode, float sb, float lb, float &o, float &lik)
{
    o = mode == 0 ? yv + nv : rintf(yv);
    lik = gauss_lik(fabsf(o), sc, sb, lb);
}

// ---- addressing: logical element i = pix * C + c of a tensor with pixel pitch ld ------------------------------------------------
struct Pitches {
    int C, dense;            // dense: every pitch of the call equals C, element i sits at offset i
};
__device__ __forceinline__ void locate(const Pitches &p, size_t i, size_t &pix, int &c)
{
    if (p.dense) {
        pix = 0;
        c = 0;
        return;
    }
    pix = i / p.C;
    c = (int)(i - pix * p.C);
}
__device__ __forceinline__ size_t at(const Pitches &p, size_t i, size_t pix, int c, int ld) { return p.dense ? i : pix * ld + c; }

// ---- forward ----------------------------------------------------------------------------------------------------------------
// VEC: one float4 of every tensor per thread (C % 4 == 0: the four elements belong to one pixel); else one float
template <bool VEC>
__global__ __launch_bounds__(256) void gc_scale_forward_kernel(const float *__restrict__ y, int ldy, NoiseSrc nl, int ldn,
                                                               const float *__restrict__ scales, int lds, float *__restrict__ out,
                                                               int ldo, float *__restrict__ lik, int ldl, size_t n, Pitches p,
                                                               int mode, float sb, float lb)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = VEC ? t * 4 : t;
    if (i >= n) return;
    size_t pix;
    int c;
    locate(p, i, pix, c);
    if (VEC) {
        const f32x4 yv = *reinterpret_cast<const f32x4 *>(y + at(p, i, pix, c, ldy));
        const f32x4 sc = *reinterpret_cast<const f32x4 *>(scales + at(p, i, pix, c, lds));
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (mode == 0) {
            if (nl.ptr) {
                const f32x4 nv = *reinterpret_cast<const f32x4 *>(nl.ptr + at(p, i, pix, c, ldn));
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = nv[e];
            } else {
                philox4(nl.seed, noise_base(nl) + (i >> 2), r);
            }
        }
        f32x4 o, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float oe, le;
            gcs_forward_elem(yv[e], r[e], sc[e], mode, sb, lb, oe, le);
            o[e] = oe;
            l[e] = le;
        }
        *reinterpret_cast<f32x4 *>(out + at(p, i, pix, c, ldo)) = o;
        *reinterpret_cast<f32x4 *>(lik + at(p, i, pix, c, ldl)) = l;
    } else {
        const float nv = mode == 0 ? noise_at(nl, i, at(p, i, pix, c, ldn)) : 0.f;
        float o, l;
        gcs_forward_elem(y[at(p, i, pix, c, ldy)], nv, scales[at(p, i, pix, c, lds)], mode, sb, lb, o, l);
        out[at(p, i, pix, c, ldo)] = o;
        lik[at(p, i, pix, c, ldl)] = l;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// The scale record has one slot per 256 logical elements whichever path runs (it is gc_backward_kernel's record): the scalar
// path's workgroup owns one slot (record_block_max), the vector path's owns four, one per wave (64 lanes x 4 elements).
template <bool VEC>
__global__ __launch_bounds__(256) void gc_scale_backward_kernel(const float *__restrict__ out, int ldo, const float *__restrict__ scales,
                                                                int lds, const float *__restrict__ dlik, int ldl,
                                                                const float *__restrict__ dout, int ldg, float *__restrict__ dsc,
                                                                int ldds, float *__restrict__ dy, int lddy, size_t n, Pitches p,
                                                                float sb, float lb, float *__restrict__ q)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = VEC ? t * 4 : t;
    float m = 0.f;
    if (i < n) {
        size_t pix;
        int c;
        locate(p, i, pix, c);
        if (VEC) {
            const f32x4 o = *reinterpret_cast<const f32x4 *>(out + at(p, i, pix, c, ldo));
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(scales + at(p, i, pix, c, lds));
            const f32x4 g = *reinterpret_cast<const f32x4 *>(dlik + at(p, i, pix, c, ldl));
            f32x4 ds, d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float dse, de;
                m = fmaxf(m, gauss_bwd_elem(o[e], sc[e], g[e], sb, lb, dse, de));
                ds[e] = dse;
                d[e] = de;
            }
            if (dsc) *reinterpret_cast<f32x4 *>(dsc + at(p, i, pix, c, ldds)) = ds;
            if (dy) {
                if (dout) {
                    const f32x4 u = *reinterpret_cast<const f32x4 *>(dout + at(p, i, pix, c, ldg));
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = __fadd_rn(d[e], u[e]);
                }
                *reinterpret_cast<f32x4 *>(dy + at(p, i, pix, c, lddy)) = d;
            }
        } else {
            float ds, d;
            m = gauss_bwd_elem(out[at(p, i, pix, c, ldo)], scales[at(p, i, pix, c, lds)], dlik[at(p, i, pix, c, ldl)], sb, lb, ds, d);
            if (dsc) dsc[at(p, i, pix, c, ldds)] = ds;
            if (dy) dy[at(p, i, pix, c, lddy)] = dout ? __fadd_rn(d, dout[at(p, i, pix, c, ldg)]) : d;
        }
    }
    if (!q) return;
    if (VEC) {
        m = wave_max(m);
        const size_t slot = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nslots = (n + 255) / 256;
        if ((threadIdx.x & 63) == 0 && slot < nslots) q[QREC_HDR + slot] = m;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            q_header(q, (int)nslots);
            q[1] = 1.f;
        }
    } else {
        record_block_max(q, m);
    }
}

// ---- |x| ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float abs_grad(float x, float g) { return g * (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)); }

// grid-stride over float4s (VEC) or floats; g == nullptr: out = |x|, else out = g * sign(x)
template <bool VEC>
__global__ __launch_bounds__(256) void abs_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ g, int ldg,
                                                  float *__restrict__ out, int ldo, size_t n, Pitches p)
{
    const size_t step = (size_t)gridDim.x * 256 * (VEC ? 4 : 1);
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1); i < n; i += step) {
        size_t pix;
        int c;
        locate(p, i, pix, c);
        if (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + at(p, i, pix, c, ldx));
            f32x4 o;
            if (g) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + at(p, i, pix, c, ldg));
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = abs_grad(xv[e], gv[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fabsf(xv[e]);
            }
            *reinterpret_cast<f32x4 *>(out + at(p, i, pix, c, ldo)) = o;
        } else {
            const float xv = x[at(p, i, pix, c, ldx)];
            out[at(p, i, pix, c, ldo)] = g ? abs_grad(xv, g[at(p, i, pix, c, ldg)]) : fabsf(xv);
        }
    }
}

constexpr unsigned ABS_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups: the rest is grid-strided

inline bool aligned16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }
// a tensor that is absent (ptr == nullptr) constrains nothing
inline bool vec_ok(const void *ptr, int ld) { return !ptr || (ld % 4 == 0 && aligned16(ptr)); }
inline bool pitch_ok(const void *ptr, int ld, int C) { return !ptr || ld >= C; }
inline bool is_dense(const void *ptr, int ld, int C) { return !ptr || ld == C; }

}   // namespace

STEM_EXPORT int stem_gc_scale_forward(const float *y, int ldy, const float *noise, int ldn, uint64_t seed, uint64_t offset,
                                      const long long *epoch_dev, uint64_t epoch_stride, const float *scales, int lds, float *out, int ldo,
                                      float *lik, int ldl, size_t npix, int C, int mode, float scale_bound, float lik_bound, void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(mode == 0 || mode == 1, "stem_gc_scale_forward: mode %d is neither 0 (noise) nor 1 (round)", mode);
    STEM_CHECK_ARG(C > 0, "stem_gc_scale_forward: C = %d", C);
    STEM_CHECK_ARG(y && scales && out && lik, "stem_gc_scale_forward: null pointer");
    if (mode != 0) noise = nullptr;
    STEM_CHECK_ARG(ldy >= C && lds >= C && ldo >= C && ldl >= C && pitch_ok(noise, ldn, C),
                   "stem_gc_scale_forward: a pixel pitch (%d %d %d %d %d) is smaller than C = %d", ldy, ldn, lds, ldo, ldl, C);
    const size_t n = npix * (size_t)C;
    const Pitches p{C, ldy == C && lds == C && ldo == C && ldl == C && is_dense(noise, ldn, C)};
    const NoiseSrc nl{noise, seed, offset, epoch_stride, epoch_dev};
    const bool vec = C % 4 == 0 && vec_ok(y, ldy) && vec_ok(noise, ldn) && vec_ok(scales, lds) && vec_ok(out, ldo) && vec_ok(lik, ldl);
    const size_t nthreads = vec ? n / 4 : n;
    STEM_CHECK_ARG(cdivz(nthreads, 256) <= 0x7FFFFFFFu, "stem_gc_scale_forward: %zu elements exceed one grid", n);
    hipLaunchKernelGGL(vec ? gc_scale_forward_kernel<true> : gc_scale_forward_kernel<false>, dim3((unsigned)cdivz(nthreads, 256)), dim3(256),
                       0, (hipStream_t)stream, y, ldy, nl, ldn, scales, lds, out, ldo, lik, ldl, n, p, mode, scale_bound, lik_bound);
    STEM_LAUNCH_CHECK("gc_scale_forward");
    return 0;
}

STEM_EXPORT int stem_gc_scale_backward(const float *out, int ldo, const float *scales, int lds, const float *dlik, int ldl, const float *dout,
                                       int ldg, float *dscales, int ldds, float *dy, int lddy, size_t npix, int C, float scale_bound,
                                       float lik_bound, float *q, void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(C > 0, "stem_gc_scale_backward: C = %d", C);
    STEM_CHECK_ARG(out && scales && dlik, "stem_gc_scale_backward: null pointer");
    STEM_CHECK_ARG(dy || !dout, "stem_gc_scale_backward: dout without dy");
    STEM_CHECK_ARG(ldo >= C && lds >= C && ldl >= C && pitch_ok(dout, ldg, C) && pitch_ok(dscales, ldds, C) && pitch_ok(dy, lddy, C),
                   "stem_gc_scale_backward: a pixel pitch (%d %d %d %d %d %d) is smaller than C = %d", ldo, lds, ldl, ldg, ldds, lddy, C);
    const size_t n = npix * (size_t)C;
    const Pitches p{C, ldo == C && lds == C && ldl == C && is_dense(dout, ldg, C) && is_dense(dscales, ldds, C) && is_dense(dy, lddy, C)};
    const bool vec = C % 4 == 0 && vec_ok(out, ldo) && vec_ok(scales, lds) && vec_ok(dlik, ldl) && vec_ok(dout, ldg) && vec_ok(dscales, ldds) &&
                     vec_ok(dy, lddy);
    const size_t nthreads = vec ? n / 4 : n;
    STEM_CHECK_ARG(cdivz(n, 256) <= 0x7FFFFFFFu, "stem_gc_scale_backward: %zu elements exceed one grid", n);
    hipLaunchKernelGGL(vec ? gc_scale_backward_kernel<true> : gc_scale_backward_kernel<false>, dim3((unsigned)cdivz(nthreads, 256)), dim3(256),
                       0, (hipStream_t)stream, out, ldo, scales, lds, dlik, ldl, dout, ldg, dscales, ldds, dy, lddy, n, p, scale_bound,
                       lik_bound, q);
    STEM_LAUNCH_CHECK("gc_scale_backward");
    return 0;
}

static int abs_launch(const char *who, const float *x, int ldx, const float *g, int ldg, float *out, int ldo, size_t npix, int C, void *stream)
{
    const size_t n = npix * (size_t)C;
    const Pitches p{C, ldx == C && ldo == C && is_dense(g, ldg, C)};
    const bool vec = C % 4 == 0 && vec_ok(x, ldx) && vec_ok(g, ldg) && vec_ok(out, ldo);
    const size_t nb = cdivz(vec ? n / 4 : n, 256);
    hipLaunchKernelGGL(vec ? abs_kernel<true> : abs_kernel<false>, dim3((unsigned)(nb < ABS_MAX_BLOCKS ? nb : ABS_MAX_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, x, ldx, g, ldg, out, ldo, n, p);
    STEM_LAUNCH_CHECK(who);
    return 0;
}

STEM_EXPORT int stem_abs_fwd(const float *x, int ldx, float *out, int ldo, size_t npix, int C, void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(C > 0, "stem_abs_fwd: C = %d", C);
    STEM_CHECK_ARG(x && out, "stem_abs_fwd: null pointer");
    STEM_CHECK_ARG(ldx >= C && ldo >= C, "stem_abs_fwd: a pixel pitch (%d %d) is smaller than C = %d", ldx, ldo, C);
    return abs_launch("abs_fwd", x, ldx, nullptr, 0, out, ldo, npix, C, stream);
}

STEM_EXPORT int stem_abs_bwd(const float *x, int ldx, const float *g, int ldg, float *dx, int lddx, size_t npix, int C, void *stream)
{
    if (npix == 0) return 0;
    STEM_CHECK_ARG(C > 0, "stem_abs_bwd: C = %d", C);
    STEM_CHECK_ARG(x && g && dx, "stem_abs_bwd: null pointer");
    STEM_CHECK_ARG(ldx >= C && ldg >= C && lddx >= C, "stem_abs_bwd: a pixel pitch (%d %d %d) is smaller than C = %d", ldx, ldg, lddx, C);
    return abs_launch("abs_bwd", x, ldx, g, ldg, dx, lddx, npix, C, stream);
}
