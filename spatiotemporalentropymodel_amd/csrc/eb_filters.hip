// EntropyBottleneck kernels for any `filters` tuple inside the caps of include/stem_eb_filters.h: the general siblings of
// entropy.hip's eb_* kernels, which hard-code the 1 -> 3 -> 3 -> 3 -> 3 -> 1 network.  Same arithmetic per element (softplus
// threshold 20, sigmoid, rintf, log1pf(expf())), same contracts.
//
// How the run-time widths stay out of private memory (no scratch in any kernel here):
//   * the transformed parameters (softplus of the matrices, biases, tanh of the factors) sit in LDS, written once per workgroup;
//   * activations are register arrays of the compile-time extent [MAXW], every loop over them is fully unrolled and guarded by
//     `o < width`; the layer loop is unrolled to the cap and guarded by `l <= L`.  The guards are uniform over a workgroup;
//   * the network's shape travels as a kernel argument (EbfNet) that is only ever indexed with compile-time constants.
#include "stem_common.h"
#include "../../include/stem_eb_filters.h"

namespace {

constexpr int MAXF = STEM_EBF_MAX_FILTERS;      // gated layers at most; MAXF + 1 layers
constexpr int MAXW = STEM_EBF_MAX_WIDTH;
constexpr int MAXNP = STEM_EBF_MAX_NPARAM;
constexpr int MAXSEG = 3 * MAXF + 2;            // parameter tensors at most

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// the network's shape: layer l maps w[l] -> w[l + 1] and starts at float off[l] of a channel's pack
struct EbfNet {
    int L, np;
    int w[MAXF + 2];
    int off[MAXF + 1];
};

// 0 = matrix (softplus), 1 = bias (as it is), 2 = factor (tanh) for float k of a channel's pack
__device__ __forceinline__ int ebf_role(const EbfNet &net, int k)
{
    int role = 1;
#pragma unroll
    for (int l = 0; l <= MAXF; ++l) {
        if (l <= net.L) {
            const int mm = net.w[l + 1] * net.w[l], r = k - net.off[l];
            if (r >= 0) role = r < mm ? 0 : (r < mm + net.w[l + 1] ? 1 : 2);
        }
    }
    return role;
}
__device__ __forceinline__ float ebf_transform(int role, float pv) { return role == 0 ? softplus_f(pv) : (role == 1 ? pv : tanhf(pv)); }

// net.w[t], net.w[t + 1], net.off[t] for a run-time t, without indexing the argument with it
struct EbfLayer {
    int wi, wo, off;
};
__device__ __forceinline__ EbfLayer ebf_layer(const EbfNet &net, int t)
{
    EbfLayer r = {1, 1, 0};
#pragma unroll
    for (int l = 0; l <= MAXF; ++l) {
        if (l == t) {
            r.wi = net.w[l];
            r.wo = net.w[l + 1];
            r.off = net.off[l];
        }
    }
    return r;
}

// _logits_cumulative (entropy_models.py:388-407) of N values at once (the parameters are read from LDS once for all of them).
// e: this thread's channel in the transformed parameters, float k at e[k * S].  KEEP: ta[n][l][o] = tanh of layer l's value in front
// of its gate, in_t[n][k] = the input of layer t: what the reverse pass needs.
template <int S, int N, bool KEEP>
__device__ __forceinline__ void ebf_logits(const EbfNet &net, const float *e, const float (&v)[N], float (&out)[N],
                                           float (&ta)[N][MAXF][MAXW], float (&in_t)[N][MAXW], int t)
{
    float h[N][MAXW];
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int k = 0; k < MAXW; ++k) h[n][k] = k == 0 ? v[n] : 0.f;
    }
#pragma unroll
    for (int l = 0; l <= MAXF; ++l) {
        if (l <= net.L) {
            const int wi = net.w[l], wo = net.w[l + 1];
            const float *m = e + net.off[l] * S;
            if (KEEP && l == t) {
#pragma unroll
                for (int n = 0; n < N; ++n) {
#pragma unroll
                    for (int k = 0; k < MAXW; ++k) in_t[n][k] = h[n][k];
                }
            }
            float g[N][MAXW];
#pragma unroll
            for (int o = 0; o < MAXW; ++o) {
#pragma unroll
                for (int n = 0; n < N; ++n) g[n][o] = 0.f;
                if (o < wo) {
                    float a[N];
                    const float b = m[(wo * wi + o) * S];
#pragma unroll
                    for (int n = 0; n < N; ++n) a[n] = b;
#pragma unroll
                    for (int k = 0; k < MAXW; ++k) {
                        if (k < wi) {
                            const float sp = m[(o * wi + k) * S];
#pragma unroll
                            for (int n = 0; n < N; ++n) a[n] += sp * h[n][k];
                        }
                    }
                    if (l < MAXF && l < net.L) {
                        const float tf = m[(wo * wi + wo + o) * S];
#pragma unroll
                        for (int n = 0; n < N; ++n) {
                            const float th = tanhf(a[n]);
                            if (KEEP) ta[n][l < MAXF ? l : 0][o] = th;
                            a[n] += tf * th;
                        }
                    }
#pragma unroll
                    for (int n = 0; n < N; ++n) g[n][o] = a[n];
                }
            }
#pragma unroll
            for (int n = 0; n < N; ++n) {
#pragma unroll
                for (int o = 0; o < MAXW; ++o) h[n][o] = g[n][o];
            }
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) out[n] = h[n][0];
}

// accumulator slots of one layer's gradients: matrix entry (o, k) at o * MAXW + k, bias o at ACC_B + o, factor o at ACC_F + o
constexpr int ACC_B = MAXW * MAXW, ACC_F = ACC_B + MAXW, ACC_N = ACC_F + MAXW;

// The reverse pass from the top layer down to layer t: gl[n] = d / d logits of value n.  PARAMS: layer t's gradients are added to
// acc -- with respect to softplus(matrix), the bias and tanh(factor): the derivatives of the two transforms do not depend on the
// pixel and are applied once, after the sum over pixels.  gv[n] = d / d v[n], computed when t == 0.
template <int S, int N, bool PARAMS>
__device__ __forceinline__ void ebf_logits_bwd(const EbfNet &net, const float *e, const float (&gl)[N],
                                               const float (&ta)[N][MAXF][MAXW], const float (&in_t)[N][MAXW], int t,
                                               float (&acc)[ACC_N], float (&gv)[N])
{
    float gh[N][MAXW];
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int k = 0; k < MAXW; ++k) gh[n][k] = k == 0 ? gl[n] : 0.f;
    }
#pragma unroll
    for (int l = MAXF; l >= 0; --l) {
        if (l <= net.L && l >= t) {
            const int wi = net.w[l], wo = net.w[l + 1];
            const float *m = e + net.off[l] * S;
            float ga[N][MAXW];
#pragma unroll
            for (int o = 0; o < MAXW; ++o) {
#pragma unroll
                for (int n = 0; n < N; ++n) ga[n][o] = 0.f;
                if (o < wo) {
                    if (l < MAXF && l < net.L) {
                        const float tf = m[(wo * wi + wo + o) * S];
#pragma unroll
                        for (int n = 0; n < N; ++n) {
                            const float th = ta[n][l < MAXF ? l : 0][o];
                            if (PARAMS && l == t) acc[ACC_F + o] += gh[n][o] * th;
                            ga[n][o] = gh[n][o] * (1.f + tf * (1.f - th * th));
                        }
                    } else {
#pragma unroll
                        for (int n = 0; n < N; ++n) ga[n][o] = gh[n][o];
                    }
                    if (PARAMS && l == t) {
#pragma unroll
                        for (int n = 0; n < N; ++n) {
                            acc[ACC_B + o] += ga[n][o];
#pragma unroll
                            for (int k = 0; k < MAXW; ++k) {
                                if (k < wi) acc[o * MAXW + k] += ga[n][o] * in_t[n][k];
                            }
                        }
                    }
                }
            }
            if (l > t || t == 0) {
                float gin[N][MAXW];
#pragma unroll
                for (int k = 0; k < MAXW; ++k) {
#pragma unroll
                    for (int n = 0; n < N; ++n) gin[n][k] = 0.f;
                    if (k < wi) {
#pragma unroll
                        for (int o = 0; o < MAXW; ++o) {
                            if (o < wo) {
                                const float sp = m[(o * wi + k) * S];
#pragma unroll
                                for (int n = 0; n < N; ++n) gin[n][k] += ga[n][o] * sp;
                            }
                        }
                    }
                }
#pragma unroll
                for (int n = 0; n < N; ++n) {
#pragma unroll
                    for (int k = 0; k < MAXW; ++k) gh[n][k] = gin[n][k];
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) gv[n] = gh[n][0];
}

// the likelihood from the two logits (entropy_models.py:410-421), as entropy.hip's eb_tail
struct EbfTail {
    float su, sl, sg, diff;
};
__device__ __forceinline__ EbfTail ebf_tail(float lo, float up)
{
    EbfTail t;
    const float s = lo + up;
    t.sg = s > 0.f ? -1.f : (s < 0.f ? 1.f : 0.f);
    t.su = sigmoid_f(t.sg * up);
    t.sl = sigmoid_f(t.sg * lo);
    t.diff = t.su - t.sl;
    return t;
}

// ---- forward: a workgroup owns FWD_CT consecutive channels and a run of pixels.  Lanes 0 .. 15 of every 16 are consecutive
// channels, so a wavefront touches 4 pixels x 64 contiguous bytes of the NHWC tensors; the 16 channels' transformed parameters are
// in LDS with the channel fastest (float k of channel cl at prep[k * FWD_CT + cl]: 16 consecutive banks, no conflict).  Serves both
// regimes: few pixels per channel (the host picks short runs, many workgroups) and the y of a factorized prior.
constexpr int FWD_CT = 16, FWD_NT = 256, FWD_PL = FWD_NT / FWD_CT;
__global__ __launch_bounds__(FWD_NT) void ebf_forward_kernel(EbfNet net, const float *z, int ldz, const float *noise,
                                                             const float *pack, const float *med, float *zhat, float *lik,
                                                             size_t npix, int C, int mode, float bound, int ppb)
{
    __shared__ float prep[MAXNP * FWD_CT];
    const int c0 = blockIdx.x * FWD_CT;
    for (int i = threadIdx.x; i < net.np * FWD_CT; i += FWD_NT) {
        const int k = i / FWD_CT, ch = c0 + (i - k * FWD_CT);
        if (ch < C) prep[i] = ebf_transform(ebf_role(net, k), pack[(size_t)ch * net.np + k]);
    }
    __syncthreads();
    const int cl = threadIdx.x % FWD_CT, c = c0 + cl;
    if (c >= C) return;
    const float *e = prep + cl;
    const size_t p0 = (size_t)blockIdx.y * ppb, p1 = p0 + ppb < npix ? p0 + ppb : npix;
    const float m = mode ? med[c] : 0.f;
    for (size_t pix = p0 + threadIdx.x / FWD_CT; pix < p1; pix += FWD_PL) {
        const size_t i = pix * C + c;
        float v = z[pix * ldz + c];
        if (mode == 0)
            v += noise[i];
        else
            v = rintf(v - m) + m;
        zhat[i] = v;
        const float vv[2] = {v - 0.5f, v + 0.5f};
        float lu[2], ta[2][MAXF][MAXW], in_t[2][MAXW];
        ebf_logits<FWD_CT, 2, false>(net, e, vv, lu, ta, in_t, 0);
        lik[i] = fmaxf(fabsf(ebf_tail(lu[0], lu[1]).diff), bound);
    }
}

// ---- backward: one workgroup per channel.  A thread cannot hold a whole network's gradients (up to 433), so the kernel makes one
// pass over the channel's pixels per layer t: the forward is recomputed, the reverse pass runs from the top down to layer t, and
// only layer t's gradients (at most 8 x 8 + 2 x 8) are accumulated.  Pass 0 reaches the input and writes dz.  O(L^2) arithmetic
// per element, no workspace.  Sums over pixels: per thread in pixel order, wavefront shuffles, then the wavefronts' partials in
// wavefront order through LDS -- no atomics, the same bits every launch.  PARAMS = false (dpack not wanted): pass 0 only.
constexpr int BWD_NT = 256;
template <bool PARAMS>
__global__ __launch_bounds__(BWD_NT) void ebf_backward_kernel(EbfNet net, const float *zhat, const float *pack, const float *dlik,
                                                              const float *dzin, float *dz, float *dpack, size_t npix, int C,
                                                              float bound)
{
    __shared__ float prep[MAXNP];
    __shared__ float red[BWD_NT / 64][ACC_N];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *p = pack + (size_t)c * net.np;
    for (int k = threadIdx.x; k < net.np; k += BWD_NT) prep[k] = ebf_transform(ebf_role(net, k), p[k]);
    __syncthreads();
    const int npass = PARAMS ? net.L + 1 : 1;
#pragma unroll 1
    for (int t = 0; t < npass; ++t) {
        float acc[ACC_N];
#pragma unroll
        for (int s = 0; s < ACC_N; ++s) acc[s] = 0.f;
        for (size_t pix = threadIdx.x; pix < npix; pix += BWD_NT) {
            const size_t i = pix * C + c;
            const float v = zhat[i];
            const float vv[2] = {v - 0.5f, v + 0.5f};
            float lu[2], ta[2][MAXF][MAXW], in_t[2][MAXW];
            ebf_logits<1, 2, true>(net, prep, vv, lu, ta, in_t, t);
            const auto [su, sl, sg, diff] = ebf_tail(lu[0], lu[1]);
            float g = dlik[i];
            if (!(fabsf(diff) >= bound || g < 0.f)) g = 0.f;     // LowerBound rule (bound_ops.py:28-31)
            const float gd = g * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));
            const float gl[2] = {-gd * sl * (1.f - sl) * sg, gd * su * (1.f - su) * sg};
            float gv[2];
            ebf_logits_bwd<1, 2, PARAMS>(net, prep, gl, ta, in_t, t, acc, gv);
            if (t == 0 && dz) dz[i] = (gv[1] + gv[0]) + (dzin ? dzin[i] : 0.f);
        }
        if (PARAMS) {
            const EbfLayer ly = ebf_layer(net, t);
            const bool gated = t < net.L;
#pragma unroll
            for (int s = 0; s < ACC_N; ++s) {
                const int o = s < ACC_B ? s / MAXW : (s - ACC_B) % MAXW, k = s < ACC_B ? s % MAXW : 0;
                if (o < ly.wo && k < ly.wi && (s < ACC_F || gated)) {
                    float x = acc[s];
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
                    if (lane == 0) red[wave][s] = x;
                }
            }
            __syncthreads();
            const int mm = ly.wo * ly.wi, nt = mm + ly.wo + (gated ? ly.wo : 0), j = threadIdx.x;
            if (j < nt) {
                const int slot = j < mm ? (j / ly.wi) * MAXW + j % ly.wi : (j < mm + ly.wo ? ACC_B + (j - mm) : ACC_F + (j - mm - ly.wo));
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < BWD_NT / 64; ++w) s += red[w][slot];
                // d softplus(x) / dx = sigmoid(x);  d tanh(x) / dx = 1 - tanh(x)^2
                const float tr = prep[ly.off + j];
                const float d = j < mm ? sigmoid_f(p[ly.off + j]) : (j < mm + ly.wo ? 1.f : 1.f - tr * tr);
                dpack[(size_t)c * net.np + ly.off + j] = s * d;
            }
            __syncthreads();
        }
    }
}

// ---- EntropyBottleneck.loss with its quantile gradient: one workgroup (the loss is one fixed-order sum, written), which walks the
// channels AUX_CT at a time -- the transformed parameters of a chunk in LDS (channel fastest), one (channel, quantile) item per
// thread of the first 3 AUX_CT, the forward keeping the gates' tanh values and the reverse pass walking the input-gradient chain
// only.  The LDS does not depend on C.
constexpr int AUX_CT = 32, AUX_NT = 256;
__global__ __launch_bounds__(AUX_NT) void ebf_aux_kernel(EbfNet net, const float *quant, const float *pack, const float *target,
                                                         float *loss, float *dq, int C, int accumulate)
{
    __shared__ float prep[MAXNP * AUX_CT];
    __shared__ float red[AUX_NT];
    float slot = 0.f;                      // this thread's items in channel order
    for (int c0 = 0; c0 < C; c0 += AUX_CT) {
        __syncthreads();
        for (int i = threadIdx.x; i < net.np * AUX_CT; i += AUX_NT) {
            const int k = i / AUX_CT, ch = c0 + (i - k * AUX_CT);
            if (ch < C) prep[i] = ebf_transform(ebf_role(net, k), pack[(size_t)ch * net.np + k]);
        }
        __syncthreads();
        const int cl = threadIdx.x / 3, q = threadIdx.x - cl * 3, c = c0 + cl;
        if (cl < AUX_CT && c < C) {
            const int i = c * 3 + q;
            const float v[1] = {quant[i]};
            float out[1], ta[1][MAXF][MAXW], in_t[1][MAXW], acc[ACC_N], gv[1];
            ebf_logits<AUX_CT, 1, true>(net, prep + cl, v, out, ta, in_t, -1);
            const float d = out[0] - target[q];
            slot += fabsf(d);
            const float gl[1] = {d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)};
            ebf_logits_bwd<AUX_CT, 1, false>(net, prep + cl, gl, ta, in_t, 0, acc, gv);
            if (dq) dq[i] = accumulate ? dq[i] + gv[0] : gv[0];
        }
    }
    red[threadIdx.x] = slot;
    __syncthreads();
    for (int s = AUX_NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = red[0];
}

// ---- pack / unpack: the 3 L + 2 tensors <-> [C][nparam]
struct EbfSegs {
    float *p[MAXSEG];
    int off[MAXSEG], len[MAXSEG];
    int nseg, np;
};
template <bool UNPACK>
__global__ __launch_bounds__(256) void ebf_pack_kernel(EbfSegs t, float *pack, int C, int accumulate)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)C * t.np) return;
    const int c = (int)(i / t.np), k = (int)(i - (size_t)c * t.np);
    float *base = t.p[0];
    int off = 0, len = t.len[0];
#pragma unroll
    for (int q = 1; q < MAXSEG; ++q) {
        if (q < t.nseg && k >= t.off[q]) {
            base = t.p[q];
            off = t.off[q];
            len = t.len[q];
        }
    }
    float *x = base + (size_t)c * len + (k - off);
    if (UNPACK)
        *x = accumulate ? *x + pack[i] : pack[i];
    else
        pack[i] = *x;
}

// the shape of the network from the host's filters; false outside the caps
bool ebf_net(const int *filters, int n, EbfNet *net)
{
    if (n < 0 || n > MAXF || (n > 0 && !filters)) return false;
    net->L = n;
    for (int i = 0; i < MAXF + 2; ++i) net->w[i] = 1;
    for (int i = 0; i < n; ++i) {
        if (filters[i] < 1 || filters[i] > MAXW) return false;
        net->w[i + 1] = filters[i];
    }
    int off = 0;
    for (int l = 0; l <= MAXF; ++l) {
        net->off[l] = off;
        if (l <= n) off += net->w[l + 1] * net->w[l] + net->w[l + 1] * (l < n ? 2 : 1);
    }
    net->np = off;
    return off <= MAXNP;
}

int ebf_segs(const EbfNet &net, float *const *tensors, EbfSegs *s)
{
    int q = 0;
    for (int l = 0; l <= net.L; ++l) {
        const int wo = net.w[l + 1], mm = wo * net.w[l];
        const int lens[3] = {mm, wo, wo}, offs[3] = {0, mm, mm + wo};
        for (int r = 0; r < (l < net.L ? 3 : 2); ++r, ++q) {
            if (!tensors[q]) return -1;
            s->p[q] = tensors[q];
            s->off[q] = net.off[l] + offs[r];
            s->len[q] = lens[r];
        }
    }
    for (int r = q; r < MAXSEG; ++r) {
        s->p[r] = nullptr;
        s->off[r] = s->len[r] = 0;
    }
    s->nseg = q;
    s->np = net.np;
    return 0;
}

#define EBF_NET(name)                                                                                                     \
    EbfNet net;                                                                                                           \
    STEM_CHECK_ARG(ebf_net(filters, n_filters, &net),                                                                     \
                   name ": filters outside the caps (at most %d filters, widths 1 .. %d; n_filters = %d)", MAXF, MAXW, n_filters)

}   // namespace

STEM_EXPORT int stem_ebf_nparam(const int *filters, int n_filters)
{
    EbfNet net;
    return ebf_net(filters, n_filters, &net) ? net.np : -1;
}

STEM_EXPORT int stem_ebf_pack(const float *const *tensors, const int *filters, int n_filters, float *pack, int C, void *stream)
{
    EBF_NET("stem_ebf_pack");
    STEM_CHECK_ARG(tensors && pack && C > 0, "stem_ebf_pack: bad arguments");
    EbfSegs s;
    STEM_CHECK_ARG(ebf_segs(net, const_cast<float *const *>(tensors), &s) == 0, "stem_ebf_pack: null tensor pointer");
    const size_t n = (size_t)C * net.np;
    hipLaunchKernelGGL(ebf_pack_kernel<false>, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)stream, s, pack, C, 0);
    STEM_LAUNCH_CHECK("ebf_pack");
    return 0;
}

STEM_EXPORT int stem_ebf_unpack_grads(const float *dpack, float *const *tensors, const int *filters, int n_filters, int C,
                                      int accumulate, void *stream)
{
    EBF_NET("stem_ebf_unpack_grads");
    STEM_CHECK_ARG(tensors && dpack && C > 0, "stem_ebf_unpack_grads: bad arguments");
    EbfSegs s;
    STEM_CHECK_ARG(ebf_segs(net, tensors, &s) == 0, "stem_ebf_unpack_grads: null tensor pointer");
    const size_t n = (size_t)C * net.np;
    hipLaunchKernelGGL(ebf_pack_kernel<true>, dim3((unsigned)cdivz(n, 256)), dim3(256), 0, (hipStream_t)stream, s,
                       const_cast<float *>(dpack), C, accumulate);
    STEM_LAUNCH_CHECK("ebf_unpack");
    return 0;
}

STEM_EXPORT int stem_ebf_forward(const float *z, int ldz, const float *noise, const float *pack, const float *medians,
                                 const int *filters, int n_filters, float *z_hat, float *lik, int B, int H, int W, int C, int mode,
                                 float bound, void *stream)
{
    EBF_NET("stem_ebf_forward");
    STEM_CHECK_ARG(z && pack && z_hat && lik, "stem_ebf_forward: null pointer");
    STEM_CHECK_ARG(C > 0 && B >= 0 && H >= 0 && W >= 0 && ldz >= C, "stem_ebf_forward: bad shape (B=%d H=%d W=%d C=%d ldz=%d)", B, H, W, C, ldz);
    STEM_CHECK_ARG((mode == 0 && noise) || (mode == 1 && medians), "stem_ebf_forward: mode %d needs %s", mode, mode ? "medians" : "noise");
    const size_t npix = (size_t)B * H * W;
    if (npix == 0) return 0;
    // runs of pixels per workgroup: a multiple of the workgroup's 16 pixel lanes, short enough for ~1024 workgroups where the tensor
    // has that many runs, and long enough that the grid's second dimension stays legal
    const size_t nct = cdivz((size_t)C, FWD_CT);
    size_t chunks = 1024 / nct ? 1024 / nct : 1;
    size_t ppb = cdivz(cdivz(npix, chunks), FWD_PL) * FWD_PL;
    while (cdivz(npix, ppb) > 65535) ppb *= 2;
    STEM_CHECK_ARG(ppb <= (size_t)1 << 30, "stem_ebf_forward: too many pixels");
    hipLaunchKernelGGL(ebf_forward_kernel, dim3((unsigned)nct, (unsigned)cdivz(npix, ppb)), dim3(FWD_NT), 0, (hipStream_t)stream, net,
                       z, ldz, noise, pack, medians, z_hat, lik, npix, C, mode, bound, (int)ppb);
    STEM_LAUNCH_CHECK("ebf_forward");
    return 0;
}

STEM_EXPORT int stem_ebf_backward(const float *z_hat, const float *pack, const float *dlik, const float *dzhat_in,
                                  const int *filters, int n_filters, float *dz, float *dpack, int B, int H, int W, int C,
                                  float bound, void *stream)
{
    EBF_NET("stem_ebf_backward");
    STEM_CHECK_ARG(z_hat && pack && dlik, "stem_ebf_backward: null pointer");
    STEM_CHECK_ARG(C > 0 && B >= 0 && H >= 0 && W >= 0, "stem_ebf_backward: bad shape (B=%d H=%d W=%d C=%d)", B, H, W, C);
    if (!dz && !dpack) return 0;
    const size_t npix = (size_t)B * H * W;
    if (dpack)
        hipLaunchKernelGGL(ebf_backward_kernel<true>, dim3(C), dim3(BWD_NT), 0, (hipStream_t)stream, net, z_hat, pack, dlik, dzhat_in,
                           dz, dpack, npix, C, bound);
    else
        hipLaunchKernelGGL(ebf_backward_kernel<false>, dim3(C), dim3(BWD_NT), 0, (hipStream_t)stream, net, z_hat, pack, dlik, dzhat_in,
                           dz, dpack, npix, C, bound);
    STEM_LAUNCH_CHECK("ebf_backward");
    return 0;
}

STEM_EXPORT int stem_ebf_aux_loss_grad(const float *quantiles, const float *pack, const float *target3, const int *filters,
                                       int n_filters, float *loss, float *dquantiles, int C, int accumulate, void *stream)
{
    EBF_NET("stem_ebf_aux_loss_grad");
    STEM_CHECK_ARG(quantiles && pack && target3 && loss, "stem_ebf_aux_loss_grad: null pointer");
    STEM_CHECK_ARG(C > 0, "stem_ebf_aux_loss_grad: C = %d", C);
    hipLaunchKernelGGL(ebf_aux_kernel, dim3(1), dim3(AUX_NT), 0, (hipStream_t)stream, net, quantiles, pack, target3, loss, dquantiles,
                       C, accumulate);
    STEM_LAUNCH_CHECK("ebf_aux");
    return 0;
}
