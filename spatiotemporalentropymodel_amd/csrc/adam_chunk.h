// The clip + Adam update of one chunk of STEM_ADAM_CHUNK parameters by one workgroup of 256 threads, with the chunk's four wavefront
// maxima: stated once for adam_bmax_kernel (optim.hip, libstem_hip.so) and adam_bmax_ranges_kernel (tail.hip, libstem_tail.so), so that
// both compile from one text and leave the same bits.
#pragma once
#include "stem_common.h"

namespace {

// One workgroup of 256 threads over chunk `chunk` (elements chunk * STEM_ADAM_CHUNK ..., the last one ragged): the element update and
// the maxima are stated here once, for adam_bmax_kernel and adam_bmax_ranges_kernel.
__device__ __forceinline__ void adam_chunk_pass(float *p, float *g, float *m, float *v, size_t n, const double *sumsq, float max_norm,
                                                float gscale, float step_size, float b1, float b2, float inv_sqrt_bc2, float eps,
                                                int zero_g, float *bmax, unsigned chunk)
{
    float coef = gscale;
    if (max_norm > 0.f && sumsq) {
        const float total = (float)sqrt(sumsq[0]) * gscale;
        coef *= fminf(max_norm / (total + 1e-6f), 1.0f);
    }
    const size_t base = (size_t)chunk * STEM_ADAM_CHUNK;
    float mx = 0.f;
    // four elements per thread and pass, all sixteen loads issued before the first use (the pass is HBM-bound: 28 B per parameter)
#pragma unroll 1
    for (int k0 = 0; k0 < STEM_ADAM_CHUNK / 256; k0 += 4) {
        float gi[4], mi[4], vi[4], pi[4];
        size_t idx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            idx[u] = base + (size_t)(k0 + u) * 256 + threadIdx.x;
            const bool ok = idx[u] < n;
            const size_t j = ok ? idx[u] : 0;
            gi[u] = ok ? g[j] : 0.f;
            mi[u] = ok ? m[j] : 0.f;
            vi[u] = ok ? v[j] : 0.f;
            pi[u] = ok ? p[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (idx[u] >= n) continue;
            const float gs = gi[u] * coef;
            if (zero_g) g[idx[u]] = 0.f;
            const float mn = mi[u] + (gs - mi[u]) * (1.f - b1);
            const float vn = vi[u] * b2 + (1.f - b2) * gs * gs;
            m[idx[u]] = mn;
            v[idx[u]] = vn;
            const float pn = pi[u] - step_size * (mn / (sqrtf(vn) * inv_sqrt_bc2 + eps));
            p[idx[u]] = pn;
            mx = fmaxf(mx, fabsf(pn));
        }
    }
    mx = wave_max(mx);                                         // one slot per wavefront: no barrier in an HBM-bound pass
    if ((threadIdx.x & 63) == 0) bmax[chunk * 4 + (threadIdx.x >> 6)] = mx;
}

}   // namespace
