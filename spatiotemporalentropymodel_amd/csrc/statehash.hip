// The conditioning-state hash of the sequence codecs (include/stem_statehash.h; libstem_statehash.so; video.py, video_pixel.py):
//     stem_state_hash   x fp32 [B][C][H][W], channels-last or planar, dense or pitched -> 64 bits per image   one or two launches
//
// out[b] = sum of mix64((i << 32) | bits(x[b,c,h,w])) mod 2^64 with i the LOGICAL NCHW index: the header states the definition.
//
// Walk.  A tensor is read in MEMORY order along its unit-stride dimension (`inner`: the channels of a channels-last tensor, the
// columns of a planar one) and the two dimensions around it (`o1` rows apart s1, `o2` apart s2): position p = (a * o2 + b) * inner + l
// sits at a * s1 + b * s2 + l.  A workgroup of 256 threads owns STEM_STATE_HASH_CHUNK consecutive positions of one image; with VEC a
// thread reads four consecutive positions as one 16-byte load (inner a multiple of 4, so the four never leave a row; pitches
// multiples of 4 and a 16-byte aligned base, so the load is aligned), 256 threads side by side, four times; without it one float at
// a time, sixteen times.  A planar position IS the logical index; a channels-last one is turned into it ((l * H + a) * W + b).  All
// of p, l, a, b and i fit 32 bits unsigned (C * H * W <= 2^32), so the two divisions per load are 32-bit ones.
//
// Sum.  Every thread adds its terms in a register, a wavefront folds its 64 sums by lane exchanges, the four wavefronts meet in LDS,
// thread 0 stores the workgroup's partial -- to out[b] itself when the image is one chunk, otherwise to workspace[b][chunk], which a
// second launch (one workgroup per image) adds up the same way.  Integer addition commutes, so neither the order inside a workgroup
// nor the order of the workgroups can move a bit; plain stores only: nothing to zero, no read-modify-write on memory, and a word the
// second launch reads has always been written by the first (a poisoned workspace comes back clean).
// Cost: two 64-bit multiplies (a few 32-bit ones each) per element and two 32-bit divisions per load against 4 bytes of HBM traffic
// per element; the pass is launch- and bandwidth-bound at the codec's shapes (profiles/state_hash.json).
#include <stdarg.h>

#include "../../include/stem_statehash.h"
#include "stem_common.h"

// this library's own message slot
static thread_local char g_err[512] = "";
void stem_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
STEM_EXPORT const char *stem_statehash_last_error(void) { return g_err; }

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_CHUNK = STEM_STATE_HASH_CHUNK;
static_assert(SH_CHUNK % (4 * SH_THREADS) == 0, "a chunk is a whole number of 16-byte loads per thread");

typedef unsigned long long u64;

__device__ inline u64 mix64(u64 z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ inline u64 term(unsigned i, float v) { return mix64(((u64)i << 32) | (u64)__float_as_uint(v)); }

// the sum over the workgroup (SH_THREADS threads), valid in thread 0
__device__ inline u64 block_sum(u64 v)
{
    __shared__ u64 red[SH_THREADS / 64];
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v += ((u64)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = red[0];
#pragma unroll
    for (int w = 1; w < SH_THREADS / 64; ++w) s += red[w];
    return s;
}

// CL: channels-last (inner = C, o1 = H, o2 = W); otherwise planar (inner = W, o1 = C, o2 = H).  n = C * H * W.
// dst[b * dst_pitch + blockIdx.x] receives the workgroup's sum.
template <bool CL, bool VEC>
__global__ __launch_bounds__(SH_THREADS) void state_hash_kernel(const float *__restrict__ x, u64 n, unsigned inner, unsigned o2, unsigned H,
                                                                unsigned W, size_t sb, size_t s1, size_t s2, u64 *__restrict__ dst,
                                                                size_t dst_pitch)
{
    const float *img = x + (size_t)blockIdx.y * sb;
    const u64 p0 = (u64)blockIdx.x * SH_CHUNK;
    u64 acc = 0;
    constexpr int PER = VEC ? 4 : 1;
#pragma unroll 4
    for (int k = 0; k < SH_CHUNK / (SH_THREADS * PER); ++k) {
        const u64 p64 = p0 + ((u64)k * SH_THREADS + threadIdx.x) * PER;
        if (p64 >= n) break;                                       // positions grow with k: nothing further is live either
        const unsigned p = (unsigned)p64;                          // n <= 2^32
        const unsigned q = p / inner, l = p - q * inner;
        const unsigned a = q / o2, b = q - a * o2;
        const float *src = img + (size_t)a * s1 + (size_t)b * s2 + l;
        if (VEC) {                                                 // inner % 4 == 0: l .. l + 3 are in this row, and all four are < n
            const f32x4 v = *reinterpret_cast<const f32x4 *>(src);
            if (CL) {
                const unsigned i = (l * H + a) * W + b, step = H * W;
                acc += term(i, v.x) + term(i + step, v.y) + term(i + 2 * step, v.z) + term(i + 3 * step, v.w);
            } else {
                acc += term(p, v.x) + term(p + 1, v.y) + term(p + 2, v.z) + term(p + 3, v.w);
            }
        } else {
            acc += term(CL ? (l * H + a) * W + b : p, *src);
        }
    }
    const u64 s = block_sum(acc);
    if (threadIdx.x == 0) dst[(size_t)blockIdx.y * dst_pitch + blockIdx.x] = s;
}

// one workgroup per image: out[b] = the sum of its nblk partials
__global__ __launch_bounds__(SH_THREADS) void state_hash_final_kernel(const u64 *__restrict__ part, unsigned nblk, u64 *__restrict__ out)
{
    const u64 *mine = part + (size_t)blockIdx.x * nblk;
    u64 acc = 0;
    for (unsigned j = threadIdx.x; j < nblk; j += SH_THREADS) acc += mine[j];
    const u64 s = block_sum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the element count of one image, or 0 when the geometry is refused
inline u64 image_elements(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    const u64 ch = (u64)C * (u64)H;                                // < 2^62
    if (ch > (1ull << 32)) return 0;
    const u64 n = ch * (u64)W;                                     // <= 2^32 * 2^31
    return n > (1ull << 32) ? 0 : n;
}

}   // namespace

STEM_EXPORT size_t stem_state_hash_workspace_bytes(int B, int C, int H, int W)
{
    const u64 n = image_elements(B, C, H, W);
    const u64 nblk = (n + SH_CHUNK - 1) / SH_CHUNK;
    return nblk <= 1 ? 0 : (size_t)B * (size_t)nblk * sizeof(uint64_t);
}

STEM_EXPORT int stem_state_hash(const float *x, int B, int C, int H, int W, size_t sb, size_t sc, size_t sh, size_t sw, uint64_t *out,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "stem_state_hash";
    STEM_CHECK_ARG(x && out, "%s: null pointer", who);
    STEM_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: a tensor of [%d, %d, %d, %d]", who, B, C, H, W);
    STEM_CHECK_ARG(B <= 65535, "%s: at most 65535 images a call, got %d", who, B);
    const u64 n = image_elements(B, C, H, W);
    STEM_CHECK_ARG(n, "%s: %d x %d x %d elements an image, the index has 32 bits", who, C, H, W);
    const size_t cap = (size_t)1 << 40;
    STEM_CHECK_ARG(sb < cap && sc < cap && sh < cap && sw < cap, "%s: strides (%zu, %zu, %zu, %zu): one of them is 2^40 or more", who, sb, sc, sh, sw);
    // the geometry in 128-bit integers: a stride below 2^40 times an extent below 2^31 does not fit 64 bits
    typedef unsigned __int128 u128;
    const u128 uC = (u128)C, uH = (u128)H, uW = (u128)W;
    const bool planar = sw == 1 && sh >= uW && sc >= (uH - 1) * sh + uW;
    const bool cl = !planar && sc == 1 && sw >= uC && sh >= (uW - 1) * sw + uC;
    STEM_CHECK_ARG(planar || cl, "%s: strides (%zu, %zu, %zu, %zu) of [%d, %d, %d, %d] are neither channels-last (sc == 1) nor planar (sw == 1) rows",
                   who, sb, sc, sh, sw, B, C, H, W);
    const u128 span = planar ? (uC - 1) * sc + (uH - 1) * sh + uW : (uH - 1) * sh + (uW - 1) * sw + uC;
    STEM_CHECK_ARG(span <= ((u128)1 << 48), "%s: strides (%zu, %zu, %zu, %zu): an image spans more than 2^48 floats", who, sb, sc, sh, sw);
    STEM_CHECK_ARG(B == 1 || sb >= span, "%s: images %zu floats apart overlap (one spans %zu)", who, sb, (size_t)span);
    STEM_CHECK_ARG(aligned_to(x, 4) && aligned_to(out, 8) && aligned_to(workspace, 8), "%s: misaligned pointer", who);
    const u64 nblk = (n + SH_CHUNK - 1) / SH_CHUNK;                // <= 2^20
    const size_t need = stem_state_hash_workspace_bytes(B, C, H, W);
    STEM_CHECK_ARG(need == 0 || workspace, "%s: null pointer (a workspace of %zu bytes is needed)", who, need);
    STEM_CHECK_ARG(workspace_bytes >= need, "%s: a workspace of %zu bytes, %zu are needed", who, workspace_bytes, need);

    const unsigned inner = planar ? (unsigned)W : (unsigned)C, o2 = planar ? (unsigned)H : (unsigned)W;
    const size_t s1 = planar ? sc : sh, s2 = planar ? sh : sw;
    const bool vec = inner % 4 == 0 && s1 % 4 == 0 && s2 % 4 == 0 && (B == 1 || sb % 4 == 0) && aligned_to(x, 16);
    u64 *dst = nblk == 1 ? reinterpret_cast<u64 *>(out) : static_cast<u64 *>(workspace);
    const size_t dst_pitch = (size_t)nblk;
    const dim3 grid((unsigned)nblk, (unsigned)B), block(SH_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define STEM_SH_LAUNCH(L, V)                                                                                                                   \
    hipLaunchKernelGGL((state_hash_kernel<L, V>), grid, block, 0, st, x, n, inner, o2, (unsigned)H, (unsigned)W, sb, s1, s2, dst, dst_pitch)
    if (cl && vec)
        STEM_SH_LAUNCH(true, true);
    else if (cl)
        STEM_SH_LAUNCH(true, false);
    else if (vec)
        STEM_SH_LAUNCH(false, true);
    else
        STEM_SH_LAUNCH(false, false);
#undef STEM_SH_LAUNCH
    STEM_LAUNCH_CHECK(who);
    if (nblk > 1) {
        hipLaunchKernelGGL(state_hash_final_kernel, dim3((unsigned)B), block, 0, st, static_cast<const u64 *>(workspace), (unsigned)nblk,
                           reinterpret_cast<u64 *>(out));
        STEM_LAUNCH_CHECK(who);
    }
    return 0;
}
