// The two data structures of the split-operand fp16 family (conv_f16x3 / conv_f16x3_img / wgrad_f16x3 / c4gdn_f16x3, written by
// f16x3_pack.hip and by the convolutions' epilogues), stated once.  The arithmetic -- two fp16 numbers per fp32 value, three MFMAs
// per fp32 product, a power-of-two scale per tensor in a scale record -- is described in stem_common.h ("the 16-bit operands").
//
// PLANES TENSOR (activations, gradients): per pixel and per 32-channel slab two consecutive rows of 32 fp16,
//     x_planes[pixel][slab][plane 0..1][32]        (SLAB = 128 B per pixel and slab = the fp32 bytes)
// addressed in 16-byte pieces of 8 channels (planes_piece); a buffer may be a 32-channel-aligned view of a wider tensor (bytes per
// pixel > nslab * SLAB).  Its scale record sits behind the payload, one slot per producing workgroup (planes_slots).
//
// PACKED WEIGHT IMAGE: per N tile and per K chunk q = slab * taps + tap (one tap x KC = 32 input channels) the exact LDS image the
// matrix kernels want, so that staging it is a straight copy:
//     w_image[N tile][chunk q][plane 0..1][rows][64 B]        row = output channel inside the tile, 64 B = 32 fp16
// with the 16-byte piece index of a row XOR-swizzled by (row >> 2) & 3 (wimg_piece): ds_read_b128 / ds_write_b128 of 64-byte rows
// are conflict-free without padding.  Rows beyond N are zero.  Two geometries:
//     gen image,  GBN = 128 rows per N tile, ceil(N / 128) tiles: conv_f16x3_gen_kernel, conv_f16x3_img_kernel, the four phase
//                 images of a transposed face (tconv_slot) one behind the other;
//     wide image, BN = 192 rows, one tile (N <= 192), all taps: conv_f16x3_kernel and its fused GDN's gamma'.
// The record behind an image (WQ_BYTES) sits behind the FULL image's size whatever prefix of the taps is packed.
#pragma once
#include "stem_common.h"

typedef hp8 h16x8;

constexpr int KC = 32;                                             // input channels per slab / K chunk
constexpr int NPL = 2, SLAB = NPL * 64;                            // planes per value; bytes per pixel and 32-channel slab
constexpr int MAXTAP = 25;                                         // taps of the largest window of the family (5 x 5)
constexpr int OOR = 0x7FFFFF00;                                    // voffset that every buffer view rejects (returns 0)

constexpr int GBN = 128;                                           // gen image: rows per N tile
constexpr int GB_PLANE = GBN * 64, GB_BUF = NPL * GB_PLANE;        // bytes of one plane of a chunk; 16384 per chunk
constexpr int BN = 192;                                            // wide image: rows
constexpr int B_PLANE = BN * 64, B_BUF = NPL * B_PLANE;            // 24576 per chunk

constexpr int WQ_SLOTS = 64;                                        // workgroups of the weights' max pass
constexpr size_t WQ_BYTES = (QREC_HDR + WQ_SLOTS) * sizeof(float);  // the record behind every packed weight image
static inline size_t planes_payload(long npix, int C) { return (size_t)npix * (C / 32) * SLAB; }
// one slot per producing workgroup: the smallest output tile of any producer is 64 pixels x 128 channels
static inline long planes_slots(long npix, int C) { return (long)cdivz((size_t)npix, 64) * cdiv(C, 128); }
static inline size_t w_image_bytes(int C, int R, int S) { return (size_t)(C / 32) * R * S * B_BUF; }
static inline size_t gen_image_bytes(int N, int C, int R, int S) { return (size_t)cdiv(N, GBN) * (C / 32) * R * S * GB_BUF; }

// ---- the transposed face of a stride-2 layer as four sub-pixel phases (forward of nn.ConvTranspose2d, input gradient of a strided
// nn.Conv2d: spatiotemporalpriors.py:814-829) ---------------------------------------------------------------------------------------
//   out[b, n, oy, ox] = sum over ch, r, s of in[b, ch, iy, ix] * w[ch][n][r][s]   with   oy = 2 iy - pad + r,  ox = 2 ix - pad + s
// An output pixel of parity (py, px) = (oy & 1, ox & 1) only meets the taps r = py + pad (mod 2), s = px + pad (mod 2): on the COARSE
// grid (qy, qx) = (oy >> 1, ox >> 1) phase (py, px) is a stride-1 convolution whose window holds those taps, tap r reading the
// coarse row qy + (py + pad - r) / 2.  Windows are kept in ascending offset order (descending r): position jy = (rmax - r) / 2.
// For 5 x 5, pad 2 the four windows are 3x3, 3x2, 2x3, 2x2 = all 25 taps once: no multiplication by structural zeros.
struct TAxis {
    int cnt, d0, rmax;             // taps of this parity, offset of the first (smallest offset), largest r
};
__host__ __device__ inline TAxis tconv_axis(int R, int pad, int par)
{
    TAxis t;
    const int rmin = (par + pad) & 1;
    t.cnt = rmin < R ? (R - 1 - rmin) / 2 + 1 : 0;
    t.rmax = rmin + 2 * (t.cnt - 1);
    t.d0 = (par + pad - t.rmax) / 2;               // even numerator: exact
    return t;
}
// position of tap (r, s) of the R x S window in the phase-ordered tap sequence [phase 0 | phase 1 | phase 2 | phase 3], phase = 2 py + px
__host__ __device__ inline int tconv_slot(int R, int S, int pad, int r, int s)
{
    const int py = (r + pad) & 1, px = (s + pad) & 1;
    int base = 0;
    for (int p = 0; p < 2 * py + px; ++p) base += tconv_axis(R, pad, p >> 1).cnt * tconv_axis(S, pad, p & 1).cnt;
    const TAxis ay = tconv_axis(R, pad, py), ax = tconv_axis(S, pad, px);
    return base + ((ay.rmax - r) / 2) * ax.cnt + (ax.rmax - s) / 2;
}

#ifdef __HIPCC__
__device__ inline int cdiv_dev(int a, int b) { return (a + b - 1) / b; }
// 16-byte piece p (channels 8 p .. 8 p + 7 of the chunk) of row nl in plane 0 of the weight chunk that starts at `chunk`; plane 1
// sits one plane (GB_PLANE / B_PLANE) behind
__device__ inline unsigned char *wimg_piece(unsigned char *chunk, int nl, int p) { return chunk + nl * 64 + ((p ^ ((nl >> 2) & 3)) << 4); }
// piece p of slab sl of a pixel, plane 0, in the dense planes tensor of nslab slabs at xp; plane 1 sits PLANE1 bytes behind
constexpr int PLANE1 = 64;
template <typename P>
__device__ inline P *planes_piece(P *xp, long pix, int nslab, int sl, int p)
{
    return xp + pix * (long)(nslab * SLAB) + sl * SLAB + p * 16;
}
// the eight values val(0) .. val(7) of a piece, times s (a power of two), as their two fp16 planes; val is called in order, each
// value split as it arrives
template <typename F>
__device__ inline void q_split8(F &&val, const float s, h16x8 &h0, h16x8 &h1)
{
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        hp_t x0, x1;
        q_split(val(c), s, x0, x1);
        h0[c] = x0; h1[c] = x1;
    }
}
#endif
